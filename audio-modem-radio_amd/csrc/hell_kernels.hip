// hell_kernels.hip -- Hellschreiber receiver for gfx950, batched and bit-exact:
// hellschreiber_demodulate (hellschreiber.py:155-187) for
// many captures at once.
//
//   pixel p of a stream = samples[p*sps : (p+1)*sps];  bit = np.mean(chunk ** 2) > 0.1
//   byte g = lookup[ sum(bit[7g + i] << i) ]           (first glyph with such a row, else '?')
//
// The decision is numpy's float arithmetic, so the sum runs in numpy's order
// (add.reduce's inner loop, DESIGN.md "Hellschreiber"):
//   acc = 0; per block of 8192 squares: acc = acc + pairwise(block)
//   pairwise(a, n): n <= 128 -> 8 accumulators r[k] = a[k], r[k] += a[i + k]
//                   (i = 8, 16, ... < n - n % 8), ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
//                   then the n % 8 tail serially (n < 8: serial from 0);
//                   else n2 = n/2 - (n/2) % 8: pairwise(a, n2) + pairwise(a + n2, n - n2)
// in the dtype numpy accumulates in (float32 for float32 / float16 input,
// float64 for float64 and every integer), each square rounded on its own in
// the dtype numpy squares in (integers wrap) before the add -- no fused
// multiply-add (-ffp-contract=off, and the two are separate statements).
//
// Two launches:
//   H0 k_hell_plan    the summation tree of ONE pixel -- it depends on sps
//                     only -- as a flat leaf list in post-order: (offset, length,
//                     merges after this leaf, end-of-block flag).  One lane, an
//                     explicit stack; ~sps/100 leaves.
//   H1 k_hell_energy  one wavefront per 7-pixel group (= one output byte).
//                     The wave is 8 teams of 8 lanes; a team sums one leaf at
//                     a time, lane k being accumulator k (8 consecutive
//                     elements per team and step), combines its 8 accumulators
//                     with three fixed cross-lane adds (xor 1, 2, 4: the
//                     bracketing above; IEEE addition commutes, so both
//                     partners hold the same sum) and adds the tail.  The 8
//                     leaf sums then go through the tree's merges on a small
//                     stack, every lane redundantly (uniform control flow, no
//                     barrier: each lane reads back only what it wrote).  At the
//                     default sps = 784 a pixel is exactly 8 leaves (96, 96, 96,
//                     104, 96, 96, 96, 104): one step of the 8 teams.  Threshold,
//                     7-pixel pack and the 128-entry lookup follow in the same
//                     launch; every sample is read once, with element loads
//                     (pixel starts p*sps are not 16-byte aligned).
#include <hip/hip_runtime.h>

#include "amr_internal.h"
#include "amr.h"
#include "hell.h"
#include "hell_glyphs.h"

namespace amr {

__constant__ uint8_t c_hell_glyphs[kHellGlyphs][kHellRows] = {AMR_HELL_GLYPH_TABLE};

// H0 (one block of 128 threads) -------------------------------------------
__global__ void k_hell_plan(int64_t sps, HellLeaf* __restrict__ tab, int64_t cap, int32_t* __restrict__ n_leaf,
                            uint8_t* __restrict__ lut) {
  {                                                // lut[v]: the first glyph, in code order, with a row == v
    const uint32_t v = threadIdx.x;
    uint8_t ch = '?';
    for (int g = kHellGlyphs - 1; g >= 0; --g)
      for (int r = 0; r < kHellRows; ++r)
        if (c_hell_glyphs[g][r] == v) ch = (uint8_t)(kHellFirst + g);
    if (v < 128) lut[v] = ch;
  }
  if (threadIdx.x != 0) return;
  // work items: a range still to split (len > 0) or a merge marker (len == 0)
  int32_t s_off[48], s_len[48];
  int64_t n = 0;
  for (int64_t b0 = 0; b0 < sps; b0 += kHellBlock) {
    int sp = 0;
    s_off[sp] = (int32_t)b0;
    s_len[sp++] = (int32_t)(sps - b0 < kHellBlock ? sps - b0 : kHellBlock);
    while (sp > 0) {
      --sp;
      const int32_t off = s_off[sp], len = s_len[sp];
      if (len == 0) {                              // both halves are on the value stack: one merge
        if (n > 0 && n <= cap) tab[n - 1].merges += 1;
      } else if (len <= 128) {
        if (n < cap) tab[n] = HellLeaf{off, len, 0, 0};
        ++n;
      } else {
        int32_t n2 = len / 2;
        n2 -= n2 % 8;
        s_off[sp] = 0;                             // popped last: the merge
        s_len[sp++] = 0;
        s_off[sp] = off + n2;                      // then the right half
        s_len[sp++] = len - n2;
        s_off[sp] = off;                           // first the left half
        s_len[sp++] = n2;
      }
    }
    if (n > 0 && n <= cap) tab[n - 1].block_end = 1;
  }
  *n_leaf = (int32_t)(n <= cap ? n : 0);           // cap is amr_hell_work_bytes' bound: never exceeded
}

// element types: the dtype numpy squares in -> the dtype np.mean accumulates in
template <int E>
struct HellElem;
template <>
struct HellElem<AMR_HELL_ELEM_F32> {
  using T = float;
  using Acc = float;
  static __device__ __forceinline__ Acc sq(T a) { return a * a; }
};
template <>
struct HellElem<AMR_HELL_ELEM_F64> {
  using T = double;
  using Acc = double;
  static __device__ __forceinline__ Acc sq(T a) { return a * a; }
};
template <>
struct HellElem<AMR_HELL_ELEM_F16> {
  using T = _Float16;
  using Acc = float;
  static __device__ __forceinline__ Acc sq(T a) {
    const float p = (float)a * (float)a;           // exact (22 bits); rounded once to float16, as numpy's half multiply
    return (float)(_Float16)p;
  }
};
template <typename S, typename U>
struct HellInt {                                    // wraps in its own width, then numpy's cast to float64
  using T = S;
  using Acc = double;
  static __device__ __forceinline__ Acc sq(T a) {
    const U u = (U)a;
    const U s = (U)(u * u);
    return (double)(S)s;
  }
};
template <> struct HellElem<AMR_HELL_ELEM_I8> : HellInt<int8_t, uint8_t> {};
template <> struct HellElem<AMR_HELL_ELEM_I16> : HellInt<int16_t, uint16_t> {};
template <> struct HellElem<AMR_HELL_ELEM_I32> : HellInt<int32_t, uint32_t> {};
template <> struct HellElem<AMR_HELL_ELEM_I64> : HellInt<int64_t, uint64_t> {};
template <> struct HellElem<AMR_HELL_ELEM_U8> : HellInt<uint8_t, uint8_t> {};
template <> struct HellElem<AMR_HELL_ELEM_U16> : HellInt<uint16_t, uint16_t> {};
template <> struct HellElem<AMR_HELL_ELEM_U32> : HellInt<uint32_t, uint32_t> {};
template <> struct HellElem<AMR_HELL_ELEM_U64> : HellInt<uint64_t, uint64_t> {};
template <>
struct HellElem<AMR_HELL_ELEM_PCM16> {              // pcm / 32768 as float64 (decoder._Pcm16): the square is exact
  using T = int16_t;
  using Acc = double;
  static __device__ __forceinline__ Acc sq(T a) {
    const double x = (double)a / 32768.0;
    return x * x;
  }
};

// float64 -> float16, rounded once (np.float16(float64)): through float32
// rounded to odd, which keeps the sticky information the second rounding needs.
__device__ __forceinline__ _Float16 half_from_double(double q) {
  float f = (float)q;
  const double d = (double)f;
  if (d != q && q == q) {                          // inexact (q finite): truncate, then set the sticky last bit
    uint32_t u = __float_as_uint(f);
    if (fabs(d) > fabs(q)) u -= 1;                 // back to the neighbour towards zero (from inf: FLT_MAX)
    f = __uint_as_float(u | 1u);
  }
  return (_Float16)f;
}

// np.mean's quotient and result dtype (sum / np.intp(sps) is a float64
// division in numpy 2, then cast to the result dtype), the threshold numpy
// compares against, and the energy widened exactly to float64.
template <int E>
__device__ __forceinline__ bool hell_decide(typename HellElem<E>::Acc sum, int64_t sps, double* e) {
  const double q = (double)sum / (double)sps;
  if (E == AMR_HELL_ELEM_F32) {
    const float m = (float)q;
    *e = (double)m;
    return m > 0.1f;                                // np.float32(m) > 0.1: the Python float is weak
  }
  if (E == AMR_HELL_ELEM_F16) {
    const float m = (float)half_from_double(q);
    *e = (double)m;
    return m > 0.0999755859375f;                    // float16(0.1)
  }
  *e = q;
  return q > 0.1;
}

// H1 -----------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(kHellThreads) void k_hell_energy(
    const typename HellElem<E>::T* __restrict__ x, int64_t x_stride, int64_t n_streams, int64_t sps, int64_t n_pix,
    int64_t n_groups, const HellLeaf* __restrict__ tab, const int32_t* __restrict__ n_leaf_p,
    const uint8_t* __restrict__ lut, uint8_t* __restrict__ out, int64_t out_stride, int64_t* __restrict__ out_len,
    double* __restrict__ energy) {
  using EL = HellElem<E>;
  using Acc = typename EL::Acc;
  __shared__ Acc s_stack[kHellThreads / kWave][kHellStack];
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  const int team = lane >> 3, k = lane & 7;
  const int64_t w = (int64_t)blockIdx.x * (kHellThreads / kWave) + wave;   // wave-uniform
  if (w >= n_streams * n_groups) return;
  const int64_t s = w / n_groups, g = w - s * n_groups;
  const int n_leaf = *n_leaf_p;
  Acc* __restrict__ stk = s_stack[wave];
  const typename EL::T* __restrict__ row = x + s * x_stride;
  const int64_t p_end = (7 * g + 7 < n_pix) ? 7 * g + 7 : n_pix;
  uint32_t v = 0;
  for (int64_t p = 7 * g; p < p_end; ++p) {
    const typename EL::T* __restrict__ px = row + p * sps;                // p < n_pix: px[0 .. sps) lies in the row
    Acc acc = (Acc)0;
    int sp = 0;
    for (int l0 = 0; l0 < n_leaf; l0 += 8) {
      // ---- each team: one leaf
      const int li = l0 + team;
      int32_t off = 0, len = 0;
      if (li < n_leaf) {
        off = tab[li].off;
        len = tab[li].len;
      }
      const typename EL::T* __restrict__ a = px + off;
      const int32_t m = len - (len & 7);
      Acc r = (Acc)0;
      if (m > 0) r = EL::sq(a[k]);                                        // r[k] = a[k]
#pragma unroll 4
      for (int32_t i = 8; i < m; i += 8) {
        const Acc q = EL::sq(a[i + k]);
        r = r + q;                                                        // r[k] += a[i + k]
      }
      // every lane takes part (a team without a full 8 holds zeros: 0 + 0 = 0, the serial sum's start)
      r = r + __shfl_xor(r, 1);                                           // r0+r1 | r2+r3 | r4+r5 | r6+r7
      r = r + __shfl_xor(r, 2);                                           // (r0+r1)+(r2+r3) | (r4+r5)+(r6+r7)
      r = r + __shfl_xor(r, 4);                                           // the leaf's 8-accumulator sum
      for (int32_t i = m; i < len; ++i) {                                 // tail (or all of a leaf < 8), serially
        const Acc q = EL::sq(a[i]);
        r = r + q;
      }
      // ---- the tree: every lane walks the 8 leaf sums in order
      const int cnt = n_leaf - l0 < 8 ? n_leaf - l0 : 8;
      for (int t = 0; t < cnt; ++t) {
        const Acc leaf = __shfl(r, 8 * t);
        const int32_t merges = tab[l0 + t].merges;
        const int32_t bend = tab[l0 + t].block_end;
        stk[sp < kHellStack ? sp : kHellStack - 1] = leaf;
        ++sp;
        for (int32_t j = 0; j < merges && sp >= 2; ++j) {
          --sp;
          const Acc right = stk[sp], left = stk[sp - 1];
          stk[sp - 1] = left + right;                                     // pairwise(a, n2) + pairwise(a + n2, n - n2)
        }
        if (bend) {
          const Acc blk = stk[0];
          acc = acc + blk;                                                // acc = acc + pairwise(block)
          sp = 0;
        }
      }
    }
    double e;
    const bool bit = hell_decide<E>(acc, sps, &e);
    v |= (bit ? 1u : 0u) << (uint32_t)(p - 7 * g);
    if (energy && lane == 0) energy[s * n_pix + p] = e;
  }
  if (lane == 0) {
    if (p_end - 7 * g == 7) out[s * out_stride + g] = lut[v & 127u];      // g < n_pix / 7 <= out_stride
    if (g == 0) out_len[s] = n_pix / 7;
  }
}

template <int E>
static void launch_energy(const void* x, int64_t x_stride, int64_t n_streams, int64_t sps, int64_t n_pix,
                          int64_t n_groups, const HellLeaf* tab, const int32_t* n_leaf, const uint8_t* lut,
                          uint8_t* out, int64_t out_stride, int64_t* out_len, double* energy, hipStream_t st) {
  const int64_t waves = n_streams * n_groups;
  const int per = kHellThreads / kWave;
  hipLaunchKernelGGL((k_hell_energy<E>), dim3((unsigned)((waves + per - 1) / per)), dim3(kHellThreads), 0, st,
                     (const typename HellElem<E>::T*)x, x_stride, n_streams, sps, n_pix, n_groups, tab, n_leaf, lut, out,
                     out_stride, out_len, energy);
}

__global__ void k_hell_zero_len(int64_t* __restrict__ out_len, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out_len[i] = 0;
}

// work: [HellLeaf x hell_leaf_cap(sps)][int32 n_leaf (16 B)][lut 128 B] = hell_work_bytes(sps) (hell.h)
hipError_t launch_hell(int elem, const void* x, int64_t x_stride, int64_t n_streams, int64_t n_samples, int64_t sps,
                       uint8_t* out, int64_t out_stride, int64_t* out_len, double* energy, void* work,
                       hipStream_t st) {
  if (n_streams <= 0) return hipSuccess;
  const int64_t n_pix = sps > 0 ? n_samples / sps : 0;
  // with an energy buffer the trailing pixels of an incomplete group are summed too
  const int64_t n_groups = energy ? (n_pix + 6) / 7 : n_pix / 7;
  if (n_groups == 0) {
    hipLaunchKernelGGL(k_hell_zero_len, dim3((unsigned)((n_streams + 255) / 256)), dim3(256), 0, st, out_len, n_streams);
    return hipGetLastError();
  }
  const int64_t cap = hell_leaf_cap(sps);
  HellLeaf* tab = (HellLeaf*)work;
  int32_t* n_leaf = (int32_t*)((char*)work + cap * (int64_t)sizeof(HellLeaf));
  uint8_t* lut = (uint8_t*)n_leaf + 16;
  hipLaunchKernelGGL(k_hell_plan, dim3(1), dim3(128), 0, st, sps, tab, cap, n_leaf, lut);
#define AMR_HELL_CASE(E)                                                                                       \
  case E:                                                                                                      \
    launch_energy<E>(x, x_stride, n_streams, sps, n_pix, n_groups, tab, n_leaf, lut, out, out_stride, out_len, \
                     energy, st);                                                                              \
    break;
  switch (elem) {
    AMR_HELL_CASE(AMR_HELL_ELEM_F32)
    AMR_HELL_CASE(AMR_HELL_ELEM_F64)
    AMR_HELL_CASE(AMR_HELL_ELEM_F16)
    AMR_HELL_CASE(AMR_HELL_ELEM_I8)
    AMR_HELL_CASE(AMR_HELL_ELEM_I16)
    AMR_HELL_CASE(AMR_HELL_ELEM_I32)
    AMR_HELL_CASE(AMR_HELL_ELEM_I64)
    AMR_HELL_CASE(AMR_HELL_ELEM_U8)
    AMR_HELL_CASE(AMR_HELL_ELEM_U16)
    AMR_HELL_CASE(AMR_HELL_ELEM_U32)
    AMR_HELL_CASE(AMR_HELL_ELEM_U64)
    AMR_HELL_CASE(AMR_HELL_ELEM_PCM16)
    default:
      return hipErrorInvalidValue;
  }
#undef AMR_HELL_CASE
  return hipGetLastError();
}

}  // namespace amr
