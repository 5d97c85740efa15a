// rs_kernels.hip -- the Reed-Solomon code of fec.ReedSolomonCodec on the GPU:
// systematic RS(255, 255 - nsym) over GF(2^8) (0x11D, alpha = 2, roots alpha^0 ..),
// shortened last block, block interleave as an index mapping, errors-and-erasures
// decoding.  DESIGN §3h states the code and why a block's failure is detected
// completely.
//
// One wavefront per block, no LDS, no barrier: each wave runs its own block's
// length, so ragged rows in one launch cannot wait on one another.  The field
// arithmetic is shift/xor in registers; nothing on a per-byte path looks a table
// up in memory.
//
// k_rs_encode: lane j holds the LFSR's parity byte j.  A message byte costs one
// lane read of the feedback byte, one cross-lane shift and a multiply of the
// lane's generator coefficient by the (wave-uniform) feedback byte.
//
// k_rs_decode: the block sits in registers, four bytes to a lane (coalesced when
// not interleaved).  Lane j forms syndrome j by Horner, as four chains over four
// segments of the block packed in one register, so a step multiplies four partial
// sums by alpha^j at once (with nsym <= 32 the two half-waves take half the block
// each); with all syndromes zero and nothing erased the wave copies the message
// out and exits.  Otherwise: erasure locator, inversion-free
// Berlekamp-Massey with the locator across the lanes, Chien search and Forney with
// positions across the lanes, and a second syndrome pass over the corrected word.
#include <hip/hip_runtime.h>

#include "rs.h"

namespace amr {
namespace {

__device__ __forceinline__ int rdlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
// lane l's value of v, for a source lane in 0 .. 63
__device__ __forceinline__ int from_lane(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }
// x * p(x) with the coefficients across the lanes: lane l takes lane l - 1's, lane 0 takes 0
__device__ __forceinline__ int shift_up(int v, int lane) {
  const int r = from_lane(v, (lane - 1) & 63);
  return lane == 0 ? 0 : r;
}
__device__ __forceinline__ int xor_reduce(int v, int lane) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v ^= from_lane(v, lane ^ off);
  return __builtin_amdgcn_readfirstlane(v);
}

// ---- GF(2^8), 0x11D ------------------------------------------------------------
__host__ __device__ constexpr int gf_xtime(int a) { return ((a << 1) ^ ((a & 0x80) ? kRsPoly : 0)) & 0xFF; }
__host__ __device__ constexpr int gf_mul(int a, int b) {
  int r = 0;
  for (int i = 0; i < 8; ++i) {
    r ^= a & -((b >> i) & 1);
    a = gf_xtime(a);
  }
  return r;
}
__host__ __device__ constexpr int gf_sq_n(int a, int n) {
  for (int i = 0; i < n; ++i) a = gf_mul(a, a);
  return a;
}
// alpha^e for 0 <= e <= 255: the product of alpha^(2^b) over e's bits
__device__ __forceinline__ int gf_exp(int e) {
  constexpr int a2[8] = {gf_sq_n(2, 0), gf_sq_n(2, 1), gf_sq_n(2, 2), gf_sq_n(2, 3),
                         gf_sq_n(2, 4), gf_sq_n(2, 5), gf_sq_n(2, 6), gf_sq_n(2, 7)};
  int r = 1;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int t = gf_mul(r, a2[b]);
    r = ((e >> b) & 1) ? t : r;
  }
  return r;
}
// a^254 = 1 / a (0 for 0)
__device__ __forceinline__ int gf_inv(int a) {
  int s = gf_mul(a, a), r = s;                     // a^2
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    s = gf_mul(s, s);                              // a^4 .. a^128
    r = gf_mul(r, s);
  }
  return r;
}
// c's multiples c * 2^b: with them a product c * v is the xor of t[b] over v's set bits
__device__ __forceinline__ void gf_multiples(int c, int (&t)[8]) {
  t[0] = c;
#pragma unroll
  for (int b = 1; b < 8; ++b) t[b] = gf_xtime(t[b - 1]);
}
__device__ __forceinline__ int gf_mul_t(const int (&t)[8], int v) {
  int r = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b) r ^= t[b] & -((v >> b) & 1);
  return r;
}

// lane j's syndrome j of the word d (byte c in lane c & 63 of d[c >> 6]), by Horner: sum_c d_c alpha^(j (len - 1 - c));
// t = the multiples of alpha^lane
__device__ __forceinline__ int syndromes(const int (&d)[4], int len, const int (&t)[8], int lane, int nsym) {
  int s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int cnt = len - 64 * q < 64 ? len - 64 * q : 64;
    for (int i = 0; i < cnt; ++i) s = gf_mul_t(t, s) ^ rdlane(d[q], i);
  }
  return lane < nsym ? s : 0;
}

__global__ __launch_bounds__(kRsThreads) void k_rs_encode(const uint8_t* __restrict__ in, int64_t in_stride,
                                                          const int64_t* __restrict__ in_len, int64_t n_rows,
                                                          int64_t nb_max, int nsym, int I, RsGen gen,
                                                          uint8_t* __restrict__ out, int64_t out_stride,
                                                          int64_t* __restrict__ out_len) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (kRsThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= n_rows * nb_max) return;
  const int64_t row = w / nb_max, B = w - row * nb_max;
  const int64_t n = uniform64(in_len[row]);
  const int k = kRsN - nsym;
  // every bound below derives from n, and n is checked against the row and the output row
  const bool ok = n >= 0 && n <= in_stride && rs_encoded_len(n, nsym) <= out_stride;
  if (!ok) {
    if (B == 0 && lane == 0) out_len[row] = -1;
    return;
  }
  const int64_t nblk = rs_ceil_div(n, k);
  if (B == 0 && lane == 0) out_len[row] = n + nblk * nsym;
  if (B >= nblk) return;
  const int mlen = n - B * k < k ? (int)(n - B * k) : k;           // this block's message bytes, 1 .. k
  const int last_len = (int)(n - (nblk - 1) * k) + nsym;           // the last block's codeword
  const uint8_t* src = in + row * in_stride + B * k;
  uint8_t* dst = out + row * out_stride;

  int t[8];
  gf_multiples(lane < nsym ? gen.g[lane] : 0, t);                  // lanes past nsym hold 0 throughout
  int reg = 0;
  for (int c0 = 0; c0 < mlen; c0 += 64) {
    const int c = c0 + lane;
    int m = 0;
    if (c < mlen) {
      m = src[c];
      dst[rs_stream_pos(B, c, I, nblk, last_len)] = (uint8_t)m;    // systematic: the message first
    }
    const int cnt = mlen - c0 < 64 ? mlen - c0 : 64;
    for (int i = 0; i < cnt; ++i) {
      const int fb = rdlane(m, i) ^ rdlane(reg, 0);
      const int nx = from_lane(reg, (lane + 1) & 63);
      reg = (lane < nsym - 1 ? nx : 0) ^ gf_mul_t(t, fb);
    }
  }
  if (lane < nsym) dst[rs_stream_pos(B, mlen + lane, I, nblk, last_len)] = (uint8_t)reg;
}

__global__ __launch_bounds__(kRsThreads) void k_rs_decode(const uint8_t* __restrict__ in, int64_t in_stride,
                                                          const int64_t* __restrict__ in_len,
                                                          const uint8_t* __restrict__ erase, int64_t n_rows,
                                                          int64_t nb_max, int nsym, int I, uint8_t* __restrict__ out,
                                                          int64_t out_stride, int64_t* __restrict__ out_len,
                                                          int32_t* __restrict__ corrected,
                                                          int32_t* __restrict__ failed) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (kRsThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (w >= n_rows * nb_max) return;
  const int64_t row = w / nb_max, B = w - row * nb_max;
  const int64_t L = uniform64(in_len[row]);
  // every bound below derives from L, and L is checked against the row, the output row and nsym
  const bool ok = L >= 0 && L <= in_stride && rs_valid_len(L, nsym) && rs_decoded_len(L, nsym) <= out_stride;
  if (!ok) {
    if (B == 0 && lane == 0) {
      out_len[row] = 0;
      corrected[row] = 0;
      failed[row] = -1;
    }
    return;
  }
  const int64_t nblk = rs_ceil_div(L, kRsN);
  if (B == 0 && lane == 0) out_len[row] = L - nblk * nsym;
  if (B >= nblk) return;
  const int last_len = (int)(L - kRsN * (nblk - 1));
  const int len = B == nblk - 1 ? last_len : kRsN;                 // nsym + 1 .. 255
  const int mlen = len - nsym;
  const uint8_t* rin = in + row * in_stride;
  const uint8_t* rer = erase ? erase + row * in_stride : nullptr;
  uint8_t* dst = out + row * out_stride + B * (kRsN - nsym);

  // ---- syndromes, four Horner chains to a lane -------------------------------------
  // The block behind leading zeros is nseg segments of m = ceil(len / nseg) bytes.  With nsym > 32 the wave
  // is one group of 64 lanes and nseg = 4; with nsym <= 32 it is two groups of 32, each with its own four of
  // nseg = 8 segments, so no lane idles.  Lane il < m of a group holds byte il of the group's four segments,
  // one to a byte of p4 (erased bytes as 0).  A step reads one lane's four bytes per group and multiplies the
  // lane's four partial sums by alpha^il at once; the sums then combine through powers of alpha^(il m).
  const bool two = nsym <= 32;
  const int il = two ? lane & 31 : lane, h = two ? lane >> 5 : 0;
  const int nseg = two ? 8 : 4;
  const int m = (len + nseg - 1) / nseg, pad = nseg * m - len;     // m <= the group's lanes
  uint32_t p4 = 0;
  int f = 0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = (4 * h + s) * m + il - pad;                      // < len
    int v = 0;
    bool e = false;
    if (il < m && c >= 0) {
      const int64_t p = rs_stream_pos(B, c, I, nblk, last_len);
      v = rin[p];
      e = rer && rer[p] != 0;
    }
    f += __popcll(__ballot(e));
    p4 |= (uint32_t)(e ? 0 : v) << (8 * s);
  }
  int t[8];
  gf_multiples(gf_exp(il), t);                                     // alpha^lane in every lane below nsym
  int S;
  {
    uint32_t t4[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) t4[b] = (uint32_t)t[b] * 0x01010101u;
    uint32_t s4 = 0;
    for (int i = 0; i < m; ++i) {
      uint32_t r = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b) r ^= t4[b] & (((s4 >> b) & 0x01010101u) * 0xFFu);
      const int x0 = rdlane((int)p4, i), x1 = rdlane((int)p4, (i + 32) & 63);
      s4 = r ^ (uint32_t)(h ? x1 : x0);
    }
    const int g = gf_exp(il * m % 255);
    S = (int)(s4 & 0xFF);
#pragma unroll
    for (int s = 1; s < 4; ++s) S = gf_mul(S, g) ^ (int)((s4 >> (8 * s)) & 0xFF);
    if (two) {                                                     // the first group's segments lie four segments higher
      const int g2 = gf_mul(g, g);
      S = gf_mul(S, gf_mul(g2, g2)) ^ from_lane(S, lane ^ 32);
    }
    S = lane < nsym ? S : 0;
  }
  if (f == 0 && __ballot(S != 0) == 0) {                           // the clean path: copy the message through
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = (4 * h + s) * m + il - pad;
      if (il < m && c >= 0 && c < mlen) dst[c] = (uint8_t)(p4 >> (8 * s));
    }
    return;
  }

  // ---- the block again, byte c in lane c & 63: o as received, d with the erased bytes zeroed ----
  int o[4], d[4];
  bool er[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = 64 * q + lane;
    o[q] = 0;
    er[q] = false;
    if (c < len) {
      const int64_t p = rs_stream_pos(B, c, I, nblk, last_len);
      o[q] = rin[p];
      er[q] = rer && rer[p] != 0;
    }
    d[q] = er[q] ? 0 : o[q];
  }

  bool fail = f > nsym;
  int cw[4] = {d[0], d[1], d[2], d[3]};
  if (!fail) {
    // ---- locators X = alpha^(len - 1 - c) and their inverses, per position ----------
    int X[4], Xi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 64 * q + lane;
      const int ex = c < len ? len - 1 - c : 0;
      X[q] = gf_exp(ex);
      Xi[q] = gf_exp(ex ? 255 - ex : 0);
    }
    // ---- erasure locator prod (1 - X x): coefficient i in lane i, coefficient 64 (f = nsym = 64 only) in top ----
    int psi = lane == 0 ? 1 : 0, top = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned long long m = __ballot(er[q]);
      while (m) {
        const int i = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int x = rdlane(X[q], i);
        top ^= gf_mul(x, rdlane(psi, 63));
        psi ^= gf_mul(x, shift_up(psi, lane));
      }
    }
    // ---- Berlekamp-Massey without inversions, started from the erasure locator --------
    // A decodable block ends with lr = e + f <= (nsym + f) / 2 <= 63 (f < nsym here), and lr never shrinks:
    // past that bound the block has failed, and below it no coefficient leaves the 64 lanes.
    int lr = f;
    {
      int bp = psi, gamma = 1;
      for (int r = f; r < nsym && !fail; ++r) {
        bp = shift_up(bp, lane);
        const int sv = from_lane(S, (r - lane) & 63);
        const int delta = xor_reduce(gf_mul(psi, lane <= r ? sv : 0), lane);
        if (delta) {
          const int nx = gf_mul(gamma, psi) ^ gf_mul(delta, bp);
          if (2 * lr <= r + f) {
            bp = psi;
            gamma = delta;
            lr = r + 1 - lr + f;
            fail = 2 * lr > nsym + f;
          }
          psi = nx;
        }
      }
    }
    if (!fail) {
      // ---- evaluator omega = S psi mod x^nsym, coefficient i in lane i -----------------
      int om = 0;
      {
        int ss = S;
        const int hi = lr < 63 ? lr : 63;                          // coefficient 64 cannot reach below x^64
        for (int b = 0; b <= hi; ++b) {
          om ^= gf_mul(rdlane(psi, b), ss);
          ss = shift_up(ss, lane);
        }
        om = lane < nsym ? om : 0;
      }
      // ---- Chien search and Forney, positions across the lanes ---------------------
      int nroots = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (64 * q < len) {
          const int c = 64 * q + lane;
          const int xi = Xi[q], y = gf_mul(xi, xi);
          // psi(x) = E(x^2) + x O(x^2) and psi'(x) = O(x^2): both from one Horner pass in y = x^2
          int E = 0, O = 0;
          for (int i = lr; i >= 0; --i) {
            const int lo = rdlane(psi, i & 63);
            const int coef = i == 64 ? top : lo;
            if (i & 1) O = gf_mul(O, y) ^ coef;
            else E = gf_mul(E, y) ^ coef;
          }
          const bool root = c < len && (E ^ gf_mul(xi, O)) == 0;
          nroots += __popcll(__ballot(root));
          int ov = 0;
          for (int i = nsym - 1; i >= 0; --i) ov = gf_mul(ov, xi) ^ rdlane(om, i);
          const int ev = gf_mul(gf_mul(X[q], ov), gf_inv(O));      // the error value X omega(1/X) / psi'(1/X)
          cw[q] = root ? d[q] ^ ev : d[q];
        }
      }
      fail = nroots != lr;                                         // every root of the locator lies inside the block
    }
    if (!fail) {
      // the corrected word is a codeword, and it lies within the bound 2 e + f <= nsym
      const int S2 = syndromes(cw, len, t, lane, nsym);
      int e = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) e += __popcll(__ballot(64 * q + lane < len && !er[q] && cw[q] != o[q]));
      fail = __ballot(S2 != 0) != 0 || 2 * e + f > nsym;
    }
  }
  int nfix = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = 64 * q + lane;
    const int v = fail ? o[q] : cw[q];                             // a failed block passes through as received
    nfix += __popcll(__ballot(c < len && v != o[q]));
    if (c < mlen) dst[c] = (uint8_t)v;
  }
  if (lane == 0) {
    if (fail) atomicAdd(&failed[row], 1);
    else if (nfix) atomicAdd(&corrected[row], nfix);
  }
}

}  // namespace

hipError_t launch_rs_encode(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, int nsym,
                            int interleave, uint8_t* out, int64_t out_stride, int64_t* out_len, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int per = kRsThreads / 64;
  const int64_t nb_max = in_stride > 0 ? rs_ceil_div(in_stride, kRsN - nsym) : 1;   // block 0's wave reports the row
  hipLaunchKernelGGL(k_rs_encode, dim3((unsigned)((n * nb_max + per - 1) / per)), dim3(kRsThreads), 0, st, in,
                     in_stride, in_len, n, nb_max, nsym, interleave, rs_generator(nsym), out, out_stride, out_len);
  return hipGetLastError();
}

hipError_t launch_rs_decode(const uint8_t* in, int64_t in_stride, const int64_t* in_len, const uint8_t* erase,
                            int64_t n, int nsym, int interleave, uint8_t* out, int64_t out_stride, int64_t* out_len,
                            int32_t* corrected, int32_t* failed, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(corrected, 0, (size_t)n * 4, st);  // the blocks of a row add to them
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(failed, 0, (size_t)n * 4, st);
  if (e != hipSuccess) return e;
  const int per = kRsThreads / 64;
  const int64_t nb_max = in_stride > 0 ? rs_ceil_div(in_stride, kRsN) : 1;
  hipLaunchKernelGGL(k_rs_decode, dim3((unsigned)((n * nb_max + per - 1) / per)), dim3(kRsThreads), 0, st, in,
                     in_stride, in_len, erase, n, nb_max, nsym, interleave, out, out_stride, out_len, corrected,
                     failed);
  return hipGetLastError();
}

}  // namespace amr
