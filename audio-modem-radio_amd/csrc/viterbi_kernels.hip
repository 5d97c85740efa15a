// viterbi_kernels.hip -- the rate-1/2, K=7 convolutional code of fec.py:72-111
// (171/133 octal) on the GPU: a maximum-likelihood hard-decision Viterbi
// decoder, its soft-input form (k_viterbi_soft) and the batched
// encoder.  DESIGN §3f states the code and the rules that make the decoder's
// output unique.
//
// k_viterbi: one wavefront per codeword, lane = the state AFTER a step (64
// states, 64 lanes).  A step reads the two predecessors' path metrics with two
// cross-lane reads, adds the branch metrics, and the 64 add-compare-select
// decisions are one __ballot.  The lane numbered t & 63 keeps step t's survivor
// word; every 64 steps the wave stores the block (512 bytes, coalesced) to its
// slice of the workspace.  The traceback walks the blocks backwards: every lane
// reloads the word it stored itself, and the wave-uniform state follows the
// decisions through lane reads.  No LDS, no barrier: each wave runs its own
// length, so ragged lengths in one launch cannot wait on one another.
#include <hip/hip_runtime.h>

#include "viterbi.h"

namespace amr {
namespace {

__device__ __forceinline__ int rdlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// one trellis step for the wave: ab = the step's two received bits (wave-uniform)
// o0 = this lane's p0-branch output bits, a0 / a1 = byte addresses of lanes p0 / p1
__device__ __forceinline__ uint64_t acs(int32_t& pm, int ab, int o0, int a0, int a1) {
  const int bm0 = __popc(o0 ^ ab);                 // Hamming distance of the p0 branch; the p1 branch's is 2 - bm0
  const int32_t c0 = __builtin_amdgcn_ds_bpermute(a0, pm) + bm0;
  const int32_t c1 = __builtin_amdgcn_ds_bpermute(a1, pm) + (2 - bm0);
  const bool d = c1 < c0;                          // strictly smaller: a tie keeps p0
  pm = d ? c1 : c0;
  return __ballot(d);
}

// the traceback from state 0 at step T, shared by k_viterbi and k_viterbi_soft: ws = the codeword's
// survivor blocks, orow = its output row
__device__ __forceinline__ void traceback(const uint64_t* __restrict__ ws, int nfull, int tail, int lane,
                                          uint8_t* __restrict__ orow, int64_t n_msg) {
  uint32_t s = 0;                                  // wave-uniform: the state after step t
  for (int b = nfull; b >= 0; --b) {
    const uint64_t wv = ws[(int64_t)b * 64 + lane];   // the word this lane stored itself
    const int wlo = (int)(uint32_t)wv, whi = (int)(uint32_t)(wv >> 32);
    uint64_t acc = 0;                              // decoded bit of step 64 b + i at bit 63 - i
    if (b < nfull) {
#pragma unroll
      for (int i = 63; i >= 0; --i) {
        const uint64_t w = ((uint64_t)(uint32_t)rdlane(whi, i) << 32) | (uint32_t)rdlane(wlo, i);
        acc |= (uint64_t)(s & 1) << (63 - i);
        s = (s >> 1) | ((uint32_t)((w >> s) & 1) << 5);
      }
    } else {
      for (int i = tail - 1; i >= 0; --i) {
        const uint64_t w = ((uint64_t)(uint32_t)rdlane(whi, i) << 32) | (uint32_t)rdlane(wlo, i);
        acc |= (uint64_t)(s & 1) << (63 - i);
        s = (s >> 1) | ((uint32_t)((w >> s) & 1) << 5);
      }
    }
    const int64_t ob = (int64_t)b * 8 + lane;      // blocks start at multiples of 64 steps = 8 output bytes
    if (lane < 8 && ob < n_msg) orow[ob] = (uint8_t)(acc >> (56 - 8 * lane));   // the 6 flush bits lie past n_msg
  }
}

__global__ __launch_bounds__(kVitThreads) void k_viterbi(const uint8_t* __restrict__ in, int64_t in_stride,
                                                         const int64_t* __restrict__ in_len, int64_t n_cw,
                                                         uint8_t* __restrict__ out, int64_t out_stride,
                                                         int64_t* __restrict__ out_len, int32_t* __restrict__ metric,
                                                         uint64_t* __restrict__ work, int64_t work_words) {
  const int lane = threadIdx.x & 63;
  const int64_t cw = (int64_t)blockIdx.x * (kVitThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (cw >= n_cw) return;
  const int64_t L = uniform64(in_len[cw]);
  // every bound below derives from L, and L is checked against the row, the output row and the workspace slice
  const bool ok = L >= 2 && L <= kVitMaxLen && (L & 1) == 0 && L <= in_stride && (L - 2) / 2 <= out_stride &&
                  ((4 * L - 2 + 63) / 64) * 64 <= work_words;
  if (!ok) {
    if (lane == 0) {
      out_len[cw] = 0;
      metric[cw] = -1;
    }
    return;
  }
  const uint8_t* row = in + cw * in_stride;
  uint64_t* ws = work + cw * work_words;
  const int64_t n_msg = (L - 2) / 2;
  const int T = (int)(4 * L - 2);                  // 8 n + 6 steps; T % 64 is never 0, so the last block is partial
  const int nfull = T >> 6, tail = T & 63;

  // ---- forward pass ----------------------------------------------------------
  const int o0 = ((__popc(lane & kVitG1) & 1) << 1) | (__popc(lane & kVitG2) & 1);   // register r0 = lane (bit 6 clear)
  const int a0 = (lane >> 1) << 2, a1 = a0 + (32 << 2);
  int32_t pm = lane == 0 ? 0 : kVitInf;
  int klo = 0, khi = 0;                            // the survivor word this lane keeps
  int bytev = 0;                                   // 64 received bytes = 256 steps, one per lane
  for (int b = 0; b <= nfull; ++b) {
    if ((b & 3) == 0) {
      const int64_t idx = (int64_t)(b >> 2) * 64 + lane;
      int v = idx < L ? row[idx] : 0;
      if (idx == L - 1) v = (v & 0x0F) << 4;       // the last byte holds 4 bits right-aligned; its high nibble is ignored
      bytev = v;
    }
    const int bb = __builtin_amdgcn_ds_bpermute((((b & 3) << 4) + (lane & 15)) << 2, bytev);   // this block's 16 bytes
    if (b < nfull) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int by = rdlane(bb, j);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint64_t w = acs(pm, (by >> (6 - 2 * k)) & 3, o0, a0, a1);
          klo = lane == 4 * j + k ? (int)(uint32_t)w : klo;
          khi = lane == 4 * j + k ? (int)(uint32_t)(w >> 32) : khi;
        }
      }
    } else {
      for (int i = 0; i < tail; ++i) {
        const int by = rdlane(bb, i >> 2);
        const uint64_t w = acs(pm, (by >> (6 - 2 * (i & 3))) & 3, o0, a0, a1);
        if (lane == i) {
          klo = (int)(uint32_t)w;
          khi = (int)(uint32_t)(w >> 32);
        }
      }
    }
    ws[(int64_t)b * 64 + lane] = ((uint64_t)(uint32_t)khi << 32) | (uint32_t)klo;
  }
  if (lane == 0) {
    out_len[cw] = n_msg;
    metric[cw] = pm;                               // state 0 at step T
  }

  // ---- traceback from state 0 at step T ---------------------------------------
  traceback(ws, nfull, tail, lane, out + cw * out_stride, n_msg);
}

// ---- V2: soft input -------------------------------------------------
// The same trellis, tie rule, survivor blocks and traceback as k_viterbi; only the
// branch metric differs: for a step's soft pair (r1, r2) a branch with outputs
// (c1, c2) costs [c1 != (r1 > 0)] |r1| + [c2 != (r2 > 0)] |r2|.  The lane that
// loads a step's pair (one pair per lane and 64-step block: 128 consecutive
// bytes per wave, no load inside a step) forms the four candidate costs for
// c1c2 = 00, 01, 10, 11 once, a byte each in one dword; a step makes that dword
// wave-uniform with one lane read, and every lane takes its p0 cost at byte o0
// and its p1 cost -- the complementary outputs -- at byte 3 - o0.
__device__ __forceinline__ uint32_t soft_costs(int r1, int r2) {
  r1 = r1 < -127 ? -127 : r1;                      // -128 counts as -127
  r2 = r2 < -127 ? -127 : r2;
  const uint32_t a1 = (uint32_t)(r1 < 0 ? -r1 : r1), a2 = (uint32_t)(r2 < 0 ? -r2 : r2);
  const uint32_t x10 = r1 > 0 ? a1 : 0u, x11 = a1 - x10;   // the first value's cost against c1 = 0 / 1 (an erasure: 0, 0)
  const uint32_t x20 = r2 > 0 ? a2 : 0u, x21 = a2 - x20;
  return (x10 + x20) | ((x10 + x21) << 8) | ((x11 + x20) << 16) | ((x11 + x21) << 24);   // each <= 254
}

// k4 = the step's four costs (wave-uniform), sh0 / sh1 = 8 * o0 / 8 * (3 - o0)
__device__ __forceinline__ uint64_t acs_soft(int32_t& pm, uint32_t k4, int sh0, int sh1, int a0, int a1) {
  const int32_t c0 = __builtin_amdgcn_ds_bpermute(a0, pm) + (int32_t)((k4 >> sh0) & 255u);
  const int32_t c1 = __builtin_amdgcn_ds_bpermute(a1, pm) + (int32_t)((k4 >> sh1) & 255u);
  const bool d = c1 < c0;                          // strictly smaller: a tie keeps p0
  pm = d ? c1 : c0;
  return __ballot(d);
}

__global__ __launch_bounds__(kVitThreads) void k_viterbi_soft(const int8_t* __restrict__ in, int64_t in_stride,
                                                              int64_t in_offset, const int64_t* __restrict__ in_len,
                                                              int64_t n_cw, uint8_t* __restrict__ out,
                                                              int64_t out_stride, int64_t* __restrict__ out_len,
                                                              int32_t* __restrict__ metric,
                                                              uint64_t* __restrict__ work, int64_t work_words) {
  const int lane = threadIdx.x & 63;
  const int64_t cw = (int64_t)blockIdx.x * (kVitThreads / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (cw >= n_cw) return;
  const int64_t nv = uniform64(in_len[cw]);
  const int64_t steps = vit_soft_steps(nv);        // 0: not a soft row length (or past the maximum)
  // every bound below derives from nv, and nv is checked against the row, the output row and the workspace slice
  const bool ok = steps > 0 && in_offset >= 0 && nv <= in_stride - in_offset && (steps - 6) / 8 <= out_stride &&
                  (steps + 63) / 64 * 64 <= work_words;
  if (!ok) {
    if (lane == 0) {
      out_len[cw] = 0;
      metric[cw] = -1;
    }
    return;
  }
  const int8_t* row = in + cw * in_stride + in_offset;
  uint64_t* ws = work + cw * work_words;
  const int T = (int)steps;                        // 8 n + 6: T % 64 is never 0, so the last block is partial
  const int64_t n_msg = (steps - 6) / 8;
  const int nfull = T >> 6, tail = T & 63;
  // coded bit c is value c, but in the byte image the last four sit four values on (past the skipped nibble)
  const int64_t cut = (nv & 15) == 0 ? nv - 8 : nv;

  // ---- forward pass ----------------------------------------------------------
  const int o0 = ((__popc(lane & kVitG1) & 1) << 1) | (__popc(lane & kVitG2) & 1);
  const int sh0 = 8 * o0, sh1 = 24 - sh0;
  const int a0 = (lane >> 1) << 2, a1 = a0 + (32 << 2);
  int32_t pm = lane == 0 ? 0 : kVitInf;
  int klo = 0, khi = 0;                            // the survivor word this lane keeps
  for (int b = 0; b <= nfull; ++b) {
    const int64_t c = 2 * ((int64_t)b * 64 + lane);   // this lane's step of the block: coded bits c, c + 1
    int costs = 0;
    if (c < 2 * (int64_t)T) {
      const int64_t idx = c >= cut ? c + 4 : c;    // idx + 1 < nv: the pair lies inside the row
      costs = (int)soft_costs(row[idx], row[idx + 1]);
    }
    if (b < nfull) {
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        const uint64_t w = acs_soft(pm, (uint32_t)rdlane(costs, i), sh0, sh1, a0, a1);
        klo = lane == i ? (int)(uint32_t)w : klo;
        khi = lane == i ? (int)(uint32_t)(w >> 32) : khi;
      }
    } else {
      for (int i = 0; i < tail; ++i) {
        const uint64_t w = acs_soft(pm, (uint32_t)rdlane(costs, i), sh0, sh1, a0, a1);
        if (lane == i) {
          klo = (int)(uint32_t)w;
          khi = (int)(uint32_t)(w >> 32);
        }
      }
    }
    ws[(int64_t)b * 64 + lane] = ((uint64_t)(uint32_t)khi << 32) | (uint32_t)klo;
  }
  if (lane == 0) {
    out_len[cw] = n_msg;
    metric[cw] = pm;                               // state 0 at step T
  }

  // ---- traceback from state 0 at step T ---------------------------------------
  traceback(ws, nfull, tail, lane, out + cw * out_stride, n_msg);
}

// one thread per output byte: 4 steps (2 in the last byte), at most 2 message bytes
__global__ __launch_bounds__(256) void k_conv_encode(const uint8_t* __restrict__ in, int64_t in_stride,
                                                     const int64_t* __restrict__ in_len, int64_t n_msg,
                                                     uint8_t* __restrict__ out, int64_t out_stride, int64_t l_max) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t m = tid / l_max, j = tid - m * l_max;
  if (m >= n_msg) return;
  const int64_t nb = in_len[m];
  if (nb < 0 || nb > in_stride || 2 * nb + 2 > out_stride || j >= 2 * nb + 2) return;
  const uint8_t* row = in + m * in_stride;
  const int64_t q = j >> 1;                        // steps 4 j .. 4 j + 3 read message bits 4 j - 6 .. 4 j + 3: bytes q - 1, q
  const uint32_t win = ((q >= 1 && q - 1 < nb ? (uint32_t)row[q - 1] : 0u) << 8) | (q < nb ? (uint32_t)row[q] : 0u);
  const int steps = j == 2 * nb + 1 ? 2 : 4;       // the last byte: the final 4 coded bits, right-aligned
  const int u0 = (j & 1) ? 12 : 8;                 // position in `win` (from its MSB) of the first step's newest bit
  uint32_t v = 0;
  for (int k = 0; k < steps; ++k) {
    const uint32_t sr = (win >> (15 - (u0 + k))) & 0x7F;
    v = (v << 2) | ((uint32_t)(__popc(sr & kVitG1) & 1) << 1) | (uint32_t)(__popc(sr & kVitG2) & 1);
  }
  out[m * out_stride + j] = (uint8_t)v;
}

}  // namespace

hipError_t launch_viterbi(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                          int64_t out_stride, int64_t* out_len, int32_t* metric, void* work, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int per = kVitThreads / 64;
  hipLaunchKernelGGL(k_viterbi, dim3((unsigned)((n + per - 1) / per)), dim3(kVitThreads), 0, st, in, in_stride, in_len,
                     n, out, out_stride, out_len, metric, (uint64_t*)work, vit_work_words(in_stride));
  return hipGetLastError();
}

hipError_t launch_viterbi_soft(const int8_t* in, int64_t in_stride, int64_t in_offset, const int64_t* in_len, int64_t n,
                               uint8_t* out, int64_t out_stride, int64_t* out_len, int32_t* metric, void* work,
                               hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int per = kVitThreads / 64;
  hipLaunchKernelGGL(k_viterbi_soft, dim3((unsigned)((n + per - 1) / per)), dim3(kVitThreads), 0, st, in, in_stride,
                     in_offset, in_len, n, out, out_stride, out_len, metric, (uint64_t*)work,
                     vit_soft_work_words(in_stride));
  return hipGetLastError();
}

hipError_t launch_conv_encode(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                              int64_t out_stride, int64_t l_max, hipStream_t st) {
  if (n <= 0 || l_max <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_conv_encode, dim3((unsigned)((n * l_max + 255) / 256)), dim3(256), 0, st, in, in_stride, in_len,
                     n, out, out_stride, l_max);
  return hipGetLastError();
}

}  // namespace amr
