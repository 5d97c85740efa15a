// msk_acq_kernels.hip -- minshift bit timing: the bit clock of
// a capture that starts anywhere.  The squared signal has a spectral line at
// twice each tone; the two lines' phase difference is the bit clock.  No search
// over offsets: one pass over x into two single-bin sums, then L scores.
// tests/minshift_cases.py restates both kernels in numpy; float64, no fma, and
// the summation orders below are the specification: bit-equal.
//
//   k_msk_lines    the segment's c_t = sum_m (x[m] x[m]) * E_t[m % (2 L)], t = 0, 1
//   k_msk_acq_max  c = the segments' sums in order; q = c1 conj(c0); P[d] = Re(q R[d]); the first maximum
#include <hip/hip_runtime.h>

#include "msk.h"
#include "psk_common.h"

namespace amr {
namespace {

// ---------------------------------------------------------------------------
// k_msk_lines.  One wave per (stream, segment of kMskSeg samples): lane j owns
// partial j, which adds the samples m = seg * 4096 + 64 a + j sequentially in a
// from 0.0 -- row a of the segment is one coalesced load of 64 consecutive
// samples.  The square is rounded first, then each of the four component
// products, then the sum.  The table index m % (2 L) is divided once, for a = 0,
// and then advanced by 64 % (2 L) with one conditional subtraction per row.
// E0 and E1 are read from LDS when a table's 2 L entries fit kMskLdsEntries
// (16 KB for both: ten workgroups' worth in a CU's 160 KB), from global memory
// otherwise.  A short last segment has fewer terms: the full rows run without a
// bounds test, the one partial row with it; a lane that gets no term keeps 0.0.
// The 64 partials are combined by the tree j with j + 32, then 16, 8, 4, 2, 1:
// after the exchange at distance w every lane holds p[j] + p[j ^ w], which for
// j < w is the tree's p[j] + p[j + w] (addition commutes), so lane 0 ends with
// the tree's sum.
constexpr int kMskLdsEntries = 512;

template <typename T, bool LDS>
__global__ __launch_bounds__(kWave) void k_msk_lines(const T* __restrict__ x, int64_t x_stride, MskParams p,
                                                     int64_t segments, const double2* __restrict__ E0,
                                                     const double2* __restrict__ E1, double* __restrict__ seg) {
  __shared__ double2 e0s[LDS ? kMskLdsEntries : 1];
  __shared__ double2 e1s[LDS ? kMskLdsEntries : 1];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x / segments, q = blockIdx.x - b * segments;
  const int64_t m0 = q * kMskSeg;
  const int cnt = p.n - m0 < kMskSeg ? (int)(p.n - m0) : kMskSeg;   // >= 1: q < ceil(n / 4096)
  const uint32_t P2 = (uint32_t)(2 * p.L);                          // <= 2^25
  if constexpr (LDS) {
    for (uint32_t i = lane; i < P2; i += kWave) {
      e0s[i] = E0[i];
      e1s[i] = E1[i];
    }
    __syncthreads();
  }
  const T* __restrict__ xb = x + b * x_stride + m0;
  uint32_t idx = (uint32_t)((uint64_t)(m0 + lane) % P2);
  const uint32_t step = (uint32_t)kWave % P2;
  double a0r = 0.0, a0i = 0.0, a1r = 0.0, a1i = 0.0;
  const int full = cnt / kWave;                 // rows every lane has a sample in
  auto term = [&](int i) {
    const double xv = In<T>::cvt(xb[i]);
    const double sq = xv * xv;
    const double2 e0 = LDS ? e0s[idx] : E0[idx];
    const double2 e1 = LDS ? e1s[idx] : E1[idx];
    a0r = a0r + sq * e0.x;
    a0i = a0i + sq * e0.y;
    a1r = a1r + sq * e1.x;
    a1i = a1i + sq * e1.y;
  };
#pragma unroll 8
  for (int a = 0; a < full; ++a) {
    term(a * kWave + lane);
    idx += step;
    if (idx >= P2) idx -= P2;
  }
  if (full * kWave + lane < cnt) term(full * kWave + lane);
#pragma unroll
  for (int w = kWave / 2; w >= 1; w >>= 1) {
    a0r = a0r + __shfl_xor(a0r, w);
    a0i = a0i + __shfl_xor(a0i, w);
    a1r = a1r + __shfl_xor(a1r, w);
    a1i = a1i + __shfl_xor(a1i, w);
  }
  if (lane == 0) {
    double2* __restrict__ o = reinterpret_cast<double2*>(seg + (size_t)blockIdx.x * 4);
    o[0] = make_double2(a0r, a0i);
    o[1] = make_double2(a1r, a1i);
  }
}

// ---------------------------------------------------------------------------
// k_msk_acq_max.  k_dsss_acq_max's shape: one wave per stream.  Lanes 0 .. 3
// add one component each of the segments' sums, in segment order from 0.0;
//   q = c1 * conj(c0) = (c1r c0r + c1i c0i, c1i c0r - c1r c0i)
//   P[d] = q.re * R[d].re - q.im * R[d].im
//   best = 0; for d = 1 .. L-1: if (P[d] > P[best]) best = d
// The sequential rule's result, for a parallel search (as k_dsss_acq_max): a
// NaN P[0] keeps 0; otherwise best ends on the first index of the greatest
// non-NaN value.  A lane scans its own d ascending with the same strict
// comparison from (P[0], 0); across lanes the larger value wins and, on equal
// values, the smaller index.
__global__ __launch_bounds__(kWave) void k_msk_acq_max(int64_t L, int64_t segments, const double* __restrict__ seg,
                                                       const double2* __restrict__ R, int64_t* __restrict__ offset,
                                                       double* __restrict__ qout) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  double c = 0.0;
  if (lane < 4) {
    const double* __restrict__ g = seg + (size_t)b * (size_t)segments * 4 + lane;
    for (int64_t s = 0; s < segments; ++s) c = c + g[s * 4];
  }
  const double c0r = __shfl(c, 0), c0i = __shfl(c, 1), c1r = __shfl(c, 2), c1i = __shfl(c, 3);
  const double qr = c1r * c0r + c1i * c0i;
  const double qi = c1i * c0r - c1r * c0i;
  const double2 r0 = R[0];
  const double p0 = qr * r0.x - qi * r0.y;
  double bv = p0;
  int64_t bi = 0;
  for (int64_t d = lane; d < L; d += kWave) {   // d = 0 compares P[0] with itself: false
    const double2 r = R[d];
    const double v = qr * r.x - qi * r.y;
    if (v > bv) {
      bv = v;
      bi = d;
    }
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const double ov = __shfl_xor(bv, m);
    const int64_t oi = __shfl_xor(bi, m);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    offset[b] = p0 != p0 ? 0 : bi;
    if (qout) *reinterpret_cast<double2*>(qout + (size_t)b * 2) = make_double2(qr, qi);
  }
}

template <typename T>
hipError_t lines_launch(const void* x, int64_t x_stride, const MskParams& p, int64_t segments, dim3 grid,
                        const double* E0, const double* E1, double* seg, hipStream_t st) {
  const double2* e0 = reinterpret_cast<const double2*>(E0);
  const double2* e1 = reinterpret_cast<const double2*>(E1);
  if (2 * p.L <= kMskLdsEntries)
    hipLaunchKernelGGL((k_msk_lines<T, true>), grid, dim3(kWave), 0, st, (const T*)x, x_stride, p, segments, e0, e1,
                       seg);
  else
    hipLaunchKernelGGL((k_msk_lines<T, false>), grid, dim3(kWave), 0, st, (const T*)x, x_stride, p, segments, e0, e1,
                       seg);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_msk_lines(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const MskParams& p,
                            const double* E0, const double* E1, double* seg, hipStream_t st) {
  const int64_t segments = msk_acq_segments(p.n);
  if (n_streams < 1 || segments < 1) return hipSuccess;
  const int64_t blocks = n_streams * segments;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  if (dtype == kF32) return lines_launch<float>(x, x_stride, p, segments, grid, E0, E1, seg, st);
  if (dtype == kF64) return lines_launch<double>(x, x_stride, p, segments, grid, E0, E1, seg, st);
  if (dtype == kI16) return lines_launch<int16_t>(x, x_stride, p, segments, grid, E0, E1, seg, st);
  return hipErrorInvalidValue;
}

hipError_t launch_msk_acq_max(int64_t L, int64_t segments, int64_t n_streams, const double* seg, const double* R,
                              int64_t* offset, double* q, hipStream_t st) {
  if (n_streams < 1) return hipSuccess;
  hipLaunchKernelGGL(k_msk_acq_max, dim3((unsigned)n_streams), dim3(kWave), 0, st, L, segments, seg,
                     reinterpret_cast<const double2*>(R), offset, q);
  return hipGetLastError();
}

}  // namespace amr
