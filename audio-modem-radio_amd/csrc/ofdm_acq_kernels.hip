// ofdm_acq_kernels.hip -- ofdm acquisition: where in an
// unaligned capture the OFDM symbols begin.  A cyclic prefix repeats the last
// Ncp samples of its symbol, so x[i] - x[i + Nu] vanishes for the Ncp samples
// i of every prefix; folded over the capture's periods of L samples and summed
// over a window of Ncp, its square is smallest where the window is a prefix.
// tests/ofdm_acquire_cases.py restates both kernels in numpy; float64, no fma,
// and the summation orders below are the specification: bit-equal.
//
//   k_ofdm_fold     g_q[r] = sum_s (x[sL + r] - x[sL + r + Nu])^2 over segment q's 64 periods
//   k_ofdm_acq_min  G = sum_q g_q; E[d] = sum_{i < Ncp} G[(d + i) % L]; first minimum; back-off
#include <hip/hip_runtime.h>

#include "ofdm.h"
#include "psk_common.h"

namespace amr {
namespace {

// ---------------------------------------------------------------------------
// k_ofdm_fold.  One lane owns one (stream, segment, r), flat index
// (b * segments + q) * L + r: consecutive lanes read consecutive samples of
// one period, whatever L is (a wave spans segments and streams when L < 64,
// so no lane idles but the grid's last few).  The lane's sum is sequential
// over the segment's periods from 0.0, the square rounded before it is added.
// The second read, Nu samples on, hits lines the wave's first reads fetched
// (Nu < L: this period's or the next one's).
// The last sample read is (M - 1) L + (L - 1) + Nu <= n - 1 by M's definition:
// nothing at or past n, nothing in a row's padding.
constexpr int kFoldBlock = 256;
constexpr int kFoldUnroll = 8;                  // periods in flight per lane (kAcqSeg is a multiple)

template <typename T>
__global__ __launch_bounds__(kFoldBlock) void k_ofdm_fold(const T* __restrict__ x, int64_t x_stride,
                                                          int64_t n_streams, OfdmParams p, int64_t periods,
                                                          int64_t segments, double* __restrict__ gq) {
  const int64_t flat = (int64_t)blockIdx.x * kFoldBlock + threadIdx.x;
  if (flat >= n_streams * segments * p.L) return;
  const int64_t bq = flat / p.L, r = flat - bq * p.L;
  const int64_t b = bq / segments, q = bq - b * segments;
  const int64_t s0 = q * kAcqSeg;
  const int cnt = periods - s0 < kAcqSeg ? (int)(periods - s0) : kAcqSeg;   // >= 1
  const T* __restrict__ a = x + b * x_stride + s0 * p.L + r;
  const T* __restrict__ c = a + p.nu;
  double acc = 0.0;
  int s = 0;
  for (; s + kFoldUnroll <= cnt; s += kFoldUnroll) {
    T u[kFoldUnroll], v[kFoldUnroll];
#pragma unroll
    for (int j = 0; j < kFoldUnroll; ++j) {      // every load of the group before the first sum
      u[j] = a[(s + j) * p.L];
      v[j] = c[(s + j) * p.L];
    }
#pragma unroll
    for (int j = 0; j < kFoldUnroll; ++j) {
      const double d = In<T>::cvt(u[j]) - In<T>::cvt(v[j]);
      acc = acc + d * d;
    }
  }
  for (; s < cnt; ++s) {
    const double d = In<T>::cvt(a[s * p.L]) - In<T>::cvt(c[s * p.L]);
    acc = acc + d * d;
  }
  gq[flat] = acc;
}

// ---------------------------------------------------------------------------
// k_ofdm_acq_min.  One wave per stream (workgroup = one wave), lane per r / d
// in strides of 64, three steps with the block's G and E rows in global
// memory between them (a row is 8 L bytes, L has no upper bound a fixed LDS
// array could hold, and the rows stay in the CU's cache: the window sum's
// reads are consecutive across lanes):
//   G[r] = ((0.0 + g_0[r]) + g_1[r]) + ...     in segment order
//   E[d] = ((0.0 + G[d]) + G[(d + 1) % L]) + ...   Ncp terms, in that order
//   best = 0; for d = 1 .. L-1: if (E[d] < E[best]) best = d
// The sequential rule's result, for a parallel search: a NaN E[0] keeps 0
// (nothing compares below a NaN); otherwise best only ever moves to a smaller
// non-NaN value, so it ends on the first index of the least non-NaN value, and
// on 0 when nothing is below E[0].  A lane scans its own d ascending with the
// same strict comparison from (E[0], 0), so it holds either that pair or the
// first index in its stride of its least value below E[0]; across lanes the
// smaller value wins and, on equal values, the smaller index.
__global__ __launch_bounds__(kWave) void k_ofdm_acq_min(OfdmParams p, int64_t segments,
                                                        const double* __restrict__ gq, double* __restrict__ G,
                                                        double* __restrict__ E, int64_t* __restrict__ dhat,
                                                        int64_t* __restrict__ offset) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t L = p.L;
  const double* __restrict__ g = gq + (size_t)b * (size_t)(segments * L);
  double* __restrict__ Gb = G + (size_t)b * (size_t)L;
  double* __restrict__ Eb = E + (size_t)b * (size_t)L;
  for (int64_t r = lane; r < L; r += kWave) {
    double acc = 0.0;
    for (int64_t q = 0; q < segments; ++q) acc = acc + g[q * L + r];
    Gb[r] = acc;
  }
  __syncthreads();                              // G is whole (the wave's own stores, waited for)
  for (int64_t d = lane; d < L; d += kWave) {
    double acc = 0.0;
    int64_t j = d;
    for (int64_t i = 0; i < p.ncp; ++i) {
      acc = acc + Gb[j];
      if (++j == L) j = 0;
    }
    Eb[d] = acc;
  }
  __syncthreads();
  const double e0 = Eb[0];
  double bv = e0;
  int64_t bi = 0;
  for (int64_t d = lane; d < L; d += kWave) {   // d = 0 compares E[0] with itself: false
    const double v = Eb[d];
    if (v < bv) {
      bv = v;
      bi = d;
    }
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const double ov = __shfl_xor(bv, m);
    const int64_t oi = __shfl_xor(bi, m);
    if (ov < bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    const int64_t best = e0 != e0 ? 0 : bi;
    int64_t o = best - p.ncp / 2;
    if (o > L - 1 - p.ncp) o -= L;
    dhat[b] = best;
    offset[b] = o;
  }
}

}  // namespace

hipError_t launch_ofdm_acquire(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const OfdmParams& p,
                               const OfdmAcq& a, hipStream_t st) {
  if (n_streams < 1) return hipSuccess;
  const int64_t periods = ofdm_acq_periods(p), segments = ofdm_acq_segments(p);
  const int64_t total = n_streams * segments * p.L;
  if (total > 0) {
    const int64_t blocks = (total + kFoldBlock - 1) / kFoldBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (dtype == kF32)
      hipLaunchKernelGGL(k_ofdm_fold<float>, grid, dim3(kFoldBlock), 0, st, (const float*)x, x_stride, n_streams, p,
                         periods, segments, a.gq);
    else if (dtype == kF64)
      hipLaunchKernelGGL(k_ofdm_fold<double>, grid, dim3(kFoldBlock), 0, st, (const double*)x, x_stride, n_streams,
                         p, periods, segments, a.gq);
    else if (dtype == kI16)
      hipLaunchKernelGGL(k_ofdm_fold<int16_t>, grid, dim3(kFoldBlock), 0, st, (const int16_t*)x, x_stride,
                         n_streams, p, periods, segments, a.gq);
    else
      return hipErrorInvalidValue;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_ofdm_acq_min, dim3((unsigned)n_streams), dim3(kWave), 0, st, p, segments, a.gq, a.G, a.E,
                     a.dhat, a.offset);
  return hipGetLastError();
}

}  // namespace amr
