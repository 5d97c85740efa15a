// dsss_acq_kernels.hip -- spread acquisition: the code phase of
// a capture that starts anywhere.  The capture is mixed down by the carrier
// table at the absolute sample index and summed per chip, u[m]; at every sample
// offset d of a bit the chips are correlated with the code, y(d, s), and the
// energy |y|^2 is summed over the capture's bits: where the window is a bit,
// every chip adds in phase.  tests/spread_cases.py restates both kernels in
// numpy; float64, no fma, and the summation orders below are the
// specification: bit-equal.
//
//   k_dsss_acquire  g_q[d] = sum_s |sum_j cs[j] u[d + sL + j spc]|^2 over segment q's 64 bits
//   k_dsss_acq_max  P = sum_q g_q; the first maximum
#include <hip/hip_runtime.h>

#include "dsss.h"
#include "psk_common.h"

namespace amr {
namespace {

// ---------------------------------------------------------------------------
// k_dsss_acquire.  One workgroup per (stream, segment, tile of offsets): lanes
// own the tile's offsets d (at most kAcqTile, two per lane), walk the segment's
// bits in order and keep y and the segment's sum in registers.  u never leaves
// the CU: it lives in an LDS ring indexed by the absolute m & (kAcqRing - 1).
// A step is (bit s, chips j0 .. j0 + jc): it needs u over
//   [d0 + sL + j0 spc,  d0 + sL + j0 spc + dcnt + (jc - 1) spc)
// jc is chosen so that this window fits the ring whatever L is (the chips of a
// bit go in ceil(C / jc) steps, y carried across them in registers, the order
// in j kept).  Where the whole code fits (jc = C) a step takes NB bits, as many
// as the ring holds -- L more u each --, so that the barriers and the loads'
// latency are paid once per NB bits (5 at L = 160); a lane then finishes each
// of its bits in turn.  Steps advance in m, so consecutive windows
// overlap and only the u past the previous window's end are computed: when the
// tile covers all of L (L <= kAcqTile) every u is computed once per segment.
// A bit longer than kAcqTile is cut into ceil(L / kAcqTile) tiles, each of
// which walks the same samples: that many times the chip sums.
//
// u[m] = sum_{i < spc} x[m + i] * Wc[(m + i) % L], sequential in i from 0.0,
// the product rounded first.  The product belongs to the sample, not to m: for
// spc <= kAcqSpcLds a batch of at most kAcqBatch u's first stages its samples'
// products in LDS, one multiply pair and one table load per sample, and u is
// then spc additions of LDS reads.  A longer chip sums straight from x and Wc.
//
// The last sample read is (L - 1) + (M - 1) L + (C - 1) spc + spc - 1 <= n - 1 by
// M's definition: nothing at or past n, nothing in a row's padding.
constexpr int kAcqBlock = 256;
constexpr int kAcqTile = 2 * kAcqBlock;         // offsets per workgroup at most
constexpr int kAcqRing = 1024;                  // u's in LDS (complex doubles; a power of two)
constexpr int kAcqBatch = 512;                  // u's computed between two barriers
constexpr int kAcqSpcLds = 128;                 // longest chip whose products are staged

template <typename T>
__global__ __launch_bounds__(kAcqBlock) void k_dsss_acquire(const T* __restrict__ x, int64_t x_stride, DsssParams p,
                                                            int64_t bits, int64_t segments, int64_t tiles, int dt,
                                                            const double2* __restrict__ Wc, CDouble* cs,
                                                            double* __restrict__ gq) {
  __shared__ double2 ring[kAcqRing];
  __shared__ double2 prod[kAcqBatch + kAcqSpcLds];
  const int tid = threadIdx.x;
  int64_t blk = blockIdx.x;
  const int64_t tile = blk % tiles;
  blk /= tiles;
  const int64_t q = blk % segments, b = blk / segments;
  const int64_t L = p.L, spc = p.spc;
  const int C = p.C;
  const int64_t d0 = tile * dt;
  if (d0 >= L) return;                          // the whole workgroup: no barrier is left waiting
  const int dcnt = L - d0 < dt ? (int)(L - d0) : dt;
  const int64_t s0 = q * kDsssSeg;
  const int cnt = bits - s0 < kDsssSeg ? (int)(bits - s0) : kDsssSeg;   // >= 1
  const T* __restrict__ xb = x + b * x_stride;
  const bool staged = spc <= kAcqSpcLds;
  const int64_t fit = 1 + (kAcqRing - dcnt) / spc;                      // chips per step: dcnt + (Jc - 1) spc <= kAcqRing
  const int Jc = fit < C ? (int)fit : C;
  const uint32_t Lu = (uint32_t)L;              // n < 2^31 (the launcher refuses more): sample indices fit 32 bits
  // a step that holds the whole code takes as many bits as the ring holds beside the first
  const int NB = Jc == C ? (int)(1 + (kAcqRing - (dcnt + (int64_t)(C - 1) * spc)) / L) : 1;
  unsigned long long neg = 0;                   // bit j: cs[j] < 0 (wave-uniform)
  for (int j = 0; j < C; ++j) neg |= (unsigned long long)(cs[j] < 0.0) << j;
  int64_t have = -1;                            // the ring holds u[m] for the previous window's m < have
  double acc[2] = {0.0, 0.0};
  for (int s = 0; s < cnt; s += NB) {
    const int nb = cnt - s < NB ? cnt - s : NB;
    double yr[2] = {0.0, 0.0}, yi[2] = {0.0, 0.0};   // carried across the steps of a bit (Jc < C: nb = 1)
    const int64_t base = d0 + (s0 + s) * L;
    for (int j0 = 0; j0 < C; j0 += Jc) {
      const int jc = C - j0 < Jc ? C - j0 : Jc;
      const int64_t wlo = base + j0 * spc, whi = wlo + dcnt + (jc - 1) * spc + (int64_t)(nb - 1) * L;
      for (int64_t ub = have > wlo ? have : wlo; ub < whi; ub += kAcqBatch) {
        const int nu = whi - ub < kAcqBatch ? (int)(whi - ub) : kAcqBatch;
        if (staged) {
          __syncthreads();                      // the previous batch's reads of prod are done
          const int np = nu + (int)spc - 1;
          for (int i = tid; i < np; i += kAcqBlock) {
            const int64_t k = ub + i;
            const double2 w = Wc[(uint32_t)k % Lu];
            const double xv = In<T>::cvt(xb[k]);
            prod[i] = make_double2(xv * w.x, xv * w.y);
          }
          __syncthreads();
          for (int i = tid; i < nu; i += kAcqBlock) {
            double ar = 0.0, ai = 0.0;
#pragma unroll 5                                // several LDS reads in flight ahead of the dependent sums
            for (int c = 0; c < (int)spc; ++c) {
              const double2 pv = prod[i + c];
              ar = ar + pv.x;
              ai = ai + pv.y;
            }
            ring[(ub + i) & (kAcqRing - 1)] = make_double2(ar, ai);
          }
        } else {
          for (int i = tid; i < nu; i += kAcqBlock) {
            const int64_t m = ub + i;
            uint32_t km = (uint32_t)m % Lu;
            double ar = 0.0, ai = 0.0;
            for (int64_t c = 0; c < spc; ++c) {
              const double2 w = Wc[km];
              const double xv = In<T>::cvt(xb[m + c]);
              ar = ar + xv * w.x;
              ai = ai + xv * w.y;
              if (++km == Lu) km = 0;
            }
            ring[m & (kAcqRing - 1)] = make_double2(ar, ai);
          }
        }
      }
      if (whi > have) have = whi;
      __syncthreads();                          // the window is whole
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int d = tid + r * kAcqBlock;
        if (d < dcnt) {
          for (int bb = 0; bb < nb; ++bb) {
            uint32_t m = (uint32_t)(wlo + d + (int64_t)bb * L);
            double ar = yr[r], ai = yi[r];
            // cs[j] * u is an exact sign flip: the sign bit of u is toggled where cs[j] < 0 (no branch, so that
            // several LDS reads are in flight ahead of the dependent sums)
#pragma unroll 4
            for (int j = 0; j < jc; ++j) {
              const double2 u = ring[m & (kAcqRing - 1)];
              const unsigned long long flip = ((neg >> (j0 + j)) & 1ull) << 63;
              ar = ar + __longlong_as_double(__double_as_longlong(u.x) ^ (long long)flip);
              ai = ai + __longlong_as_double(__double_as_longlong(u.y) ^ (long long)flip);
              m += (uint32_t)spc;
            }
            if (Jc == C) {                      // the bit is whole: its energy, in bit order
              acc[r] = acc[r] + (ar * ar + ai * ai);
            } else {
              yr[r] = ar;
              yi[r] = ai;
            }
          }
        }
      }
      __syncthreads();                          // before the next step overwrites the ring
    }
    if (Jc != C) {
#pragma unroll
      for (int r = 0; r < 2; ++r) acc[r] = acc[r] + (yr[r] * yr[r] + yi[r] * yi[r]);
    }
  }
  double* __restrict__ g = gq + (size_t)(b * segments + q) * (size_t)L + (size_t)d0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int d = tid + r * kAcqBlock;
    if (d < dcnt) g[d] = acc[r];
  }
}

// ---------------------------------------------------------------------------
// k_dsss_acq_max.  k_ofdm_acq_min's shape: one wave per stream, lane per d in
// strides of 64.
//   P[d] = ((0.0 + g_0[d]) + g_1[d]) + ...     in segment order
//   best = 0; for d = 1 .. L-1: if (P[d] > P[best]) best = d
// The sequential rule's result, for a parallel search: a NaN P[0] keeps 0
// (nothing compares above a NaN); otherwise best only ever moves to a larger
// non-NaN value, so it ends on the first index of the greatest non-NaN value,
// and on 0 when nothing is above P[0].  A lane scans its own d ascending with
// the same strict comparison from (P[0], 0); across lanes the larger value
// wins and, on equal values, the smaller index.
__global__ __launch_bounds__(kWave) void k_dsss_acq_max(DsssParams p, int64_t segments,
                                                        const double* __restrict__ gq, double* __restrict__ P,
                                                        int64_t* __restrict__ offset) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t L = p.L;
  const double* __restrict__ g = gq + (size_t)b * (size_t)(segments * L);
  double* __restrict__ Pb = P + (size_t)b * (size_t)L;
  for (int64_t d = lane; d < L; d += kWave) {
    double acc = 0.0;
    for (int64_t q = 0; q < segments; ++q) acc = acc + g[q * L + d];
    Pb[d] = acc;
  }
  __syncthreads();                              // P is whole (the wave's own stores, waited for)
  const double p0 = Pb[0];
  double bv = p0;
  int64_t bi = 0;
  for (int64_t d = lane; d < L; d += kWave) {   // d = 0 compares P[0] with itself: false
    const double v = Pb[d];
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
  if (lane == 0) offset[b] = p0 != p0 ? 0 : bi;
}

}  // namespace

hipError_t launch_dsss_acquire(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const DsssParams& p,
                               const double* Wc, const double* cs, const DsssAcq& a, hipStream_t st) {
  if (n_streams < 1) return hipSuccess;
  if (p.n > 0x7fffffffLL) return hipErrorInvalidValue;
  const int64_t bits = dsss_acq_bits(p), segments = dsss_acq_segments(p);
  if (segments > 0) {
    const int64_t tiles = (p.L + kAcqTile - 1) / kAcqTile;
    const int dt = (int)((p.L + tiles - 1) / tiles);
    const int64_t blocks = n_streams * segments * tiles;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    const double2* w = reinterpret_cast<const double2*>(Wc);
    CDouble* c = (CDouble*)cs;
    if (dtype == kF32)
      hipLaunchKernelGGL(k_dsss_acquire<float>, grid, dim3(kAcqBlock), 0, st, (const float*)x, x_stride, p, bits,
                         segments, tiles, dt, w, c, a.gq);
    else if (dtype == kF64)
      hipLaunchKernelGGL(k_dsss_acquire<double>, grid, dim3(kAcqBlock), 0, st, (const double*)x, x_stride, p, bits,
                         segments, tiles, dt, w, c, a.gq);
    else if (dtype == kI16)
      hipLaunchKernelGGL(k_dsss_acquire<int16_t>, grid, dim3(kAcqBlock), 0, st, (const int16_t*)x, x_stride, p, bits,
                         segments, tiles, dt, w, c, a.gq);
    else
      return hipErrorInvalidValue;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_dsss_acq_max, dim3((unsigned)n_streams), dim3(kWave), 0, st, p, segments, a.gq, a.P, a.offset);
  return hipGetLastError();
}

}  // namespace amr
