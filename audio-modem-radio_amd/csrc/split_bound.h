// split_bound.h -- the time-split layouts' STRICT bound on the device, stated
// once for both modems (PSK: psk_split_kernels.hip KS1 / KS2 and KB1 / KB2,
// one band-pass filter per stream; FSK: fsk_kernels.hip FS1 / FS2 and KF1 /
// KF2, one per (stream, tone)).  split_strict.h derives the bound and designs
// its tables on the host (StrictBp); here are
//   * the per-step accumulator of the chunk kernels (StepBound),
//   * one filter run's scratch row and per-pass scalars (StrictRow),
//   * the two block stages that turn the per-block step bounds and per-chunk
//     start bounds into a bound on every output block of the filtfilt:
//     KB1 E1[J]  the forward pass, output block J: the split's and the serial's
//                rounding (block sums of D through W, the cut remainder at max D),
//                the chunk starts' errors (+ truncation tk * peak) through GS
//     KB2 E2[J]  the backward pass at forward block J: the forward rounding
//                through the backward pass (K12, exact at block resolution), the
//                start errors through |h| (HS), the last input's error through the
//                zi start (TZ), its own rounding and starts (in its own block index)
//     max E2 = F bounds |split - serial| on every sample of the filter's output
//     while the a-posteriori caps hold (each pass's difference <= 2^-10 of its
//     input peak; the callers flag a row past them).
// The serial's rounding is the split's within those caps.  Every sum is of
// non-negative terms.  The stages are grid-wide (thread = output block, grid.y
// = row; a row's maxima meet in its bnd slots by atomicMax between stages):
// round 6's first cut ran them in one workgroup per stream, 1.05 ms of a
// 1.4 ms strict one-capture call.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "amr_internal.h"

namespace amr {

constexpr int kKbThreads = 256;
// both paths' rounding of a pass (the serial's within the caps of the split's)
constexpr double kKbTwo = 2.0 + 0x1p-20;

// |v| as ordered bits (NaN above inf above every finite value)
__device__ __forceinline__ unsigned long long abs_bits(double v) {
  return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffULL;
}
__device__ __forceinline__ double bnd_get(const unsigned long long* b, int i) {
  return __longlong_as_double((long long)b[i]);
}
// a wave's maximum of non-negative v into *m (one atomic per wave)
__device__ __forceinline__ void wave_max_to(unsigned long long* m, double v, bool live) {
  unsigned long long x = live ? abs_bits(v) : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long y = __shfl_xor(x, o);
    x = y > x ? y : x;
  }
  if ((threadIdx.x & 63) == 0 && x != 0ull) atomicMax(m, x);
}

// A chunk's per-step bounds (split_strict.h): the rounding one DF-II-T step of
// scipy's order commits, summed over states, is at most
//   D = u2 sz + kx |x| + ky |y|,  sz = sum_{i>=1} |z_i| of the pre-step states
// (sz in the caller's own pairing: step_bound_pre, fsk_step_sz).  Keeps the
// chunk's largest D and stores the sums of D per block of kStrictBlk outputs
// to dblk (chunks start on block boundaries, so a block stays within a lane).
struct StepBound {
  double kx, ky;
  double* dblk;
  double dmax = 0.0, dsum = 0.0;
  int dcnt = 0;
  __device__ __forceinline__ void add(double sz, double x, double y, int64_t index) {
    const double dd = __builtin_fma(kStrictU2, sz, __builtin_fma(kx, fabs(x), ky * fabs(y)));
    dmax = fmax(dmax, dd);
    dsum += dd;
    if (++dcnt == kStrictBlk) {
      dblk[index / kStrictBlk] = dsum;
      dsum = 0.0;
      dcnt = 0;
    }
  }
  // after the chunk's last output: the pass's last, partial block
  __device__ __forceinline__ void finish(int64_t last_index) {
    if (dcnt > 0) dblk[last_index / kStrictBlk] = dsum;
  }
};

// One filter run's row: its scratch, its 8 maxima
//   bw: 0 D1max, 1 E1max (KB1), 2 max|y1|, 3 D2max, 4 S1max (KB1), 5 max|f|
//       (PSK), 6 Fmax (KB2), 7 Xmax (PSK KB3)
// and the scalars of its two passes: the input peaks (peak1; p2 = max|y1| +
// cap1), the caps, and the forward pass's per-row terms c1
struct StrictRow {
  double* sc;
  unsigned long long* bw;
  double D1m, y1m, D2m, peak1, cap1, p2, cap2, c1;
};
__device__ __forceinline__ StrictRow strict_row(const StrictBp& d, const StrictRows& r, unsigned long long* bnd,
                                                int64_t row, unsigned long long peak_bits) {
  StrictRow k;
  k.sc = r.sc + row * r.sstride;
  k.bw = bnd + row * 8;
  k.D1m = bnd_get(k.bw, 0);
  k.y1m = bnd_get(k.bw, 2);
  k.D2m = bnd_get(k.bw, 3);
  k.peak1 = __longlong_as_double((long long)peak_bits);
  k.cap1 = 0x1p-10 * k.peak1;
  k.p2 = k.y1m + k.cap1;
  k.cap2 = 0x1p-10 * k.p2;
  const double sec1 = kStrictU2 * d.zb * k.cap1 + d.ky * k.cap1;
  // the forward pass's per-row terms (besides the block sums)
  k.c1 = d.g1x * (sec1 + 2 * 0x1p-1060) + d.gmax * 0x1p-53 * d.zi_sum * k.peak1;
  return k;
}

// A pass's own terms at its block K: its rounding (the D blocks dblk through
// W, the cut remainder at the pass's max D), and its chunk's start error (the
// start bound ds[chunk] + the truncation tk * the pass's input peak, through
// GS at the block's place in the chunk; LB blocks per chunk, none for the
// chunk at the pass's start)
__device__ __forceinline__ double strict_own_r(const StrictBp& d, const double* dblk, double Dm, int64_t K) {
  double r = d.w_tail * Dm;
  const int64_t dn = K + 1 < d.nw ? K + 1 : d.nw;
#pragma unroll 8
  for (int64_t dl = 0; dl < dn; ++dl) r = __builtin_fma(d.W[dl], dblk[K - dl], r);
  return r;
}
__device__ __forceinline__ double strict_own_st(const StrictBp& d, const double* ds, double peak, int64_t K,
                                                int64_t LB) {
  const int64_t c = K / LB;
  const int64_t q = K - c * LB;
  return c > 0 ? (q < 64 ? d.GS[q] : d.gmax) * (ds[c] + d.tk * peak) : 0.0;
}

// KB1 at block J: stores S1[J], E1[J]; the caller takes their maxima to bw[4], bw[1]
struct StrictE1 {
  double e, st;
};
__device__ __forceinline__ StrictE1 strict_e1_block(const StrictBp& d, const StrictRows& r, const StrictRow& k,
                                                    int64_t J, int64_t LB) {
  StrictE1 o{0.0, 0.0};
  if (J < r.nb1) {
    const double rr = strict_own_r(d, k.sc + strict_off_d1(r), k.D1m, J);
    o.st = strict_own_st(d, k.sc + strict_off_ds1(r), k.peak1, J, LB);
    o.e = kKbTwo * rr + k.c1 + o.st;
    k.sc[strict_off_s1(r) + J] = o.st;
    k.sc[strict_off_e1(r) + J] = o.e;
  }
  return o;
}

// KB2 at forward block J (after KB1's maxima): stores and returns E2[J]; the
// caller takes its maximum to bw[6]
__device__ __forceinline__ double strict_e2_block(const StrictBp& d, const StrictRows& r, const StrictRow& k,
                                                  int64_t J, int64_t LB, int64_t m1) {
  const int64_t nb1 = r.nb1;
  const double* d1 = k.sc + strict_off_d1(r);
  const double* d2 = k.sc + strict_off_d2(r);
  const double* ds2 = k.sc + strict_off_ds2(r);
  const double* e1 = k.sc + strict_off_e1(r);
  const double* s1 = k.sc + strict_off_s1(r);
  const double E1max = bnd_get(k.bw, 1), S1max = bnd_get(k.bw, 4);
  const double E1last = fmax(e1[nb1 - 1], nb1 > 1 ? e1[nb1 - 2] : 0.0);
  const double sec2 = kStrictU2 * d.zb * k.cap2 + d.kx * E1max + d.ky * k.cap2;
  const double c2 = d.hz * k.c1 + d.g1x * (sec2 + 2 * 0x1p-1060) + 2.0 * d.gmax * 0x1p-53 * d.zi_sum * k.p2;
  // the backward pass's own rounding and starts at its block K (its own index)
  auto own2 = [&](int64_t K) {
    if (K < 0 || K >= nb1) return 0.0;
    return kKbTwo * strict_own_r(d, d2, k.D2m, K) + strict_own_st(d, ds2, k.p2, K, LB);
  };
  auto tzw = [&](int64_t q) { return q < d.nz ? d.TZ[q] : d.tz_tail; };
  double e = 0.0;
  if (J < nb1) {
    // forward block J: j in [16 J, 16 J + 15] <-> backward index k2 = m1 - 1 - j
    double a = d.k12_tail * k.D1m;
    // the taps whose block lies inside the pass, in the same (ascending) order
    const int64_t klo = d.k12_off - J > 0 ? d.k12_off - J : 0;
    const int64_t khi = nb1 - J + d.k12_off < d.nk ? nb1 - J + d.k12_off : d.nk;
#pragma unroll 8
    for (int64_t kq = klo; kq < khi; ++kq) a = __builtin_fma(d.K12[kq], d1[J + kq - d.k12_off], a);
    double h = d.hs_tail * S1max;
    const int64_t hhi = nb1 - J < d.nh ? nb1 - J : d.nh;
#pragma unroll 8
    for (int64_t db = 0; db < hhi; ++db) h = __builtin_fma(d.HS[db], s1[J + db], h);
    const int64_t jhi = 16 * J + 15 < m1 - 1 ? 16 * J + 15 : m1 - 1;
    const int64_t k2lo = m1 - 1 - jhi, k2hi = m1 - 1 - 16 * J;
    const int64_t Ka = k2lo / kStrictBlk, Kb = k2hi / kStrictBlk;
    const double tz = fmax(tzw(Ka), tzw(Kb)) * E1last;
    const double o2 = fmax(own2(Ka), own2(Kb));
    e = kKbTwo * a + h + tz + o2 + c2;
    k.sc[strict_off_e2(r) + J] = e;
  }
  return e;
}

}  // namespace amr
