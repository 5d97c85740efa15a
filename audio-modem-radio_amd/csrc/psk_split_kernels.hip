// psk_split_kernels.hip -- the PSK time-split (chunk-parallel) layout, for
// one capture or a few: the latency path of the reference's own call pattern
// (filebeep_advanced_v2.py:324, 1112 decode one capture at a time).
//
// qpsk_demodulate / bpsk_demodulate (modem.py:189-266 / 68-135) are four
// serial recurrences per stream -- band-pass filtfilt forward and backward,
// low-pass filtfilt forward and backward (modem.py:194-204) -- so a lone
// stream's serial path is ~4 x 96 000 dependent steps (the row layout:
// 10.5 ms for one 1-s capture).  Here each pass is cut into
// chunks of L outputs, one lane per chunk, and every chunk starts its
// recursion W samples early from a zero state (or, the chunk that holds the
// pass's first sample, from scipy's exact initial state zi * x0).  The
// filters are stable, so after W samples the zero start has decayed below
// the rounding level (W per filter from its impulse responses,
// api.cpp split_design); what remains is a DIFFERENT ROUNDING TRAJECTORY:
// the chunked values differ from the serial ones by rounding noise amplified
// by the filter (a DF-II-T with poles at |z| = 0.989 amplifies its rounding
// by ~1e7).  So the symbols are NOT bit-exact, and the decisions are made
// exact by a margin instead, in one of two modes:
//   * DEFAULT (a measured premise, not a proof): the symbol error is taken to
//     be below E = kappa * peak|x| (kappa per plan: 64 x the L1 noise gain
//     u * sum_i ||g_i||_1 of both filters).  Measured, not derived: the
//     worst error over tones, square waves, noise, modulated, clipped, chirp
//     and adversarially searched inputs at 10+ parameter sets stays >= 16x
//     (tests: >= 56x) below kappa * peak (tests/test_split_margin.py,
//     tests/test_gpu_split.py).  An input outside that evidence could in
//     principle exceed E, and an unflagged decision could then differ.
//   * STRICT (AMR_PSK_SPLIT_STRICT=1 / amr_psk_plan_set_split_strict): KS1 /
//     KS2 also accumulate per-block rounding bounds of every step, and KB
//     (KB1-KB4, k_split_strict_*) turn them into a per-symbol bound e(k) that
//     holds for every input (a forward error analysis of the DF-II-T chain,
//     csrc/split_strict.h; a pass whose error exceeds 2^-10 of its input's
//     peak flags the stream instead).  E = e(k) then, and the margin below is
//     a proof.
//   * either way a differential product whose decision could move by its
//     error -- |d error|_2 <= E (|s0|_2 + |s1|_2 + E) (strict: e1 |s0|_2 +
//     e0 |s1|_2 + e0 e1, e = a bound on the symbol's complex error), times
//     sqrt2 for QPSK's ||di| - |dr||, not for BPSK's |dr| -- flags its stream
//     (so does exact silence: every zero product is flagged);
//   * a flagged stream's batch is recomputed by the serial row-layout kernels
//     (psk_kernels.hip: bit-exact), launched behind these ones and gated on
//     the flag count on the device (they exit at once when it is zero).
// Unflagged decisions are the reference's bit for bit under strict mode; under
// the default they are whenever the measured premise holds for the input.
//
// Kernels (grid.y = stream, lanes = chunks; no LDS, no barriers):
//   KS0 k_split_bp_state_fwd / _bwd (default; AMR_PSK_SPLIT_CONV=0: off): a
//                        wave per chunk computes its band-pass start state by
//                        convolution -> zs [B][c1][8], KS1 / KS2 then run only
//                        their L outputs (no w1-step warm-up)
//   KS1 k_split_bp_fwd   ext(x) -> y1 [B][m1]   (+ the stream's peak |ext x|, the
//                        extension -- from the host's edge table for a raw
//                        integer capture (odd_ext.h) -- included)
//   KS2 k_split_bp_bwd   y1 reversed -> f [B][n]
//   KS3 k_split_lp_fwd   lane = (chunk, component): f * lo, odd ext -> y3 [B][2][m2]
//   KS4 k_split_lp_bwd   y3 reversed -> symbol samples sym [B][S][2]
//   KB1-KB4 k_split_strict_e1 / _e2 / _x / _e (strict mode only; thread =
//                        (block or symbol, stream); KB1 / KB2: split_bound.h):
//                        the block step bounds -> per-symbol bound e [B][S]
//   KS5 k_split_slice    thread = (stream, word): numpy's fma differential
//                        product, the sector / sign decision, the margin
//                        check -> words, flag, count
// then k_sync_pack (util_kernels.hip) and the gated serial fallback (api.cpp).
// Each step is the lane kernels' arithmetic (psk_common.h df2t_step /
// bp_step_zo / lp_step), so a chunk's recursion is scipy's operation for
// operation from its start state (oracle/amr_oracle.c oracle_psk_split_symbols
// reproduces these symbols exactly).
#include <math.h>
#include <stdlib.h>

#include "amr_internal.h"
#include "psk_common.h"
#include "split_bound.h"
#include "split_chain.h"

namespace amr {

template <bool ZO>
__device__ __forceinline__ double split_bp_step(double (&z)[8], const Iir& f, double x) {
  if constexpr (ZO) return bp_step_zo(z, f, x);
  else return df2t_step<8>(z, f, x);
}
template <bool ZO>
__device__ __forceinline__ void split_bp_warm(double (&z)[8], const Iir& f, double x) {
  if constexpr (ZO) (void)bp_warm_zo(z, f, x);
  else (void)bp_warm(z, f, x);
}
template <bool SYM>
__device__ __forceinline__ double split_lp_step(double (&z)[4], const Iir& f, double x) {
  if constexpr (SYM) return lp_step(z, f, x);
  else return df2t_step<4>(z, f, x);
}

// STRICT (split_bound.h StepBound): the pre-step states' sum_{i>=1} |z_i| of
// one band-pass step, z1..z7 in this pairing
__device__ __forceinline__ double step_bound_pre(const double (&z)[8]) {
  return ((fabs(z[1]) + fabs(z[2])) + (fabs(z[3]) + fabs(z[4]))) + ((fabs(z[5]) + fabs(z[6])) + fabs(z[7]));
}
// STRICT: stream s's scratch row, and KS0's bound into its slot off
__device__ __forceinline__ double* strict_sc(const PskSplit& sp, int64_t s) { return sp.rows.sc + s * sp.rows.sstride; }
__device__ __forceinline__ ConvBound strict_conv_bound(const PskSplit& sp, int64_t s, int64_t off) {
  return ConvBound{sp.sb.kabs, sp.sb.z0abs, sp.sb.gam, strict_sc(sp, s) + off};
}

// KS0 (sp.conv): a band-pass chunk's start state without a warm-up.  The
// state before output o0 of a pass that starts at 0 from zi v0 is
//   Z0[o0] v0 + sum_{m < o0} K[m] v(o0 - 1 - m)
// (K, Z0: the filter's state responses, api.cpp split_state_tables); the
// w1-step warm-up computes the same map truncated at m < w1 (the zero start),
// in w1 dependent steps of one lane.  Here it is a dot product over a whole
// wave: lane l takes m = l (mod 64) in ascending order (FMA), then a
// butterfly sum over the lanes (lane 0's order: ((p0 + p1) + (p2 + p3)) ...;
// oracle/amr_oracle.c conv_state restates it), the Z0 term while o0 <= w1.
// Chunk 0 keeps scipy's zi * v0.  One wave per chunk, four per workgroup
// (split_chain.h split_conv_state).
template <typename T, bool ST>
__global__ __launch_bounds__(256) void k_split_bp_state_fwd(PskBuffers buf, PskParams p, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= sp.c1) return;   // whole waves
  const T* __restrict__ x = reinterpret_cast<const T*>(buf.x) + s * buf.x_stride;
  const int64_t n = p.n;
  const int pad = p.pad1;
  const OddExt<T> ox(x, buf.edge, s, n, pad);
  split_conv_state<8, ST>(
      sp.ktab, sp.z0tab, sp.w1, c * sp.L, ox.left(0),
      [&](int64_t j) -> double {
        if (j < pad) return ox.left(j);
        if (j < pad + n) return In<T>::cvt(x[j - pad]);
        return ox.right(j - pad - n);
      },
      sp.zs + (s * sp.c1 + c) * 8,
      ST ? strict_conv_bound(sp, s, strict_off_ds1(sp.rows) + c) : ConvBound{});
}

template <bool ST>
__global__ __launch_bounds__(256) void k_split_bp_state_bwd(PskBuffers buf, PskParams p, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= sp.c1) return;
  const int64_t m1 = p.m1;
  const double* __restrict__ y1 = sp.y1 + s * m1;
  split_conv_state<8, ST>(
      sp.ktab, sp.z0tab, sp.w1, c * sp.L, y1[m1 - 1], [&](int64_t k) { return y1[m1 - 1 - k]; },
      sp.zs + (s * sp.c1 + c) * 8,
      ST ? strict_conv_bound(sp, s, strict_off_ds2(sp.rows) + c) : ConvBound{});
}

// KS1: the band-pass's forward pass over ext(x) (odd extension in the input's
// precision, In<T>), outputs [o0, o1) of chunk c
template <typename T, bool ZO, bool ST>
__global__ __launch_bounds__(64) void k_split_bp_fwd(PskBuffers buf, PskParams p, Iir f, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= sp.c1) return;
  const T* __restrict__ x = reinterpret_cast<const T*>(buf.x) + s * buf.x_stride;
  const int64_t n = p.n, m1 = p.m1;
  const int pad = p.pad1;
  const int64_t o0 = c * sp.L, o1 = o0 + sp.L < m1 ? o0 + sp.L : m1;
  const OddExt<T> ox(x, buf.edge, s, n, pad);
  double z[8];
  int64_t j = split_chunk_start(z, sp.conv ? sp.zs + (s * sp.c1 + c) * 8 : nullptr, f.zi,
                                [&] { return ox.left(0); }, o0, sp.w1);
  double* __restrict__ y1 = sp.y1 + s * m1;
  unsigned long long pk = 0;
  // ST: this chunk's step bounds (D1 blocks, the largest) and largest |y1|
  [[maybe_unused]] StepBound acc{sp.sb.kx, sp.sb.ky, ST ? strict_sc(sp, s) + strict_off_d1(sp.rows) : nullptr};
  [[maybe_unused]] double ymax = 0.0;
  auto out = [&](int64_t jj, double e) {
    if constexpr (ST) {
      const double sz = step_bound_pre(z);
      const double y = split_bp_step<ZO>(z, f, e);
      y1[jj] = y;
      acc.add(sz, e, y, jj);
      ymax = fmax(ymax, fabs(y));                 // (NaN / inf input: the peak test flags the stream)
    } else {
      y1[jj] = split_bp_step<ZO>(z, f, e);
    }
    const unsigned long long b = abs_bits(e);
    pk = b > pk ? b : pk;
  };
  auto body = [&](int64_t jj, double e) {
    if (jj < o0) split_bp_warm<ZO>(z, f, e);
    else out(jj, e);
  };
  // head extension, the samples themselves, tail extension
  for (; j < o1 && j < pad; ++j) body(j, ox.left(j));
  const int64_t jm = o1 < pad + n ? o1 : pad + n;
  if (j < jm) {
    split_chain_2(
        j, o0, jm, fwd_blocks(x - pad, [](T v) { return In<T>::cvt(v); }),
        [&](int64_t jj) { return In<T>::cvt(x[jj - pad]); },
        [&](int64_t, double e) { split_bp_warm<ZO>(z, f, e); }, out);
    j = jm;
  }
  for (; j < o1; ++j) body(j, ox.right(j - pad - n));
  atomicMax(&sp.peak[s], pk);
  if constexpr (ST) {
    acc.finish(o1 - 1);
    atomicMax(sp.bnd + s * 8 + 0, abs_bits(acc.dmax));
    atomicMax(sp.bnd + s * 8 + 2, abs_bits(ymax));
  }
}

// KS2: the band-pass's backward pass (scipy runs lfilter over y1 reversed,
// from zi * y1[-1]); chunk c covers reversed positions [o0, o1), i.e. f[i] for
// i = m1 - 1 - k - pad
template <bool ZO, bool ST>
__global__ __launch_bounds__(64) void k_split_bp_bwd(PskBuffers buf, PskParams p, Iir f, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= sp.c1) return;
  const int64_t n = p.n, m1 = p.m1;
  const int pad = p.pad1;
  const double* __restrict__ y1 = sp.y1 + s * m1;
  double* __restrict__ fo = sp.f + s * n;
  const int64_t o0 = c * sp.L, o1 = o0 + sp.L < m1 ? o0 + sp.L : m1;
  double z[8];
  const int64_t k = split_chunk_start(z, sp.conv ? sp.zs + (s * sp.c1 + c) * 8 : nullptr, f.zi,
                                      [&] { return y1[m1 - 1]; }, o0, sp.w1);
  // ST: this chunk's step bounds (D2 blocks, the largest) and largest |f|
  [[maybe_unused]] StepBound acc{sp.sb.kx, sp.sb.ky, ST ? strict_sc(sp, s) + strict_off_d2(sp.rows) : nullptr};
  [[maybe_unused]] double fmx = 0.0;
  split_chain_2(
      k, o0, o1, bwd_blocks(y1, m1 - 1), [&](int64_t kk) { return y1[m1 - 1 - kk]; },
      [&](int64_t, double v) { split_bp_warm<ZO>(z, f, v); },
      [&](int64_t kk, double v) {
        [[maybe_unused]] double sz = 0.0;
        if constexpr (ST) sz = step_bound_pre(z);
        const double y = split_bp_step<ZO>(z, f, v);
        const int64_t i = m1 - 1 - kk - pad;
        if (i >= 0 && i < n) {
          fo[i] = y;
          if constexpr (ST) fmx = fmax(fmx, fabs(y));
        }
        if constexpr (ST) acc.add(sz, v, y, kk);
      });
  if constexpr (ST) {
    acc.finish(o1 - 1);
    atomicMax(sp.bnd + s * 8 + 3, abs_bits(acc.dmax));
    atomicMax(sp.bnd + s * 8 + 5, abs_bits(fmx));
  }
}

// KS3: the low-pass's forward pass of one component of the baseband
// (f + 0j) * lo (numpy's complex multiply: per component f * lo_c, except
// bb[0], whose addend -(0 * lo_im) / 0 * lo_re the plan's lo table carries --
// as k_lp_lane), odd extension 2 * x0 - x[k] per component
template <bool SYM>
__global__ __launch_bounds__(64) void k_split_lp_fwd(PskBuffers buf, PskParams p, Iir f, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= 2 * sp.c2) return;
  const int comp = (int)(q & 1);
  const int64_t c = q >> 1;
  const int64_t n = p.n, m2 = p.m2;
  const int pad = p.pad2;
  const double* __restrict__ fi = sp.f + s * n;
  const double* __restrict__ loc = buf.lo2 + (size_t)comp * n;
  const double* lo4 = buf.lo + 2 * comp;
  auto Xm = [&](int64_t i) { return fi[i] * loc[i]; };
  const double x0 = fi[0] * lo4[0] + lo4[1];
  const double xl = Xm(n - 1);
  const int64_t o0 = c * sp.L, o1 = o0 + sp.L < m2 ? o0 + sp.L : m2;
  double z[4];
  int64_t j = split_chunk_start(z, nullptr, f.zi, [&] { return 2.0 * x0 - Xm(pad); }, o0, sp.w2);
  double* __restrict__ y3 = sp.y3 + ((size_t)s * 2 + comp) * m2;
  auto body = [&](int64_t jj, double e) {
    const double y = split_lp_step<SYM>(z, f, e);
    if (jj >= o0) y3[jj] = y;
  };
  for (; j < o1 && j <= pad; ++j) body(j, j < pad ? 2.0 * x0 - Xm(pad - j) : x0);
  const int64_t jm = o1 < pad + n ? o1 : pad + n;
  if (j < jm) {
    split_chain_2(
        j, o0, jm,
        [&](int64_t jj, double (&v)[kSplitRun]) {
          double a[kSplitRun], l[kSplitRun];
          run_load<kSplitRun>(fi + (jj - pad), a);
          run_load<kSplitRun>(loc + (jj - pad), l);
#pragma unroll
          for (int q = 0; q < kSplitRun; ++q) v[q] = a[q] * l[q];
        },
        [&](int64_t jj) { return Xm(jj - pad); },
        [&](int64_t, double e) { (void)split_lp_step<SYM>(z, f, e); },
        [&](int64_t jj, double e) { y3[jj] = split_lp_step<SYM>(z, f, e); });
    j = jm;
  }
  for (; j < o1; ++j) body(j, 2.0 * xl - Xm(n - 2 - (j - pad - n)));
}

// KS4: the low-pass's backward pass; the symbol samples baseband[first::sps]
// (modem.py:92, 209) go to sym [B][S][re, im]
template <bool SYM>
__global__ __launch_bounds__(64) void k_split_lp_bwd(PskBuffers buf, PskParams p, Iir f, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (q >= 2 * sp.c2) return;
  const int comp = (int)(q & 1);
  const int64_t c = q >> 1;
  const int64_t n = p.n, m2 = p.m2, S = p.n_sym, first = p.first, sps = p.sps;
  const int pad = p.pad2;
  const double* __restrict__ y3 = sp.y3 + ((size_t)s * 2 + comp) * m2;
  double* __restrict__ so = sp.sym + (size_t)s * S * 2 + comp;
  const int64_t o0 = c * sp.L, o1 = o0 + sp.L < m2 ? o0 + sp.L : m2;
  double z[4];
  const int64_t k = split_chunk_start(z, nullptr, f.zi, [&] { return y3[m2 - 1]; }, o0, sp.w2);
  // over the outputs, sample i = m2 - 1 - k - pad falls by one per step:
  // r = (i - first) mod sps counts down to the next symbol sample
  const int64_t i0 = m2 - 1 - (k > o0 ? k : o0) - pad;
  int64_t r = ((i0 - first) % sps + sps) % sps;
  split_chain_2(
      k, o0, o1, bwd_blocks(y3, m2 - 1), [&](int64_t kk) { return y3[m2 - 1 - kk]; },
      [&](int64_t, double v) { (void)split_lp_step<SYM>(z, f, v); },
      [&](int64_t kk, double v) {
        const double y = split_lp_step<SYM>(z, f, v);
        const int64_t i = m2 - 1 - kk - pad;
        if (r == 0 && i >= first && i < n) so[(i - first) / sps * 2] = y;
        r = r == 0 ? sps - 1 : r - 1;
      });
}

// KB (STRICT; split_strict.h): four grid-wide stages (grid = block tiles x
// streams; the per-stream maxima meet in bnd's free slots by atomicMax) turn
// KS0-KS2's per-block step bounds and per-chunk start bounds into a bound e(k)
// on each symbol component's |split - reference|:
//   KB1 E1[J], KB2 E2[J]  the band-pass's forward and backward pass at output
//              block J (split_bound.h strict_e1_block / strict_e2_block)
//   KB3 X[fb]  the mixer's output error over sample block fb
//   KB4 e(k)   the symbol's complex error: lpc[k] x the largest X within the
//              low-pass's reach of symbol k (and the extension's source blocks)
//              + the cut remainder (one complex sum through the unit-modulus
//              mixer), + sqrt2 x the per-component roundings (mixer, c3 P3)
// A stream past the a-posteriori caps gets e = inf: flagged.  The final factor
// 1 + 2^-30 covers the sums' own rounding.
__device__ __forceinline__ StrictRow kb_row(const PskSplit& sp, int64_t s) {
  return strict_row(sp.sb, sp.rows, sp.bnd, s, sp.peak[s]);
}

__global__ __launch_bounds__(kKbThreads) void k_split_strict_e1(PskParams p, PskSplit sp) {
  const int64_t J = (int64_t)blockIdx.x * kKbThreads + threadIdx.x;
  const StrictRow k = kb_row(sp, blockIdx.y);
  const StrictE1 o = strict_e1_block(sp.sb, sp.rows, k, J, sp.L / kStrictBlk);
  (void)p;
  wave_max_to(k.bw + 1, o.e, J < sp.rows.nb1);
  wave_max_to(k.bw + 4, o.st, J < sp.rows.nb1);
}

__global__ __launch_bounds__(kKbThreads) void k_split_strict_e2(PskParams p, PskSplit sp) {
  const int64_t J = (int64_t)blockIdx.x * kKbThreads + threadIdx.x;
  const StrictRow k = kb_row(sp, blockIdx.y);
  const double e = strict_e2_block(sp.sb, sp.rows, k, J, sp.L / kStrictBlk, p.m1);
  wave_max_to(k.bw + 6, e, J < sp.rows.nb1);
}

__global__ __launch_bounds__(kKbThreads) void k_split_strict_x(PskParams p, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t fb = (int64_t)blockIdx.x * kKbThreads + threadIdx.x;
  const StrictRow k = kb_row(sp, s);
  const int64_t n = p.n;
  const double* e2 = k.sc + strict_off_e2(sp.rows);
  const double fm = bnd_get(k.bw, 5) + bnd_get(k.bw, 6);
  double x = 0.0;
  const bool live = fb < sp.nbs;
  if (live) {
    const int64_t ilo = 16 * fb, ihi = 16 * fb + 15 < n - 1 ? 16 * fb + 15 : n - 1;
    const double F = fmax(e2[(ilo + p.pad1) / kStrictBlk], e2[(ihi + p.pad1) / kStrictBlk]);
    x = F * (1.0 + 0x1p-50) + 0x1.02p-52 * fm;
    k.sc[strict_off_x(sp) + fb] = x;
  }
  wave_max_to(k.bw + 7, x, live);
}

__global__ __launch_bounds__(kKbThreads) void k_split_strict_e(PskParams p, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t kk = (int64_t)blockIdx.x * kKbThreads + threadIdx.x;
  const StrictRow k = kb_row(sp, s);
  const int64_t n = p.n, nbs = sp.nbs, S = p.n_sym;
  const double* xb = k.sc + strict_off_x(sp);
  double* eo = k.sc + strict_off_e(sp);
  const double E1max = bnd_get(k.bw, 1), Fmax = bnd_get(k.bw, 6), Xmax = bnd_get(k.bw, 7);
  const double fm = bnd_get(k.bw, 5) + Fmax;
  const double P3 = 3.0 * (fm + Xmax);
  const bool ok = E1max <= k.cap1 && Fmax <= k.cap2;      // false for NaN
  if (kk < S) {
    // the symbol's complex error: the band-pass error f reaches it through the
    // mixer's unit-modulus lo (|lo| <= 1 + 2u) and the real low-pass kernel, so
    // as one complex sum, |.|_2 <= (lpc xw + lp_tail Xmax)(1 + 2^-50); the
    // per-component roundings (the mixer's rho, the low-pass's own c3 P3) are
    // independent per component: sqrt2 on those alone
    const double rho = 0x1.02p-52 * fm;
    const double t0 = sp.lp_tail * Xmax, t1 = 0x1.6a09e667f3bcdp+0 * ((sp.lpc[kk] + sp.lp_tail) * rho + sp.c3 * P3);
    const int64_t t = p.first + kk * p.sps;
    const int64_t lo = t - sp.lp_rad - p.pad2, hi = t + sp.lp_rad + p.pad2;
    const int64_t flo = lo > 0 ? lo / kStrictBlk : 0, fhi = (hi < n - 1 ? hi : n - 1) / kStrictBlk;
    double xw = fmax(xb[0], xb[nbs - 1]);
    for (int64_t fb = flo; fb <= fhi; ++fb) xw = fmax(xw, xb[fb]);
    const double e = (1.0 + 0x1p-30) * (__builtin_fma(sp.lpc[kk], xw, t0) * (1.0 + 0x1p-50) + t1);
    eo[kk] = ok ? e : __builtin_inf();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* scal = eo + S;
    scal[0] = E1max;
    scal[1] = Fmax;
    scal[2] = Xmax;
    scal[3] = ok ? P3 : -P3;
  }
}

// an upper bound on |s|_2 = hypot(re, im): the rounded sqrt of the rounded
// sum of squares is within 4u of it, so x (1 + 2^-50) covers it; |s|_1 (a1,
// always an upper bound) where the squares could underflow or it is smaller
__device__ __forceinline__ double norm2_up(double re, double im, double a1) {
  if (!(a1 >= 0x1p-500 && a1 <= 0x1p500)) return a1;
  const double r = sqrt(__builtin_fma(re, re, im * im)) * (1.0 + 0x1p-50);
  return r < a1 ? r : a1;
}

// KS5: one thread per (stream, 32-bit word): the differential products of the
// word's symbols in numpy's fma form, the reference's decision (qpsk_dibit /
// real < 0, as K4a), and the margin: a symbol's error <= E, so |d error|_2
// <= E (|s0|_2 + |s1|_2 + E), times sqrt2 for QPSK's L1 use (+ forming d's own
// rounding; |s|_2 from above, norm2_up -- round 6; before it |s|_1 and the
// sqrt2 for BPSK too, up to 2x wider);
// a decision closer than that to its boundary -- QPSK's diagonals
// ||di| - |dr|| (K4a's 2^-29 sliver on top), BPSK's dr = 0 -- flags the stream
__global__ __launch_bounds__(64) void k_split_slice(PskBuffers buf, PskParams p, PskSplit sp) {
  const int64_t s = blockIdx.y;
  const int64_t w = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (w >= p.n_words) return;
  const bool qpsk = p.kind == kQpsk;
  const int per = qpsk ? 16 : 32;
  const int64_t S = p.n_sym;
  const int64_t k0 = w * per;
  const int64_t k1 = k0 + per < S - 1 ? k0 + per : S - 1;
  const double peak = __longlong_as_double((long long)sp.peak[s]);
  const double E = sp.kappa * peak;
  // tiny / huge / non-finite input: every decision goes the serial way
  bool flag = !(peak >= 0x1p-400 && peak <= 0x1p400);
  // STRICT: |symbol error|_2 <= e(k) (KB4; inf when the stream's caps failed);
  // else kappa * peak for every symbol
  const double sq2 = 0x1.6a09e667f3bcdp+0;
  const double* eo = sp.strict ? strict_sc(sp, s) + strict_off_e(sp) : nullptr;
  auto esym = [&](int64_t k) { return eo[k]; };
  const double* __restrict__ sy = sp.sym + (size_t)s * S * 2;
  uint32_t word = 0;
  double br = sy[2 * k0], bi0 = sy[2 * k0 + 1];
  double e0 = sp.strict ? esym(k0) : E;
  for (int64_t k = k0; k < k1; ++k) {
    const double pr = sy[2 * (k + 1)], pim = sy[2 * (k + 1) + 1];
    const double bi = -bi0;
    const double dr = __builtin_fma(pr, br, -(pim * bi));
    const double a0 = fabs(br) + fabs(bi), a1 = fabs(pr) + fabs(pim);
    const double r0 = norm2_up(br, bi, a0), r1 = norm2_up(pr, pim, a1);
    const double e1 = sp.strict ? esym(k + 1) : E;
    // |d error|_2 <= e1 |s0|_2 + e0 |s1|_2 + e0 e1 (r: upper bounds on |s|_2); QPSK's
    // |di| - |dr| moves by at most its L1 norm (x sqrt2), BPSK's dr by the L2 norm itself
    const double dx = sp.strict ? (e1 * r0 + e0 * r1) + e0 * e1 : E * (r0 + r1 + E);
    const double md = (qpsk ? sq2 * dx : dx) * (1.0 + 0x1p-40) + 0x1p-48 * (a0 * a1);
    e0 = e1;
    if (qpsk) {
      const double di = __builtin_fma(pr, bi, pim * br);
      const double adr = fabs(dr), adi = fabs(di);
      if (!(fabs(adi - adr) > md + 0x1p-29 * (adr + adi))) flag = true;
      word |= qpsk_dibit(dr, di) << (30 - 2 * (int)(k & 15));
    } else {
      if (!(fabs(dr) > md)) flag = true;
      word |= (dr < 0 ? 1u : 0u) << (31 - (int)(k & 31));
    }
    br = pr;
    bi0 = pim;
  }
  buf.words[(size_t)s * p.n_words + w] = word;
  if (flag && atomicOr(&sp.flag[s], 1) == 0) atomicAdd(sp.count, 1);
}

// (KS0 +) KS1 + (KS0 +) KS2
hipError_t launch_psk_split_bp(const PskBuffers& b, const PskParams& p, const Iir& bp, const PskSplit& sp,
                               hipStream_t st) {
  const int64_t B = b.n_streams;
  if (B < 1) return hipSuccess;
  if (B > 65535 || bp.nt != 9) return hipErrorInvalidValue;
  const dim3 blk(64), g1((unsigned)((sp.c1 + 63) / 64), (unsigned)B);
  const dim3 blk0(256), g0((unsigned)((sp.c1 + 3) / 4), (unsigned)B);
  const bool zo = p.bp_zero_odd && p.bp_sym;
  if (sp.conv && (!sp.ktab || !sp.z0tab || !sp.zs)) return hipErrorInvalidValue;
  // the strict bound covers the convolution starts only (no FMA warm-ups)
  if (sp.strict && (!sp.conv || !sp.bnd || !sp.sb.kabs || !sp.sb.z0abs || !sp.lpc)) return hipErrorInvalidValue;
  const bool stv = sp.strict != 0;
#define KS0F(T) \
  do { \
    if (stv) hipLaunchKernelGGL((k_split_bp_state_fwd<T, true>), g0, blk0, 0, st, b, p, sp); \
    else hipLaunchKernelGGL((k_split_bp_state_fwd<T, false>), g0, blk0, 0, st, b, p, sp); \
  } while (0)
#define KS1F(T) \
  do { \
    if (zo) { \
      if (stv) hipLaunchKernelGGL((k_split_bp_fwd<T, true, true>), g1, blk, 0, st, b, p, bp, sp); \
      else hipLaunchKernelGGL((k_split_bp_fwd<T, true, false>), g1, blk, 0, st, b, p, bp, sp); \
    } else { \
      if (stv) hipLaunchKernelGGL((k_split_bp_fwd<T, false, true>), g1, blk, 0, st, b, p, bp, sp); \
      else hipLaunchKernelGGL((k_split_bp_fwd<T, false, false>), g1, blk, 0, st, b, p, bp, sp); \
    } \
  } while (0)
  if (sp.conv) {
    switch (b.dtype) {
      case kF32: KS0F(float); break;
      case kF64: KS0F(double); break;
      case kI16: KS0F(int16_t); break;
      default: return hipErrorInvalidValue;
    }
  }
  switch (b.dtype) {
    case kF32: KS1F(float); break;
    case kF64: KS1F(double); break;
    case kI16: KS1F(int16_t); break;
    default: return hipErrorInvalidValue;
  }
#undef KS1F
#undef KS0F
  if (sp.conv) {
    if (stv) hipLaunchKernelGGL(k_split_bp_state_bwd<true>, g0, blk0, 0, st, b, p, sp);
    else hipLaunchKernelGGL(k_split_bp_state_bwd<false>, g0, blk0, 0, st, b, p, sp);
  }
  if (zo) {
    if (stv) hipLaunchKernelGGL((k_split_bp_bwd<true, true>), g1, blk, 0, st, b, p, bp, sp);
    else hipLaunchKernelGGL((k_split_bp_bwd<true, false>), g1, blk, 0, st, b, p, bp, sp);
  } else {
    if (stv) hipLaunchKernelGGL((k_split_bp_bwd<false, true>), g1, blk, 0, st, b, p, bp, sp);
    else hipLaunchKernelGGL((k_split_bp_bwd<false, false>), g1, blk, 0, st, b, p, bp, sp);
  }
  return hipGetLastError();
}

// KS3 + KS4
hipError_t launch_psk_split_lp(const PskBuffers& b, const PskParams& p, const Iir& lp, const PskSplit& sp,
                               hipStream_t st) {
  const int64_t B = b.n_streams;
  if (B < 1) return hipSuccess;
  if (B > 65535 || lp.nt != 5) return hipErrorInvalidValue;
  const dim3 blk(64), g2((unsigned)((2 * sp.c2 + 63) / 64), (unsigned)B);
  if (p.lp_sym) {
    hipLaunchKernelGGL((k_split_lp_fwd<true>), g2, blk, 0, st, b, p, lp, sp);
    hipLaunchKernelGGL((k_split_lp_bwd<true>), g2, blk, 0, st, b, p, lp, sp);
  } else {
    hipLaunchKernelGGL((k_split_lp_fwd<false>), g2, blk, 0, st, b, p, lp, sp);
    hipLaunchKernelGGL((k_split_lp_bwd<false>), g2, blk, 0, st, b, p, lp, sp);
  }
  return hipGetLastError();
}

// KS5
hipError_t launch_psk_split_slice(const PskBuffers& b, const PskParams& p, const PskSplit& sp, hipStream_t st) {
  const int64_t B = b.n_streams;
  if (B < 1 || p.n_words < 1 || p.n_bits < 1) return hipSuccess;
  if (B > 65535) return hipErrorInvalidValue;
  const dim3 blk(64), g5((unsigned)((p.n_words + 63) / 64), (unsigned)B);
  if (sp.strict) {
    if (!sp.rows.sc || sp.L % kStrictBlk != 0) return hipErrorInvalidValue;
    auto g = [&](int64_t units) { return dim3((unsigned)((units + kKbThreads - 1) / kKbThreads), (unsigned)B); };
    hipLaunchKernelGGL(k_split_strict_e1, g(sp.rows.nb1), dim3(kKbThreads), 0, st, p, sp);
    hipLaunchKernelGGL(k_split_strict_e2, g(sp.rows.nb1), dim3(kKbThreads), 0, st, p, sp);
    hipLaunchKernelGGL(k_split_strict_x, g(sp.nbs), dim3(kKbThreads), 0, st, p, sp);
    hipLaunchKernelGGL(k_split_strict_e, g(p.n_sym), dim3(kKbThreads), 0, st, p, sp);
  }
  hipLaunchKernelGGL(k_split_slice, g5, blk, 0, st, b, p, sp);
  return hipGetLastError();
}

}  // namespace amr
