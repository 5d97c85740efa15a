// fsk_api.cpp -- C ABI of the FSK demodulator and the FFT/Hilbert entry
// points (include/amr.h).  Host code; compiled by hipcc.
//
// Pipeline per call (all on the plan's stream):
//   F1  k_fsk_bandpass2         x -> z = f_mark + i f_space           [B][n] c128
//   F2  H[z] = IFFT_n(-i sgn(k) FFT_n(z)) in three passes z -> u -> v -> cmp,
//       the last forming both envelopes: bit = |a_mark| > |a_space|   [B][n/8] u8
//   F3  k_fsk_decide + k_sync_pack  cmp bits -> words -> bytes
// A length that is not 5-smooth runs each FFT_n as a Bluestein convolution of
// length M (u, v then hold M-long rows).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "fsk_exact.h"
#include "fft.h"
#include "iir_design.h"
#include "plan_core.h"
#include "split_strict.h"

namespace amr {
hipError_t launch_fsk_bandpass(int, const void*, int64_t, int64_t, double*, double2*, const FskParams&,
                               const FskIir&, hipStream_t);
hipError_t launch_fsk_decide(const uint8_t*, uint32_t*, int64_t, const FskParams&, hipStream_t);
hipError_t launch_fsk_split(int, const void*, int64_t, int64_t, double2*, const FskParams&, const FskIir&,
                            const FskSplit&, hipStream_t);
int64_t fsk_bandpass_scratch_bytes(int64_t n_streams, int64_t n, int pad);
}  // namespace amr

using namespace amr;

namespace {

// Device FFT of one logical length n, run as one of
//   two-pass   M = n = n1 * n2 (launch_fft / launch_fft_filter: the fused paths)
//   six-step   M = n = L1 * L2 past the two-pass limit: transpose, L2-point
//              row FFTs, twiddle-transpose, L1-point row FFTs, transpose
//   Bluestein  n not plannable: a length-M circular convolution, M >= 2n-1,
//              itself two-pass or six-step
// Plain-order epilogues after a six-step / Bluestein transform go through the
// Bluestein post kernel with a unit chirp.
struct FftPlan {
  int64_t n = 0;
  int64_t M = 0;                 // transform length run: n, or the Bluestein length
  bool bluestein = false;
  bool six = false;              // M runs six-step
  FftDesc d{};                   // length M (two-pass)
  FftDesc d1{}, d2{};            // lengths L1, L2 (six-step)
  int64_t L1 = 0, L2 = 0;
  const double2* tw6_lo = nullptr;   // W_M^t, t < 256
  const double2* tw6_hi = nullptr;   // W_M^(256 t)
  const double2* chirp = nullptr;    // Bluestein chirp, or all ones (six-step, plain epilogues)
  const double2* bhat = nullptr;     // FFT_M(bw) (two-pass Bluestein filter table)
  const double2* bhat_c = nullptr;   // conj(FFT_M(bw)) (six-step Bluestein: applied by the post kernel)
  int64_t max_batch = 0;
  // what the plan owns on the device (freed with it; a plan's fsk_plan_free
  // releases them with the plan's own buffers): the tables the pointers above
  // look into, and the six-step scratch [max_batch][M] x 2
  struct Mem {
    std::vector<DevBuf> tables;
    DevBuf s1, s2;
  } mem;
};

// device copy of interleaved host values
hipError_t upload(FftPlan& f, const std::vector<double>& h, const double2** out) {
  DevBuf t;
  hipError_t e = t.reserve((int64_t)h.size() * 8 + 16, nullptr);
  if (e != hipSuccess) return e;
  e = hipMemcpy(t.get(), h.data(), h.size() * 8, hipMemcpyHostToDevice);
  *out = t.as<const double2>();
  f.mem.tables.push_back(std::move(t));
  return e;
}

// two-pass descriptor of length L (fft_split must succeed)
int desc_init(FftPlan& f, FftDesc& d, int64_t L) {
  int n1 = 0, n2 = 0;
  if (!fft_split(L, n1, n2)) return fail(AMR_E_INVALID, "FFT length " + std::to_string(L) + " does not split");
  const int64_t nhi = (L + 255) / 256;
  std::vector<double> host;
  auto put = [&](const std::vector<double>& w) { host.insert(host.end(), w.begin(), w.end()); };
  put(twiddles(n2, n2));
  put(twiddles(n1, n1));
  put(twiddles(L, 256));
  put(twiddles(L, nhi, 256));
  const double2* t = nullptr;
  HIP_TRY(upload(f, host, &t));
  d.n = L;
  d.n1 = n1;
  d.n2 = n2;
  if (!fill_fft_len(d.a, n2, t) || !fill_fft_len(d.c, n1, t + n2))
    return fail(AMR_E_INVALID, "FFT factor plan failed for n=" + std::to_string(L));
  d.tw_lo = t + n2 + n1;
  d.tw_hi = t + n2 + n1 + 256;
  return AMR_OK;
}

// X = FFT_M(in) (or the true inverse) by six steps; out may alias in; s1, s2 scratch.
hipError_t six_fft(const FftPlan& f, const double2* in, double2* out, int64_t batch, bool inverse, hipStream_t st) {
  if (batch > f.max_batch) return hipErrorInvalidValue;
  const int64_t L1 = f.L1, L2 = f.L2;
  double2 *const s1 = f.mem.s1.as<double2>(), *const s2 = f.mem.s2.as<double2>();
  // in[j1 + L1 j2] = [j2][j1] -> s1[j1][j2]
  hipError_t e = launch_transpose(in, s1, L2, L1, batch, nullptr, nullptr, false, st);
  // L2-point transforms of every row j1 -> s1[j1][k2]
  if (e == hipSuccess) e = launch_fft(s1, s2, s1, f.d2, batch * L1, inverse, st);
  // times W_M^(j1 k2), -> s2[k2][j1]
  if (e == hipSuccess) e = launch_transpose(s1, s2, L1, L2, batch, f.tw6_lo, f.tw6_hi, inverse, st);
  // L1-point transforms of every row k2 -> s2[k2][k1]
  if (e == hipSuccess) e = launch_fft(s2, s1, s2, f.d1, batch * L2, inverse, st);
  // X[k2 + L2 k1] = out[k1][k2]
  if (e == hipSuccess) e = launch_transpose(s2, out, L2, L1, batch, nullptr, nullptr, false, st);
  return e;
}

// IFFT_M(FFT_M(a) * FFT_M(bw)) in place in a (Bluestein's convolution), six-step
hipError_t six_conv(const FftPlan& f, double2* a, double2* tmp, int64_t batch, hipStream_t st) {
  FftEpi store{};
  store.mode = kStore;
  store.n = f.M;
  hipError_t e = six_fft(f, a, a, batch, false, st);
  if (e == hipSuccess) e = launch_bs_post(a, a, f.bhat_c, f.M, f.M, batch, false, store, st);   // * FFT(bw)
  if (e == hipSuccess) e = six_fft(f, a, tmp, batch, true, st);
  return e;
}

// How FFT_n runs (host only): two-pass (M = n = n1 * n2), six-step (M = n =
// L1 * L2) or Bluestein over a two-pass / six-step M.  False: no plan.
struct FftShape {
  int64_t M = 0;
  bool bluestein = false, six = false;
  int n1 = 0, n2 = 0;            // the two-pass split of M (when !six)
  int64_t L1 = 0, L2 = 0;        // the six-step split of M (when six)
};
bool fft_shape(int64_t n, FftShape& sh) {
  int a = 0, b = 0;
  if (fft_split(n, a, b)) {
    sh.M = n;
  } else if (fft_six_split(n, sh.L1, sh.L2)) {
    sh.M = n;
    sh.six = true;
  } else {
    sh.bluestein = true;
    sh.M = fft_good_size(2 * n - 1);
    if (sh.M < 0) return false;
    if (!fft_split(sh.M, a, b)) {
      if (!fft_six_split(sh.M, sh.L1, sh.L2)) return false;
      sh.six = true;
    }
  }
  if (!sh.six) fft_split(sh.M, sh.n1, sh.n2);
  return true;
}

// Plans FFT_n for up to max_batch rows; needs the stream for the Bluestein kernel FFT.
int fft_plan_init(FftPlan& f, int64_t n, hipStream_t st, int64_t max_batch) {
  static std::once_flag smem_once;
  static hipError_t smem_err = hipSuccess;
  std::call_once(smem_once, [] { smem_err = fft_configure_smem(); });
  HIP_TRY(smem_err);
  f.n = n;
  f.max_batch = max_batch;
  FftShape sh;
  if (!fft_shape(n, sh)) return fail(AMR_E_INVALID, "no FFT plan for length " + std::to_string(n));
  f.M = sh.M;
  f.bluestein = sh.bluestein;
  f.six = sh.six;
  const int64_t L1 = sh.L1, L2 = sh.L2;
  const int64_t M = f.M;
  if (f.six) {
    f.L1 = L1;
    f.L2 = L2;
    if (int rc = desc_init(f, f.d1, L1)) return rc;
    if (int rc = desc_init(f, f.d2, L2)) return rc;
    const int64_t nhi = (M + 255) / 256;
    std::vector<double> host = twiddles(M, 256);
    const std::vector<double> hi = twiddles(M, nhi, 256);
    host.insert(host.end(), hi.begin(), hi.end());
    const double2* t = nullptr;
    HIP_TRY(upload(f, host, &t));
    f.tw6_lo = t;
    f.tw6_hi = t + 256;
    HIP_TRY(f.mem.s1.reserve(max_batch * M * 16, nullptr));
    HIP_TRY(f.mem.s2.reserve(max_batch * M * 16, nullptr));
  } else {
    if (int rc = desc_init(f, f.d, M)) return rc;
  }
  if (!f.bluestein && !f.six) return AMR_OK;
  std::vector<double> w((size_t)(2 * n));
  if (f.bluestein) {
    // chirp w_j = exp(i pi j^2 / n); j^2 reduced mod 2n keeps the angle exact
    for (int64_t j = 0; j < n; ++j) {
      const int64_t r = (j * j) % (2 * n);
      const double ang = M_PI * (double)r / (double)n;
      w[(size_t)(2 * j)] = std::cos(ang);
      w[(size_t)(2 * j + 1)] = std::sin(ang);
    }
  } else {
    for (int64_t j = 0; j < n; ++j) w[(size_t)(2 * j)] = 1.0;   // unit chirp: plain epilogues
  }
  HIP_TRY(upload(f, w, &f.chirp));
  if (!f.bluestein) return AMR_OK;
  // convolution kernel bw[m] = w_m, bw[M-m] = w_m (0 < m < n), zero elsewhere; bhat = FFT_M(bw)
  std::vector<double> bw((size_t)(2 * M), 0.0);
  for (int64_t m = 0; m < n; ++m) {
    bw[(size_t)(2 * m)] = w[(size_t)(2 * m)];
    bw[(size_t)(2 * m + 1)] = w[(size_t)(2 * m + 1)];
    if (m > 0) {
      bw[(size_t)(2 * (M - m))] = w[(size_t)(2 * m)];
      bw[(size_t)(2 * (M - m) + 1)] = w[(size_t)(2 * m + 1)];
    }
  }
  const double2* bwd = nullptr;
  HIP_TRY(upload(f, bw, &bwd));
  f.mem.tables.emplace_back();
  HIP_TRY(f.mem.tables.back().reserve(M * (int64_t)sizeof(double2), nullptr));
  double2* bh = f.mem.tables.back().as<double2>();
  if (!f.six) {
    DevBuf tmp;
    HIP_TRY(tmp.reserve(M * (int64_t)sizeof(double2), nullptr));
    hipError_t e = launch_fft(bwd, tmp.as<double2>(), bh, f.d, 1, false, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // before tmp is freed
    HIP_TRY(e);
    f.bhat = bh;
  } else {
    // conj(FFT_M(bw)) by six steps (the post kernel multiplies by conj(w))
    hipError_t e = six_fft(f, bwd, bh, 1, false, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    HIP_TRY(e);
    std::vector<double> hb((size_t)(2 * M));
    HIP_TRY(hipMemcpy(hb.data(), bh, (size_t)M * 16, hipMemcpyDeviceToHost));
    for (int64_t m = 0; m < M; ++m) hb[(size_t)(2 * m + 1)] = -hb[(size_t)(2 * m + 1)];
    HIP_TRY(hipMemcpy(bh, hb.data(), (size_t)M * 16, hipMemcpyHostToDevice));
    f.bhat_c = bh;
  }
  return AMR_OK;
}

// out = FFT_n(in) or IFFT_n(in).  u, v: [batch][M] scratch; in != u; out != v.
hipError_t fft_c2c(const FftPlan& f, const double2* in, double2* u, double2* v, double2* out, int64_t batch,
                   bool inverse, hipStream_t st) {
  if (!f.bluestein) {
    if (f.six) return six_fft(f, in, out, batch, inverse, st);
    return launch_fft(in, u, out, f.d, batch, inverse, st);
  }
  FftEpi store{};
  store.mode = kStore;
  store.n = f.n;        // row stride of `out` (launch_fft_filter sets its own)
  hipError_t e = launch_bs_pre(in, u, f.chirp, f.n, f.M, batch, inverse, st);
  if (f.six) {
    if (e == hipSuccess) e = six_conv(f, u, v, batch, st);
  } else {
    if (e == hipSuccess) e = launch_fft_filter(u, v, u, v, f.d, batch, kMulTab, f.bhat, store, st);
  }
  if (e == hipSuccess) e = launch_bs_post(v, out, f.chirp, f.n, f.M, batch, inverse, store, st);
  return e;
}

// epi(IFFT_n(-i*sgn(k) * FFT_n(in))) = epi(H[in]), the Hilbert transform of
// each row (scipy.signal.hilbert(x).imag for real x).  u, v: [batch][M]
// scratch, in != u, v; a kStore / kEnvOut result lands in hilbert_out(f, u, v).
double2* hilbert_out(const FftPlan& f, double2* u, double2* v) { return (f.bluestein || f.six) ? v : u; }

hipError_t fft_hilbert(const FftPlan& f, const double2* in, double2* u, double2* v, int64_t batch, FftEpi epi,
                       hipStream_t st) {
  epi.n = f.n;
  if (!f.bluestein && !f.six) return launch_fft_filter(in, u, v, u, f.d, batch, kHilbert, nullptr, epi, st);
  const int64_t n = f.n, M = f.M;
  FftEpi store{};
  store.mode = kStore;
  FftEpi hil{};
  hil.mode = kHilbert;
  hil.n = n;
  hipError_t e = hipSuccess;
  if (!f.bluestein) {
    // six-step, M = n: W = -i sgn(k) FFT(in) -> v; IFFT via conj: FFT(conj W) -> v, post conj/scale + epi
    e = six_fft(f, in, u, batch, false, st);
    if (e == hipSuccess) e = launch_bs_post(u, v, f.chirp, n, n, batch, false, hil, st);
    if (e == hipSuccess) e = launch_bs_pre(v, u, f.chirp, n, n, batch, true, st);
    if (e == hipSuccess) e = six_fft(f, u, v, batch, false, st);
    if (e == hipSuccess) e = launch_bs_post(v, v, f.chirp, n, n, batch, true, epi, st);
    return e;
  }
  // forward: W = -i sgn(k) FFT_n(in) -> u (n-long rows)
  e = launch_bs_pre(in, u, f.chirp, n, M, batch, false, st);
  if (f.six) {
    if (e == hipSuccess) e = six_conv(f, u, v, batch, st);
  } else {
    if (e == hipSuccess) e = launch_fft_filter(u, v, u, v, f.d, batch, kMulTab, f.bhat, store, st);
  }
  if (e == hipSuccess) e = launch_bs_post(v, u, f.chirp, n, M, batch, false, hil, st);
  // inverse: epi(IFFT_n(W)) -> v / cmp
  if (e == hipSuccess) e = launch_bs_pre(u, v, f.chirp, n, M, batch, true, st);
  if (f.six) {
    if (e == hipSuccess) e = six_conv(f, v, u, batch, st);
  } else {
    if (e == hipSuccess) e = launch_fft_filter(v, u, v, u, f.d, batch, kMulTab, f.bhat, store, st);
  }
  if (e == hipSuccess) e = launch_bs_post(u, v, f.chirp, n, M, batch, true, epi, st);
  return e;
}

}  // namespace

struct amr_fsk_plan : PlanCore<AMR_TF_COUNT> {
  FskParams p{};
  FskIir f{};
  FftPlan fft{};
  int64_t max_streams = 0;
  int64_t out_cap = 0;
  // Every device buffer the plan owns (dev_mem.h DevBuf), in the sets the
  // byte totals below sum (fsk_scratch_bytes, fsk_split_bytes,
  // fsk_strict_bytes, fsk_out_staging_bytes); fsk_plan_free releases them
  // together, after the streams are drained and before they are destroyed.
  struct Mem {
    // HBM scratch, allocated with the plan (dd: by the first host entry)
    // natural layout (p.lc.on == 0): z [B][n], u / v [B][M] (u also F1's
    // checkpoint scratch).  Live-column layout (p.lc.on, amr_internal.h
    // LiveCols): z = [B][L | D] (n per stream), u = C [B][nl * n2] -- also F1's
    // checkpoint scratch and, on the host entries, the staged input -- and no v.
    DevBuf z, u, v;
    DevBuf dd;       // see keep_z below
    DevBuf cmp;      // [B][bits_stride] packed compare bits (fft.h fft_bits_stride)
    DevBuf words;    // [B][n_words]
    // the exact path (fsk_exact_kernels.hip)
    DevBuf xflags;   // [B / 32] F2's flags, bit s of word s / 32 (cleared by F1 every batch)
    DevBuf amb;      // [B] F1's ambiguity scale per stream
    DevBuf xlist;    // [B] flagged ordinal -> stream, then [1] the count
    DevBuf xslots;   // [n_slots][slot_doubles] envelope scratch
    DevBuf xbits;    // [B][bits_stride] the flagged streams' exact compare bits
    DevBuf xpool;    // pocketfft's twiddle / chirp tables of length n
    DevBuf xL;       // pocketfft's plans of length n (device copy)
    // the time-split F1, on the first split call: the forward outputs and
    // peaks of as many streams as the largest split call so far, and FS0's
    // tables [2][w][6] + [2][w + 1][6] with the zs states behind them
    DevBuf split_y1, split_peak, split_cz;
    // its STRICT mode: the tables, per-stream maxima [B][2][8] and scratch
    DevBuf strict_tab, strict_bnd, strict_sc;
    // staging for the host API
    DevBuf d_x;      // the staged input of a plan that does not keep z
    DevBuf d_out, d_len, d_sync, d_edge;   // one group, whole or not at all (reserve_all); d_edge:
                                           // amr_fsk_demod_host_edges' table [max_streams][2 pad]
  } mem;
  // keep_z (live layout with the exact path): the column pass writes the dead
  // tiles' transform to dd [B][nd * n2] instead of over z's dead columns, so
  // all of z (the band-pass output) survives F2 for the exact path; dd also
  // takes the host entries' staged input (>= 8 B per sample: nd >= n1 / 2).
  // dd (9.6 B per sample at FSK9600) is allocated by the first host entry,
  // which needs a staging buffer anyway; until then the device entries run
  // lean -- dead tiles in place, a flagged stream's F1 re-run from the
  // caller's x (E1) -- so a device-entry plan holds z + C only
  // (AMR_FSK_KEEPZ=1: dd at creation, every call keeps z; =0: never)
  bool keep_z = false;         // the plan can keep z (dd sized); a call does when dd is allocated
  // reservations, counted by amr_fsk_plan_scratch_bytes before the first host
  // entry allocates them: dd's size, and d_x's (0 with keep_z)
  int64_t dd_bytes = 0;
  int64_t staging_bytes = 0;
  // the exact path for streams with a compare inside F2's margin (fsk_exact_kernels.hip)
  bool exact_on = false;
  int32_t* xcount_host = nullptr;   // host-mapped: the count E3 last saw (FskExact count_hint)
  int32_t* xcount_dev = nullptr;    // its device pointer
  // the synchronous host entry (amr_fsk_demod_host) reads E0's count on the
  // host before the envelope kernels: none flagged -> E1-E3 are not launched
  // at all; else E2's grid is sized from this batch's own count
  bool count_sync = false;
  // the counts E3 reported before the last kHintDepth launches:
  // E2's grid follows their maximum, so one clean batch between flagged ones
  // does not shrink the grid of the next flagged batch to kIdleGrid
  static constexpr int kHintDepth = 8;
  int32_t hint_hist[kHintDepth]{};
  int hint_pos = 0;
  bool x_lean = false;         // pf_hilbert_lean: E2 runs the lean fused kernel
  int64_t slot_doubles = 0;
  int n_slots = 0;
  bool ran_exact = false;      // the last call ran the exact path (its count is in xlist[max_streams])
  int exact_mode = 1;          // amr_fsk_plan_set_exact_mode: 0 off, 1 F2's flags, 2 every stream
  bool no_bound = false;       // fsk_fft_bound found no tau (p.tau = +inf): mode 1 runs as mode 2
  // the time-split F1 (fsk_kernels.hip FS1-FS3): designed
  // with the plan; used for calls of at most kFskSplitMaxStreams streams
  // (amr_fsk_plan_set_layout overrides); its forward outputs and peaks in
  // split_y1 / split_peak, allocated on the first split call (<= 1024 streams)
  bool split_ok = false;
  int64_t split_w = 0;
  double split_kappa = 0.0, split_hl1 = 0.0, split_tau = 0.0;
  int split_mode = AMR_FSK_LAYOUT_AUTO;
  bool split_now = false;      // this call runs the split F1 (z approximate: no keep_z, E1 re-runs F1)
  bool last_split = false;
  int64_t split_L = 0;
  int64_t split_reserved = 0;  // what amr_fsk_plan_bytes_estimate counts for them (<= 1024 streams)
  // FS0's convolution start states: tables [2][w][6] + [2][w + 1][6] (host
  // copy made with the design), on the device with the zs states in split_cz
  std::vector<double> split_tab_host;
  // the split F1's STRICT mode (round 6; split_strict.h strict_design_bp per
  // tone, fsk_kernels.hip FS0-FS2 with ST, KF1-KF2, FS3): designed on the
  // first strict call; its tables, per-stream maxima and scratch in
  // strict_tab / strict_bnd / strict_sc
  int strict_mode = -1;        // amr_fsk_plan_set_split_strict: 1 on, 0 off, -1 the default
  bool strict_designed = false, strict_ok = false, last_strict = false;
  StrictDesign sdes[2];
};

namespace {

// the byte totals amr_fsk_plan_scratch_bytes / amr_fsk_plan_resident_bytes report, from the buffers
int64_t fsk_scratch_bytes(const amr_fsk_plan* pl) {      // what amr_fsk_plan_create allocated, and dd once it exists
  const amr_fsk_plan::Mem& m = pl->mem;
  return m.z.bytes() + m.u.bytes() + m.v.bytes() + m.dd.bytes() + m.cmp.bytes() + m.words.bytes() + m.xflags.bytes() +
         m.amb.bytes() + m.xlist.bytes() + m.xslots.bytes() + m.xbits.bytes() + m.xpool.bytes() + m.xL.bytes() +
         pl->fft.mem.s1.bytes() + pl->fft.mem.s2.bytes();
}
int64_t fsk_split_bytes(const amr_fsk_plan* pl) {
  return pl->mem.split_y1.bytes() + pl->mem.split_peak.bytes() + pl->mem.split_cz.bytes();
}
int64_t fsk_strict_bytes(const amr_fsk_plan* pl) {
  return pl->mem.strict_tab.bytes() + pl->mem.strict_bnd.bytes() + pl->mem.strict_sc.bytes();
}
int64_t fsk_out_staging_bytes(const amr_fsk_plan* pl) {
  return pl->mem.d_out.bytes() + pl->mem.d_len.bytes() + pl->mem.d_sync.bytes() + pl->mem.d_edge.bytes();
}

// set device, drain the stream, drop the gather gate; then the buffers; then events and the stream
void fsk_plan_free(amr_fsk_plan* pl) {
  if (!pl) return;
  (void)hipSetDevice(pl->device);
  if (pl->stream) (void)hipStreamSynchronize(pl->stream);
  gate_free(pl->gate);
  if (pl->xcount_host) (void)hipHostFree(pl->xcount_host);
  pl->mem = amr_fsk_plan::Mem{};                 // frees every device buffer
  pl->fft.mem = FftPlan::Mem{};
  core_destroy_events(*pl);
  if (pl->stream) (void)hipStreamDestroy(pl->stream);
  delete pl;
}

// this call keeps z whole through F2 (dd allocated: see amr_fsk_plan::dd;
// a split call's z is not scipy's, so the exact path re-runs F1 instead)
bool keeps_z(const amr_fsk_plan* pl) { return pl->keep_z && pl->mem.dd && !pl->split_now; }

// F1 over the B streams of x -> z (and, with the exact path on, each
// stream's ambiguity scale; the flag words cleared).  Caller holds mu.
constexpr int64_t kFskSplitMaxStreams = 1024;   // AUTO: calls of at most this many streams split

// The split F1's launch geometry: L outputs per chunk (at least
// kFskSplitMinL and w / 4, so warm-ups are at most 4x the useful work, and
// long enough to keep a launch within kFskSplitLanes lanes)
constexpr int64_t kFskSplitMinL = 64;
constexpr int64_t kFskSplitLanes = 65536;
// with FS0's convolution start states (AMR_FSK_SPLIT_CONV=0: the warm-ups):
// chunks of kFskSplitConvMinL..MaxL outputs, about kFskSplitConvChunks (chunk,
// tone) waves per call -- the PSK split's rule (api.cpp kSplitConv*)
constexpr int64_t kFskSplitConvMinL = 128;
constexpr int64_t kFskSplitConvMaxL = 1024;
constexpr int64_t kFskSplitConvChunks = 3072;
// the split F1's strict margin by default (AMR_FSK_SPLIT_STRICT=0 / 1 overrides)
constexpr int kFskStrictDefault = 1;
bool fsk_split_conv_on(const amr_fsk_plan* pl) {
  static const bool env = env_not_off("AMR_FSK_SPLIT_CONV");
  return env && pl->split_ok && !pl->split_tab_host.empty();
}
// STRICT: AMR_FSK_SPLIT_STRICT=0 / 1 sets the default, amr_fsk_plan_set_split_strict
// a plan's; the bound covers the convolution starts only
bool fsk_split_strict_on(const amr_fsk_plan* pl) {
  static const int env = env_tri("AMR_FSK_SPLIT_STRICT");   // unset: kFskStrictDefault
  const bool want = pl->strict_mode >= 0 ? pl->strict_mode == 1 : (env < 0 ? kFskStrictDefault : env) == 1;
  return want && fsk_split_conv_on(pl);
}
FskSplit fsk_split_params(amr_fsk_plan* pl, int64_t B, int64_t L) {
  FskSplit sp{};
  const int64_t m1 = pl->p.n + 2 * (int64_t)pl->p.pad;
  sp.conv = fsk_split_conv_on(pl) ? 1 : 0;
  const int64_t lanes = (2 * B * m1 + kFskSplitLanes - 1) / kFskSplitLanes;
  if (L > 0) sp.L = L;
  else if (sp.conv)
    sp.L = std::max(lanes, std::min(kFskSplitConvMaxL, std::max(kFskSplitConvMinL,
                                                                  (2 * B * m1 + kFskSplitConvChunks - 1) /
                                                                      kFskSplitConvChunks)));
  else sp.L = std::max({kFskSplitMinL, pl->split_w / 4, lanes});
  sp.w = pl->split_w;
  if (L <= 0 && sp.conv && fsk_split_strict_on(pl) && pl->strict_ok)   // chunks on block boundaries
    sp.L = (sp.L + kStrictBlk - 1) / kStrictBlk * kStrictBlk;
  sp.c = (m1 + sp.L - 1) / sp.L;
  sp.tau = pl->split_tau;
  sp.y1 = pl->mem.split_y1.as<double>();
  sp.peak = pl->mem.split_peak.as<unsigned long long>();
  pl->split_L = sp.L;
  return sp;
}

// STRICT: the per-tone designs from FS0's tables (host arithmetic, once) and
// their device copy: per tone split_strict.h strict_bp_append's tables
int fsk_strict_prepare(amr_fsk_plan* pl) {
  if (pl->strict_designed) return AMR_OK;
  pl->strict_designed = true;
  pl->strict_ok = false;
  if (!pl->split_ok || pl->split_tab_host.empty()) return AMR_OK;
  const int nt = pl->p.nt;
  const int64_t w = pl->split_w;
  bool ok = true;
  for (int t = 0; t < 2 && ok; ++t) {
    const Iir fi = make_iir(pl->f.b[t], pl->f.a[t], pl->f.zi[t], nt);
    StrictDesign& d = pl->sdes[t];
    ok = strict_design_bp(fi, pl->split_tab_host.data() + (size_t)t * w * 6,
                          pl->split_tab_host.data() + (size_t)(2 * w + t * (w + 1)) * 6, w, d,
                          strict_detail::responses(fi)) &&
         d.g1x * (d.kx + 2.0 * d.ky) < 0.125;
    d.ok = ok;
  }
  if (!ok) return AMR_OK;
  std::vector<double> tab;
  for (int t = 0; t < 2; ++t) strict_bp_append(pl->sdes[t], tab);
  HIP_TRY(pl->mem.strict_tab.reserve((int64_t)tab.size() * 8, nullptr));
  HIP_TRY(hipMemcpy(pl->mem.strict_tab.get(), tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  pl->strict_ok = true;
  return AMR_OK;
}
// STRICT: this call's scratch and maxima for B streams, and sp's strict fields
int ensure_fsk_strict(amr_fsk_plan* pl, FskSplit& sp, int64_t B) {
  // (a diagnostic's forced chunk off block boundaries runs without it)
  if (!sp.conv || !fsk_split_strict_on(pl) || !pl->strict_ok || sp.L % kStrictBlk != 0) return AMR_OK;
  const int64_t m1 = pl->p.n + 2 * (int64_t)pl->p.pad;
  sp.rows.nb1 = (m1 + kStrictBlk - 1) / kStrictBlk;
  sp.rows.c = sp.c;
  sp.rows.sstride = strict_off_end(sp.rows);
  HIP_TRY(pl->mem.strict_sc.reserve(B * 2 * sp.rows.sstride * 8, pl->stream));
  HIP_TRY(pl->mem.strict_bnd.reserve(B * 2 * 64, pl->stream));
  sp.strict = 1;
  sp.hl1 = pl->split_hl1;
  sp.rows.sc = pl->mem.strict_sc.as<double>();
  sp.bnd = pl->mem.strict_bnd.as<unsigned long long>();
  sp.sb[0] = strict_bp_view(pl->sdes[0], pl->mem.strict_tab.as<double>());
  sp.sb[1] = strict_bp_view(pl->sdes[1], pl->mem.strict_tab.as<double>() + strict_bp_doubles(pl->sdes[0]));
  return AMR_OK;
}
// the tables and this call's zs in split_cz (grown as needed), then sp's pointers into it
int ensure_split_conv(amr_fsk_plan* pl, FskSplit& sp, int64_t B) {
  if (!sp.conv) return AMR_OK;
  const int64_t tab = (int64_t)pl->split_tab_host.size() * 8;
  const int64_t need = tab + B * 2 * sp.c * 6 * 8;
  DevBuf& cz = pl->mem.split_cz;
  if (cz.bytes() < need || !cz) {
    HIP_TRY(cz.reserve(need, pl->stream));
    HIP_TRY(hipMemcpy(cz.get(), pl->split_tab_host.data(), (size_t)tab, hipMemcpyHostToDevice));
  }
  sp.ktab = cz.as<double>();
  sp.z0tab = cz.as<double>() + 2 * sp.w * 6;
  sp.zs = cz.as<double>() + tab / 8;
  return AMR_OK;
}
// the forward outputs and peaks of B streams
int ensure_split_buffers(amr_fsk_plan* pl, int64_t B) {
  const int64_t m1 = pl->p.n + 2 * (int64_t)pl->p.pad;
  HIP_TRY(pl->mem.split_y1.reserve(B * 2 * m1 * 8, pl->stream));
  HIP_TRY(pl->mem.split_peak.reserve(B * 8, pl->stream));
  return AMR_OK;
}
// does this call run the split F1?  Only with the exact path on (it is what
// makes the split's decisions exact)
bool use_split(const amr_fsk_plan* pl, int64_t B) {
  static const bool env_off = !env_not_off("AMR_FSK_SPLIT");
  if (!pl->split_ok || !pl->exact_on || pl->exact_mode == 0 || pl->p.n_bits == 0 || B < 1 || B > 65535) return false;
  if (pl->split_mode == AMR_FSK_LAYOUT_SPLIT) return true;
  return pl->split_mode == AMR_FSK_LAYOUT_AUTO && !env_off && B <= kFskSplitMaxStreams;
}

int run_fsk_f1(amr_fsk_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride, bool exact) {
  FskParams p = pl->p;
  if (!(exact && pl->exact_on && pl->exact_mode != 0)) p.amb = nullptr;
  p.force_exact = pl->exact_mode == 2 || pl->no_bound ? 1 : 0;
  if (pl->split_now) {
    if (int rc = ensure_split_buffers(pl, B)) return rc;
    if (fsk_split_strict_on(pl))
      if (int rc = fsk_strict_prepare(pl)) return rc;
    FskSplit sp = fsk_split_params(pl, B, 0);
    if (int rc = ensure_split_conv(pl, sp, B)) return rc;
    if (int rc = ensure_fsk_strict(pl, sp, B)) return rc;
    pl->last_strict = sp.strict != 0;
    HIP_TRY(launch_fsk_split(dtype, d_x, x_stride, B, pl->mem.z.as<double2>(), p, pl->f, sp, pl->stream));
    return AMR_OK;
  }
  HIP_TRY(launch_fsk_bandpass(dtype, d_x, x_stride, B, pl->mem.u.as<double>(), pl->mem.z.as<double2>(), p, pl->f,
                              pl->stream));
  return AMR_OK;
}

// F2 over the B streams of z: the Hilbert filter, whose last pass forms both
// envelopes, packs the compare bits and flags the streams with a compare
// inside the margin (or, env_out on a natural-layout plan, stores the
// envelopes themselves in hilbert_out(u, v)).
int run_fsk_f2(amr_fsk_plan* pl, int64_t B, bool env_out) {
  FftEpi env{};
  env.mode = env_out ? kEnvOut : kEnvelope;
  env.z = pl->mem.z.as<double2>();
  env.bits = pl->mem.cmp.as<uint8_t>();
  env.bits_stride = pl->p.bits_stride;
  if (!env_out && pl->exact_on && pl->exact_mode != 0) {
    env.amb = pl->mem.amb.as<double>();
    env.xflags = pl->mem.xflags.as<uint32_t>();
  }
  if (pl->p.lc.on) {
    if (env_out) return fail(AMR_E_INVALID, "live-column plan: envelopes go through a natural-layout plan");
    const LiveCols& lc = pl->p.lc;
    HIP_TRY(launch_fft_hilbert_live(pl->mem.z.as<double2>(), pl->mem.u.as<double2>(),
                                    keeps_z(pl) ? pl->mem.dd.as<double2>() : nullptr, pl->fft.d, B, lc, env,
                                    pl->stream));
  } else {
    HIP_TRY(fft_hilbert(pl->fft, pl->mem.z.as<double2>(), pl->mem.u.as<double2>(), pl->mem.v.as<double2>(), B, env,
                        pl->stream));
  }
  return AMR_OK;
}

// The exact path over F2's flagged streams: with keep_z straight from z (F2
// left it whole), otherwise F1 again over their input x (still resident).
int run_fsk_exact(amr_fsk_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride) {
  if (!pl->exact_on || pl->exact_mode == 0) return AMR_OK;
  FskExact X{};
  X.flags = pl->mem.xflags.as<uint32_t>();
  X.list = pl->mem.xlist.as<int32_t>();
  X.count = pl->mem.xlist.as<int32_t>() + pl->max_streams;
  X.rows = reinterpret_cast<double*>(pl->mem.z.as<double2>());
  X.live = keeps_z(pl) ? 1 : 0;
  X.lc = pl->p.lc;
  X.slots = pl->mem.xslots.as<double>();
  X.slot_doubles = pl->slot_doubles;
  X.n_slots = pl->n_slots;
  X.L = pl->mem.xL.as<PfLen>();
  X.pool = pl->mem.xpool.as<double>();
  X.fct = (double)(1.0L / (long double)pl->p.n);
  X.xbits = pl->mem.xbits.as<uint8_t>();
  X.fuse = (int)pf_fuse_on();
  X.lean = X.fuse && pl->x_lean;
  X.count_host = pl->xcount_dev;
  if (pl->xcount_host) {
    pl->hint_hist[pl->hint_pos] = *reinterpret_cast<volatile int32_t*>(pl->xcount_host);
    pl->hint_pos = (pl->hint_pos + 1) % amr_fsk_plan::kHintDepth;
    X.count_hint = *std::max_element(pl->hint_hist, pl->hint_hist + amr_fsk_plan::kHintDepth);
  } else {
    X.count_hint = B;
  }
  hipStream_t st = pl->stream;
  return timed(*pl, AMR_TF_EXACT, [&]() -> int {
    pl->ran_exact = true;
    HIP_TRY(launch_fsk_exact_list(B, X, st));
    if (pl->count_sync) {
      int32_t c = 0;
      HIP_TRY(hipMemcpyAsync(&c, X.count, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (c == 0) {                            // nothing flagged: F3 takes every stream's fast-path bits
        pl->ran_exact = false;
        *pl->xcount_host = 0;
        return AMR_OK;
      }
      X.count_hint = c;
    }
    if (!X.live) {
      // E1: F1 again over the flagged streams only (list mode), natural z layout
      FskParams p1 = pl->p;
      p1.amb = nullptr;
      p1.lc = LiveCols{};
      p1.xlist = X.list;
      p1.xcount = X.count;
      HIP_TRY(launch_fsk_bandpass(dtype, d_x, x_stride, B, pl->mem.u.as<double>(), pl->mem.z.as<double2>(), p1, pl->f, st));
    }
    HIP_TRY(launch_fsk_exact_env(B, pl->p, X, st));
    return AMR_OK;
  });
}

// F1, F2 (and the exact path) on a device-resident batch: x -> cmp (or the envelopes).  Caller holds mu.
int run_fsk_front(amr_fsk_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride, bool env_out) {
  if (env_out) pl->split_now = false;        // the envelopes themselves: scipy's F1
  if (int rc = timed(*pl, AMR_TF_BANDPASS, [&] { return run_fsk_f1(pl, d_x, dtype, B, x_stride, !env_out); })) return rc;
  // one timing slot for the whole Hilbert filter (column, middle and final passes)
  if (int rc = timed(*pl, AMR_TF_HILBERT, [&] { return run_fsk_f2(pl, B, env_out); })) return rc;
  if (env_out) return AMR_OK;
  return run_fsk_exact(pl, d_x, dtype, B, x_stride);
}

// no decision window (sps // 4 == 0): empty bit string -> b''   (modem.py:320-323)
int fsk_empty_outputs(amr_fsk_plan* pl, int64_t B, int64_t* d_len, int64_t* d_sync) {
  HIP_TRY(gate_wait(pl->gate, pl->stream));
  HIP_TRY(hipMemsetAsync(d_len, 0, (size_t)B * 8, pl->stream));
  HIP_TRY(hipMemsetAsync(d_sync, 0xFF, (size_t)B * 8, pl->stream));
  return AMR_OK;
}

// F3: compare bits -> decided words -> sync + pack.  Caller holds mu.
int run_fsk_back(amr_fsk_plan* pl, const DemodIo& io) {
  const int64_t B = io.B;
  hipStream_t st = pl->stream;
  // a flagged stream's bits come from xbits only when this call's E0-E3 wrote
  // them (exact mode 0 leaves the flag words of an earlier call untouched)
  FskParams p = pl->p;
  if (!pl->ran_exact) p.xflags = nullptr;
  return timed(*pl, AMR_TF_DECIDE, [&]() -> int {
    HIP_TRY(launch_fsk_decide(pl->mem.cmp.as<uint8_t>(), pl->mem.words.as<uint32_t>(), B, p, st));
    HIP_TRY(gate_wait(pl->gate, st));             // the outputs: after any gather still reading them
    HIP_TRY(launch_sync_pack(pl->mem.words.as<uint32_t>(), pl->p.n_words, pl->p.n_bits, B, io.out, io.out_stride, io.len,
                             io.sync, st));
    return AMR_OK;
  });
}

// the call's odd-extension table (odd_ext.h) in the plan's FskParams for the
// launches of one call (F1, its split form and the exact path's F1 re-run
// copy pl->p); cleared when the call returns.  Caller holds mu.
struct EdgeScope {
  FskParams& p;
  EdgeScope(FskParams& q, const double* e) : p(q) { p.edge = e; }
  ~EdgeScope() { p.edge = nullptr; }
};

// d_edge: [B][2 pad] for a raw-integer capture (include/amr.h
// amr_fsk_demod_host_edges), or null
int run_fsk(amr_fsk_plan* pl, const DemodIo& io, const double* d_edge = nullptr) {
  if (int rc = check_demod_args(pl, io, ArgOrder::device)) return rc;
  EdgeScope edge_scope(pl->p, d_edge);
  core_clear_used(*pl);
  pl->ran_exact = false;
  pl->split_now = use_split(pl, io.B);
  pl->last_split = pl->split_now;
  if (io.B == 0) return AMR_OK;
  if (pl->p.n_bits == 0) return fsk_empty_outputs(pl, io.B, io.len, io.sync);
  return timed(*pl, AMR_TF_LAUNCH, [&]() -> int {
    if (int rc = run_fsk_front(pl, io.x, io.dtype, io.B, io.x_stride, false)) return rc;
    return run_fsk_back(pl, io);
  });
}

// Where the host entries stage the input (max_streams rows of up to 8 B per
// sample): dd with keep_z (the column pass overwrites it after F1 read it),
// else d_x, where it stays for the exact path's F1 re-run after F2.
int staging_buffer(amr_fsk_plan* pl, void** buf) {
  DevBuf& b = pl->keep_z ? pl->mem.dd : pl->mem.d_x;
  HIP_TRY(b.reserve(pl->keep_z ? pl->dd_bytes : pl->max_streams * pl->p.n * 8, pl->stream));
  *buf = b.get();
  return AMR_OK;
}
int stage_input(amr_fsk_plan* pl, const void* x, int dtype, int64_t B, int64_t x_stride, void** staged,
                Copy how = Copy::sync) {
  const int64_t es = dtype_size(dtype);
  const int64_t n = pl->p.n;
  if (int rc = staging_buffer(pl, staged)) return rc;
  return upload_batch(how, *staged, x, n * es, x_stride * es, B, pl->stream);
}

// the host entries' output staging and the edge table (amr_fsk_demod_host_edges)
int ensure_out_staging(amr_fsk_plan* pl) {
  const int64_t ms = pl->max_streams;
  amr_fsk_plan::Mem& m = pl->mem;
  // (the inner parentheses keep the braces' commas from splitting the macro's argument)
  HIP_TRY((reserve_all({{m.d_out, ms * pl->out_cap}, {m.d_len, ms * 8}, {m.d_sync, ms * 8},
                        {m.d_edge, ms * 2 * (int64_t)pl->p.pad * 8}}, pl->stream)));
  return AMR_OK;
}

// Live-column layout for this plan (amr_internal.h LiveCols), or off: needs a
// two-pass length n = n1 * n2 with n1 a multiple of sps and a decision window.
// Every index the kernels use is checked here on the host (the float
// divisions of lc_div, the [L | D] offsets as a bijection onto [0, n)).
LiveCols plan_live_cols(const FftShape& f, const FskParams& p) {
  LiveCols lc{};
  static const bool off = !env_not_off("AMR_FSK_LIVE");
  const int64_t q = p.sps / 4, half = p.sps / 2;
  if (off || f.bluestein || f.six || p.n_bits == 0 || q < 1) return lc;
  const int n1 = f.n1, n2 = f.n2;
  if (p.sps > n1 || n1 % p.sps != 0 || (int64_t)n1 * n2 != p.n) return lc;
  lc.n1 = n1;
  lc.n2 = n2;
  lc.sps = (int)p.sps;
  lc.w0 = (int)(half - q);
  lc.nw = (int)(2 * q);
  lc.nl = n1 / lc.sps * lc.nw;
  lc.nd = n1 - lc.nl;
  lc.inv_n1 = 1.0f / (float)n1;
  lc.inv_sps = 1.0f / (float)lc.sps;
  lc.inv_nw = 1.0f / (float)lc.nw;
  lc.inv_ndp = 1.0f / (float)(lc.sps - lc.nw);
  if (lc.nd < 1) return LiveCols{};
  for (int j1 = 0; j1 < n1; ++j1) {
    bool live = false;
    const int pos = lc_col_pos(lc, j1, live);
    const int v = j1 % lc.sps;
    if (live != (v >= lc.w0 && v < lc.w0 + lc.nw)) return LiveCols{};
    if ((live ? lc_live_col(lc, pos) : lc_dead_col(lc, pos)) != j1) return LiveCols{};
  }
  std::vector<uint8_t> seen((size_t)p.n, 0);
  for (int64_t i = 0; i < p.n; ++i) {
    const int64_t o = lc_zoff(lc, (int)i);
    if (o < 0 || o >= p.n || seen[(size_t)o]) return LiveCols{};
    seen[(size_t)o] = 1;
  }
  lc.on = 1;
  return lc;
}

// Sizes of an FSK plan's device buffers from its shape alone (no device
// work): amr_fsk_plan_create allocates exactly these; amr_fsk_plan_bytes_estimate
// sums them for the drop-in plan cache before it creates a plan.
struct FskGeom {
  FskParams p{};
  FftShape sh;
  int64_t z = 0, u = 0, v = 0, dd = 0, cmp = 0, words = 0, six = 0, staging = 0, out = 0, out_cap = 0;
  int64_t split = 0;       // the split F1's buffers for up to kFskSplitMaxStreams streams (allocated on use)
  bool keep_z = false;
  bool dd_eager = false;   // AMR_FSK_KEEPZ=1: dd at creation (else on the first host entry)
  // the exact path: flags, scales, list, slots, exact bits, pocketfft tables
  bool exact = false;
  int n_slots = 0;
  int64_t slot_doubles = 0, xflags = 0, amb = 0, xlist = 0, xslots = 0, xbits = 0, xpool = 0, xplan = 0;
  int64_t total() const {
    return z + u + v + dd + cmp + words + six + staging + out + xflags + amb + xlist + xslots + xbits + xpool + xplan +
           split;
  }
};
bool fsk_geometry(int64_t n, int64_t sps, int nt, int64_t max_streams, FskGeom& g) {
  FskParams& p = g.p;
  p.n = n;
  p.sps = sps;
  p.nt = nt;
  p.pad = 3 * nt;
  const int64_t q = sps / 4, half = sps / 2;
  p.n_bits = (q > 0 && n > half) ? (n - half + sps - 1) / sps : 0;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
  g.out_cap = p.n_bits / 8 + 1;
  if (!fft_shape(n, g.sh)) return false;
  const int64_t M = g.sh.M;
  const bool plain = g.sh.bluestein || g.sh.six;   // epilogue in natural order (post kernel)
  p.rn1 = plain ? n : g.sh.n1;
  p.rn2 = plain ? 1 : g.sh.n2;
  p.lc = plan_live_cols(g.sh, p);
  p.bits_stride = p.lc.on ? (int64_t)((p.lc.nl + 7) >> 3) * p.rn2 : fft_bits_stride(p.rn1, p.rn2);
  p.inv_rn1 = 1.0f / (float)p.rn1;
  const int64_t s1_bytes = fsk_bandpass_scratch_bytes(max_streams, n, p.pad);
  if (p.lc.on) {
    // C: the live columns' transform; before the column pass it holds F1's checkpoints
    g.u = std::max(max_streams * (int64_t)p.lc.nl * p.lc.n2 * 16, s1_bytes);
  } else {
    g.u = std::max(max_streams * M * 16, s1_bytes);
    g.v = max_streams * M * 16;
  }
  g.staging = max_streams * n * 8;                   // d_x, allocated on the first host call
  // z; after F2, the exact path's rows ([ordinal][n] (f_mark, f_space))
  g.z = max_streams * n * 16;
  g.cmp = max_streams * p.bits_stride;
  g.words = max_streams * p.n_words * 4;
  g.six = g.sh.six ? 2 * max_streams * M * 16 : 0;
  g.out = max_streams * (g.out_cap + 16 + 2 * (int64_t)p.pad * 8);   // host-API output staging + edge table
  // (+ FS0's tables, w <= n / 4, and start states at L >= kFskSplitConvMinL)
  // (+ the strict margin's per-tone scratch: 5 blocks rows of ceil(m1 / 16) and
  // two chunk rows, the maxima, and the tables -- W, K12, HS, TZ <= 4 w / 16 + 64 each)
  const int64_t m1g = n + 2 * (int64_t)p.pad;
  const int64_t strict_row = 5 * ((m1g + kStrictBlk - 1) / kStrictBlk) + 2 * (m1g / kFskSplitConvMinL + 2);
  g.split = std::min<int64_t>(max_streams, kFskSplitMaxStreams) *
                (2 * m1g * 8 + 8 + 96 * (m1g / kFskSplitConvMinL + 2) + 2 * (strict_row * 8 + 64)) +
            2 * (2 * (n / 4) + 1) * 48 + 2 * (2 * (n / 4) + 1 + 4 * (2 * (n / 4) / 16 + 64) + 64) * 8;
  // the exact path (AMR_FSK_EXACT=0: off), at every length with decisions to make
  static const bool exact_env = env_not_off("AMR_FSK_EXACT");
  g.exact = exact_env && p.n_bits > 0;
  if (g.exact) {
    g.slot_doubles = pf_even(n) + pf_scratch_doubles_n(n);   // the row, then its transforms' scratch
    // one persistent workgroup per slot: up to 2 per stream and 512 (2 per
    // CU; the launch takes no more than are resident at once, E2's register
    // budget allows one per CU), within 2 GiB of slots
    g.n_slots = (int)std::max<int64_t>(
        1, std::min<int64_t>({2 * max_streams, 512, ((int64_t)1 << 31) / (g.slot_doubles * 8)}));
    g.xflags = (max_streams + 31) / 32 * 4;
    g.amb = max_streams * 8;
    g.xlist = (max_streams + 1) * 4;
    g.xslots = (int64_t)g.n_slots * g.slot_doubles * 8;
    g.xbits = max_streams * p.bits_stride;
    g.xpool = pf_pool_doubles_bound(n) * 8;
    g.xplan = (int64_t)sizeof(PfLen);
    // live layout: keep all of z through F2 (the exact path then needs no F1
    // re-run); the dead tiles' transform and the staged input go to dd
    // (AMR_FSK_KEEPZ=0, an A/B switch: dead tiles in place, the F1 re-run)
    static const bool keepz_env = env_not_off("AMR_FSK_KEEPZ");
    static const bool eager_env = env_on("AMR_FSK_KEEPZ");
    g.keep_z = keepz_env && p.lc.on && (int64_t)p.lc.nd * p.lc.n2 * 2 >= n;
    if (g.keep_z) {
      g.dd = max_streams * (int64_t)p.lc.nd * p.lc.n2 * 16;   // counted: a host entry allocates it
      g.dd_eager = eager_env;
      g.staging = 0;
    }
  }
  return true;
}

// The split F1's design (the PSK layout's rule, iir_design.h):
// per tone, a chunk's outputs differ from scipy's by (1) the zero start,
// decayed after w samples to tail(w) * zmax * 3 peak (the odd extension
// triples the input peak) and carried through the backward pass (its L1 gain
// h1) -- w is chosen to bring that below u G / 16 -- and (2) a different
// rounding trajectory, G = g1 (1 + h1): the forward pass's rounding (noise
// gain g1) filtered backward, plus the backward pass's own.  kappa = 64.25 u
// G over the tones (measured >= 30x above the worst error,
// tests/test_split_margin.py); an envelope then moves by at most kappa *
// ||ifft(h)||_1 * peak|ext x|, the margin F2 adds for split calls.  Refused
// when a warm-up exceeds n / 4 or the margin would pass 2^-24 of the peak.
constexpr double kFskSplitSafety = 64.0;
// both tones' response sums (iir_design.h iir_gains): walked once, shared by
// the split design and F2's FFT bound
void fsk_tone_gains(const FskIir& f, int nt, IirGains g[2]) {
  for (int t = 0; t < 2; ++t) {
    g[t] = iir_gains(make_iir(f.b[t], f.a[t], nullptr, nt));
    if (!g[t].ok) return;        // no design and no bound without both
  }
}
bool fsk_split_design(const IirGains g[2], int nt, int64_t n, int64_t* w_out, double* kappa_out, double* hl1_out) {
  if (nt != 7 || n < 64 || !g[0].ok || !g[1].ok) return false;
  const double u = 0x1p-53;
  double G = 0.0;
  for (int t = 0; t < 2; ++t) G = std::max(G, g[t].g1 * (1.0 + g[t].h1));
  const double tol = 0x1p-4 * u * G;
  int64_t w = 0;
  for (int t = 0; t < 2; ++t) {
    const int64_t wt = warmup_for(g[t], g[t].zmax * 3.0 * g[t].h1, tol);
    if (wt < 0) return false;
    w = std::max(w, wt);
  }
  const double kappa = (kFskSplitSafety + 0.25) * u * G;
  const double hl1 = hilbert_l1(n) * (1.0 + 0x1p-20);
  if (w > n / 4 || !(kappa * hl1 <= 0x1p-16)) return false;
  *w_out = w;
  *kappa_out = kappa;
  *hl1_out = hl1;
  return true;
}

// F2's margin scale tau from a standard FFT rounding bound (round 6, DESIGN.md
// §2 item 6).  F2 keeps a compare only when |env_mark - env_space| > 2 tau
// peak|ext x|; the fast path's and pocketfft's envelopes each differ from
// |hilbert(z)| in exact arithmetic by at most (4 eps + 4u) ||z||_2 per tone,
// eps the transform's relative 2-norm error:
//   direct (FFTPACK-style / two-pass / six-step) length M, widest radix p:
//     eps = L eta / (1 - L eta), L = ceil(log2 M), eta = max(8.5u, sqrt(p)
//     gamma_{p+4} / log2 p) + 2u (a radix-p pass's 2-norm error per binary
//     level -- Higham's radix-2 eta = mu + gamma_4 (sqrt2 + mu) generalised --
//     plus twiddles within 2u);
//   Bluestein (n, M): (Bmax / sqrt n) (2 eps_M + 2 gc) + sqrt(2n - 1) eps_M +
//     gc, gc = sqrt2 gamma_2 + 2u (a complex product with a rounded chirp):
//     the chirp product, FFT_M, the product with the kernel's spectrum (whose
//     own FFT-computed table is off by <= eps_M ||B||_2 = eps_M sqrt(M (2n -
//     1)) -- the sqrt(2n - 1) term), IFFT_M, the chirp product.  Bmax =
//     max |FFT_M(kernel)| <= sqrt(n) (6 + 2 ln n): the chirp exp(i pi m^2 / n)
//     is periodic (n or 2n) with Fourier coefficients of modulus 1 / sqrt(n)
//     (a quadratic Gauss sum), so the windowed kernel's spectrum is a sum of
//     Dirichlet kernels D_{2n-1}, whose values on a grid sum to <= 2 (2n - 1)
//     + P (ln(P / 2) + 1) (measured max |B| = 2.0-2.2 sqrt(n));
// and ||z||_2 <= (G^2 sqrt(m1) + 2 G R + R^2) peak|ext x| per tone (G the
// band-pass's L1 gain, R the L2 norm of its zi-start transient: both
// filtfilt passes).  tau = max(2^-36, (4 eps_fast + 4 eps_ref + 8u) max
// ||z||_2 / peak): a compare F2 keeps cannot differ between the two paths.
// ~13 x 2^-36 at n = 96000 (the measured difference stays ~1e-15 of the
// peak, tests/test_gpu_fsk.py); the flag rate of real signals is unchanged.
struct FskFftBound {
  double tau = 0.0, eps_fast = 0.0, eps_ref = 0.0, zmax = 0.0;
  bool fast_blue = false, ref_blue = false;
  int64_t fast_M = 0, ref_M = 0;
};
int64_t lpf_of(int64_t n) {
  int64_t r = 1;
  for (int64_t q = 2; q * q <= n; ++q)
    while (n % q == 0) {
      r = q;
      n /= q;
    }
  return n > 1 ? std::max(r, n) : r;
}
bool fsk_fft_bound(const FskIir& f, const IirGains gains[2], int nt, int64_t n, int pad, FskFftBound& o) {
  if (!gains[0].ok || !gains[1].ok) return false;
  const double u = 0x1p-53;
  auto gam = [&](double k) { return k * u / (1.0 - k * u); };
  auto eta_of = [&](int64_t p) {
    const double r = (double)std::max<int64_t>(p, 2);
    return std::max(8.5 * u, std::sqrt(r) * gam(r + 4.0) / std::max(1.0, std::log2(r))) + 2.0 * u;
  };
  auto eps_direct = [&](int64_t M, int64_t p) {
    const double e = std::ceil(std::log2((double)std::max<int64_t>(M, 2))) * eta_of(p);
    return e / (1.0 - e);
  };
  const double gc = std::sqrt(2.0) * gam(2.0) + 2.0 * u;
  const double bq = 6.0 + 2.0 * std::log((double)n);   // Bmax / sqrt(n)
  auto eps_blue = [&](int64_t M) {
    const double em = eps_direct(M, lpf_of(M));
    return bq * (2.0 * em + 2.0 * gc) + std::sqrt(2.0 * (double)n - 1.0) * em + gc;
  };
  FftShape sh;
  if (!fft_shape(n, sh)) return false;
  bool rb = false;
  int64_t rn2 = n, rp = 1;
  pf_hilbert_shape(n, &rb, &rn2, &rp);
  o.fast_blue = sh.bluestein;
  o.fast_M = sh.M;
  o.ref_blue = rb;
  o.ref_M = rn2;
  o.eps_fast = sh.bluestein ? eps_blue(sh.M) : eps_direct(n, lpf_of(n));
  o.eps_ref = rb ? eps_blue(rn2) : eps_direct(n, rp);
  const double m1 = (double)(n + 2 * (int64_t)pad);
  double zb = 0.0;
  for (int t = 0; t < 2; ++t) {
    const Iir fi = make_iir(f.b[t], f.a[t], f.zi[t], nt);
    const IirGains& g = gains[t];
    const double R = zi_response_l2(fi);
    if (!(R >= 0.0)) return false;
    const double G = g.h1 * (1.0 + 0x1p-20);
    zb = std::max(zb, G * G * std::sqrt(m1) + 2.0 * G * R + R * R);
  }
  o.zmax = zb;
  const double tau = (4.0 * o.eps_fast + 4.0 * o.eps_ref + 8.0 * u) * zb * (1.0 + 0x1p-20);
  o.tau = std::max(kAmbTau, tau);
  return std::isfinite(o.tau);
}

}  // namespace

extern "C" {

int amr_fsk_fft_margin(int64_t n, const double* mb, const double* ma, const double* mzi, const double* sb,
                       const double* sa, const double* szi, int nt, double* out) {
  if (!mb || !ma || !mzi || !sb || !sa || !szi || !out || nt < 2 || nt > 8 || n <= 3 * nt)
    return fail(AMR_E_INVALID, "amr_fsk_fft_margin: bad argument");
  FskIir f{};
  for (int i = 0; i < nt; ++i) {
    f.b[0][i] = mb[i];
    f.a[0][i] = ma[i];
    f.b[1][i] = sb[i];
    f.a[1][i] = sa[i];
  }
  for (int i = 0; i < nt - 1; ++i) {
    f.zi[0][i] = mzi[i];
    f.zi[1][i] = szi[i];
  }
  FskFftBound o;
  IirGains g[2];
  fsk_tone_gains(f, nt, g);
  if (!fsk_fft_bound(f, g, nt, n, 3 * nt, o)) return fail(AMR_E_INVALID, "amr_fsk_fft_margin: no bound for these filters at n");
  out[0] = o.tau;
  out[1] = o.eps_fast;
  out[2] = o.eps_ref;
  out[3] = o.zmax;
  out[4] = o.fast_blue ? 1.0 : 0.0;
  out[5] = (double)o.fast_M;
  out[6] = o.ref_blue ? 1.0 : 0.0;
  out[7] = (double)o.ref_M;
  return AMR_OK;
}

int amr_fsk_plan_margin(amr_fsk_plan* plan, double* tau, double* tau_split) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (tau) *tau = plan->p.tau;
  if (tau_split) *tau_split = plan->split_tau;
  return AMR_OK;
}

int amr_fsk_split_design(int64_t n, const double* mb, const double* ma, const double* sb, const double* sa, int nt,
                         int64_t* warmup, double* kappa, double* hilbert_l1_out) {
  if (!mb || !ma || !sb || !sa || nt != 7) return fail(AMR_E_INVALID, "amr_fsk_split_design: bad argument");
  FskIir f{};
  for (int i = 0; i < nt; ++i) {
    f.b[0][i] = mb[i];
    f.a[0][i] = ma[i];
    f.b[1][i] = sb[i];
    f.a[1][i] = sa[i];
  }
  int64_t w = 0;
  double k = 0.0, h = 0.0;
  IirGains g[2];
  if (n >= 64) fsk_tone_gains(f, nt, g);
  if (!fsk_split_design(g, nt, n, &w, &k, &h)) return fail(AMR_E_INVALID, "no time-split design for these filters at n");
  if (warmup) *warmup = w;
  if (kappa) *kappa = k;
  if (hilbert_l1_out) *hilbert_l1_out = h;
  return AMR_OK;
}

int64_t amr_fsk_plan_bytes_estimate(int64_t n, int64_t sps, int ntaps, int64_t max_streams) {
  if (n < 1 || sps < 1 || ntaps < 1 || max_streams < 1)
    return fail(AMR_E_INVALID, "amr_fsk_plan_bytes_estimate: bad argument");
  FskGeom g;
  if (!fsk_geometry(n, sps, ntaps, max_streams, g)) return fail(AMR_E_INVALID, "no FFT plan for this length");
  return g.total();
}

int amr_fsk_plan_create(amr_fsk_plan** out, int device, int64_t n, int64_t sps, const double* mb, const double* ma,
                        const double* mzi, const double* sb, const double* sa, const double* szi, int nt,
                        int64_t max_streams) {
  if (!out || !mb || !ma || !mzi || !sb || !sa || !szi) return fail(AMR_E_INVALID, "amr_fsk_plan_create: NULL argument");
  *out = nullptr;
  if (sps < 1 || max_streams < 1) return fail(AMR_E_INVALID, "bad sps/max_streams");
  if (nt != 7) return fail(AMR_E_INVALID, "FSK band-pass must have 7 taps (butter(3, band))");
  if (ma[0] != 1.0 || sa[0] != 1.0) return fail(AMR_E_INVALID, "a[0] must be 1 (scipy butter form)");
  if (n <= 3 * nt)
    return fail(AMR_E_PADLEN, "The length of the input vector x must be greater than padlen, which is " +
                                  std::to_string(3 * nt) + ".");
  auto* pl = new amr_fsk_plan();
  pl->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete pl;
    return fail(AMR_E_NODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  }
  FskGeom geo;
  if (!fsk_geometry(n, sps, nt, max_streams, geo)) {
    delete pl;
    return fail(AMR_E_INVALID, "no FFT plan for length " + std::to_string(n));
  }
  FskParams& p = pl->p;
  p = geo.p;
  for (int i = 0; i < nt; ++i) {
    pl->f.b[0][i] = mb[i];
    pl->f.a[0][i] = ma[i];
    pl->f.b[1][i] = sb[i];
    pl->f.a[1][i] = sa[i];
  }
  for (int i = 0; i < nt - 1; ++i) {
    pl->f.zi[0][i] = mzi[i];
    pl->f.zi[1][i] = szi[i];
  }
  pl->max_streams = max_streams;
  pl->out_cap = geo.out_cap;
  e = hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    fsk_plan_free(pl);
    return fail(AMR_E_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  if (int rc = fft_plan_init(pl->fft, n, pl->stream, max_streams)) {
    fsk_plan_free(pl);
    return rc;
  }
  pl->staging_bytes = geo.staging;
  pl->dd_bytes = geo.dd;
  pl->split_reserved = geo.split;
  amr_fsk_plan::Mem& m = pl->mem;
  struct A { DevBuf& buf; int64_t bytes; };
  const A allocs[] = {
      {m.z, geo.z},         {m.u, geo.u},         {m.v, geo.v},         {m.dd, geo.dd_eager ? geo.dd : 0},
      {m.cmp, geo.cmp},     {m.words, geo.words}, {m.xflags, geo.xflags}, {m.amb, geo.amb},
      {m.xlist, geo.xlist}, {m.xslots, geo.xslots}, {m.xbits, geo.xbits}, {m.xpool, geo.xpool},
      {m.xL, geo.xplan},
  };
  for (const A& a : allocs) {
    if (a.bytes == 0) continue;
    e = a.buf.reserve(a.bytes, nullptr);
    if (e != hipSuccess) {
      fsk_plan_free(pl);
      return fail(AMR_E_NOMEM, "hipMalloc(" + std::to_string(a.bytes) + " B): " + hipGetErrorString(e));
    }
  }
  if (geo.exact) {
    // E2's grid hint (FskExact count_hint): none yet, so the full grid
    e = hipHostMalloc((void**)&pl->xcount_host, sizeof(int32_t), hipHostMallocMapped);
    if (e == hipSuccess) {
      *pl->xcount_host = (int32_t)max_streams;
      for (int32_t& h : pl->hint_hist) h = (int32_t)max_streams;
      e = hipHostGetDevicePointer((void**)&pl->xcount_dev, pl->xcount_host, 0);
    }
    if (e != hipSuccess) {
      fsk_plan_free(pl);
      return fail(AMR_E_NOMEM, std::string("hipHostMalloc (exact-path count hint): ") + hipGetErrorString(e));
    }
    // pocketfft's plans of length n: tables to the device, then the Bluestein
    // tables that need a device transform (into the envelope slots' scratch)
    std::vector<double> pool;
    PfLen L{};
    if (!pf_len_build(n, L, pool) || (int64_t)pool.size() > geo.xpool / 8 || geo.xslots / 8 < 4 * L.bl.n2) {
      fsk_plan_free(pl);
      return fail(AMR_E_INVALID, "exact path: pocketfft plan of length " + std::to_string(n));
    }
    e = hipMemcpy(pl->mem.xpool.as<double>(), pool.data(), pool.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(pl->mem.xL.as<PfLen>(), &L, sizeof(PfLen), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = pf_finish(L, m.xL.as<PfLen>(), m.xpool.as<double>(), m.xslots.as<double>(), pl->stream);
    if (e == hipSuccess) e = hipMemset(pl->mem.xflags.as<uint32_t>(), 0, (size_t)geo.xflags);
    if (e != hipSuccess) {
      fsk_plan_free(pl);
      return fail(AMR_E_HIP, std::string("exact path tables: ") + hipGetErrorString(e));
    }
    pl->exact_on = true;
    pl->x_lean = pf_hilbert_lean(L);
    // keep_z reads z in the [L | D] layout through the lean kernel only; a
    // live-layout length is 5-smooth, so pocketfft's plans are always lean
    pl->keep_z = geo.keep_z;
    if (pl->keep_z && !pl->x_lean) {
      fsk_plan_free(pl);
      return fail(AMR_E_INVALID, "exact path: live-layout length " + std::to_string(n) + " without a lean plan");
    }
    pl->p.amb = pl->mem.amb.as<double>();
    pl->p.xflags = pl->mem.xflags.as<uint32_t>();         // F3 reads a flagged stream's bits from xbits
    pl->p.xbits = pl->mem.xbits.as<uint8_t>();
    pl->n_slots = geo.n_slots;
    pl->slot_doubles = geo.slot_doubles;
  }
  {
    FskFftBound fb;
    IirGains g[2];
    fsk_tone_gains(pl->f, nt, g);
    if (fsk_fft_bound(pl->f, g, nt, n, p.pad, fb)) {
      p.tau = fb.tau;
    } else {
      // no bound (a band-pass whose responses outlast iir_design.h's walk, or
      // grow): no compare of F2's can be kept, so every stream of every call
      // goes through the exact path (run_fsk_f1 force_exact) -- the
      // reference decodes these captures, and so does the plan
      pl->no_bound = true;
      p.tau = std::numeric_limits<double>::infinity();
    }
    double kappa = 0.0, hl1 = 0.0;
    pl->split_ok = fsk_split_design(g, nt, n, &pl->split_w, &kappa, &hl1);
    pl->split_kappa = kappa;
    pl->split_hl1 = hl1;
    pl->split_tau = p.tau + kappa * hl1;
    if (pl->split_ok) {   // FS0's tables, per tone: K [w][6], then Z0 [w + 1][6]
      const int64_t w = pl->split_w;
      pl->split_tab_host.assign((size_t)(2 * w + 2 * (w + 1)) * 6, 0.0);
      for (int t = 0; t < 2; ++t) {
        const Iir fi = make_iir(pl->f.b[t], pl->f.a[t], pl->f.zi[t], nt);
        split_state_tables(fi, w, pl->split_tab_host.data() + (size_t)t * w * 6,
                           pl->split_tab_host.data() + (size_t)(2 * w + t * (w + 1)) * 6);
      }
    }
  }
  *out = pl;
  return AMR_OK;
}

int amr_fsk_plan_destroy(amr_fsk_plan* plan) {
  fsk_plan_free(plan);
  return AMR_OK;
}
int64_t amr_fsk_plan_out_capacity(const amr_fsk_plan* plan) { return plan ? plan->out_cap : -1; }
int64_t amr_fsk_plan_scratch_bytes(const amr_fsk_plan* plan) {
  if (!plan) return -1;
  // scratch + the host-API staging (allocated on the first amr_fsk_demod_host:
  // d_x, or dd on a plan that keeps z)
  return fsk_scratch_bytes(plan) + plan->staging_bytes + (plan->mem.dd ? 0 : plan->dd_bytes) +
         plan->max_streams * (plan->out_cap + 16 + 2 * (int64_t)plan->p.pad * 8) +
         // == fsk_geometry().total() (split calls <= 1024 streams)
         std::max(plan->split_reserved, fsk_split_bytes(plan) + fsk_strict_bytes(plan));
}
int64_t amr_fsk_plan_resident_bytes(const amr_fsk_plan* plan) {
  if (!plan) return -1;
  // what is allocated now: a plan that only ever ran the device entry holds
  // no staging (no d_x, no dd, no output staging)
  return fsk_scratch_bytes(plan) + plan->mem.d_x.bytes() + fsk_out_staging_bytes(plan) + fsk_split_bytes(plan) +
         fsk_strict_bytes(plan);
}
int64_t amr_fsk_plan_fft_length(const amr_fsk_plan* plan) { return plan ? plan->fft.M : -1; }
int amr_fsk_plan_live_columns(const amr_fsk_plan* plan) { return plan ? plan->p.lc.on : -1; }

int amr_fsk_plan_split_conv(amr_fsk_plan* plan) {
  if (!plan) return -1;
  std::lock_guard<std::mutex> lk(plan->mu);
  return fsk_split_conv_on(plan) ? 1 : 0;
}

int amr_fsk_plan_set_layout(amr_fsk_plan* plan, int layout) {
  if (!plan || layout < AMR_FSK_LAYOUT_AUTO || layout > AMR_FSK_LAYOUT_SPLIT)
    return fail(AMR_E_INVALID, "amr_fsk_plan_set_layout: bad argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  plan->split_mode = layout;
  return AMR_OK;
}

int amr_fsk_plan_split_info(amr_fsk_plan* plan, int* last_split, int64_t* warmup, int64_t* chunk, double* kappa,
                            double* tau) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  std::lock_guard<std::mutex> lk(plan->mu);   // run_fsk / fsk_split_params write these under it
  if (last_split) *last_split = plan->last_split ? 1 : 0;
  if (warmup) *warmup = plan->split_ok ? plan->split_w : -1;
  if (chunk) *chunk = plan->split_L;
  if (kappa) *kappa = plan->split_kappa;
  if (tau) *tau = plan->split_tau;
  return AMR_OK;
}

int amr_fsk_plan_set_split_strict(amr_fsk_plan* plan, int mode) {
  if (!plan || mode < -1 || mode > 1) return fail(AMR_E_INVALID, "amr_fsk_plan_set_split_strict: bad argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  plan->strict_mode = mode;
  return AMR_OK;
}

int amr_fsk_plan_split_strict(amr_fsk_plan* plan) {
  if (!plan) return -1;
  std::lock_guard<std::mutex> lk(plan->mu);
  return fsk_split_strict_on(plan) ? 1 : 0;
}

int amr_fsk_plan_last_strict(amr_fsk_plan* plan) {
  if (!plan) return -1;
  std::lock_guard<std::mutex> lk(plan->mu);
  return plan->last_strict ? 1 : 0;
}

int amr_fsk_split_strict_design(const double* b, const double* a, const double* zi, int nt, int64_t w, double* consts,
                                double* tabs) {
  if (!b || !a || !zi || !consts || nt < 2 || nt > kMaxTaps || w < 1)
    return fail(AMR_E_INVALID, "amr_fsk_split_strict_design: bad argument");
  const Iir f = make_iir(b, a, zi, nt);
  const int N = nt - 1;
  std::vector<double> tab((size_t)(2 * w + 1) * N);
  split_state_tables(f, w, tab.data(), tab.data() + (size_t)w * N);
  StrictDesign d;
  const bool ok = strict_design_bp(f, tab.data(), tab.data() + (size_t)w * N, w, d, strict_detail::responses(f)) &&
                  d.g1x * (d.kx + 2.0 * d.ky) < 0.125;
  // the PSK entry's layout (amr_psk_split_strict_design) without the low-pass
  const double v[32] = {d.g1x, d.gmax, d.hz, d.tk, d.zi_sum, d.zb, d.kx, d.ky, kStrictU2,
                        d.gam, 0.0, (double)w, 0.0, 0.0, (double)d.W.size(), (double)d.K12.size(),
                        (double)d.HS.size(), (double)d.GS.size(), (double)d.TZ.size(), (double)d.k12_off, d.w_tail,
                        d.k12_tail, d.hs_tail, d.tz_tail, 0.0, 0.0, ok ? 1.0 : 0.0, 0.0};
  for (int i = 0; i < 32; ++i) consts[i] = v[i];
  if (!ok) return fail(AMR_E_INVALID, "no strict bound for this filter");
  if (tabs) {
    double* o = tabs;
    for (const std::vector<double>* t : {&d.kabs, &d.z0abs, &d.W, &d.K12, &d.HS, &d.GS, &d.TZ}) {
      std::memcpy(o, t->data(), t->size() * 8);
      o += t->size();
    }
  }
  return AMR_OK;
}

int amr_fsk_split_bounds_host(amr_fsk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                              double* z_out, double* bnd_out, double* peak_out) {
  if (!plan || !x || !z_out || !bnd_out || !peak_out || B < 1)
    return fail(AMR_E_INVALID, "amr_fsk_split_bounds_host: bad argument");
  if (!dtype_size(dtype)) return fail(AMR_E_INVALID, "unknown dtype");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  if (!plan->split_ok || !fsk_split_conv_on(plan)) return fail(AMR_E_INVALID, "no convolution-start split F1 for this plan");
  if (plan->p.n_bits == 0) return fail(AMR_E_INVALID, "amr_fsk_split_bounds_host: this plan has no decision bits");
  if (B > plan->max_streams || B > 65535) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < plan->p.n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  const int saved = plan->strict_mode;
  plan->strict_mode = 1;
  int rc = fsk_strict_prepare(plan);
  if (!rc && !plan->strict_ok) rc = fail(AMR_E_INVALID, "no strict bound for this plan's filters");
  const int64_t n = plan->p.n;
  void* xs = nullptr;
  if (!rc) rc = stage_input(plan, x, dtype, B, x_stride, &xs);
  if (!rc) rc = ensure_split_buffers(plan, B);
  FskParams p = plan->p;
  p.lc = LiveCols{};                         // natural order for the caller
  p.amb = nullptr;
  FskSplit sp{};
  if (!rc) {
    sp = fsk_split_params(plan, B, 0);
    rc = ensure_split_conv(plan, sp, B);
  }
  if (!rc) rc = ensure_fsk_strict(plan, sp, B);
  if (!rc && !sp.strict) rc = fail(AMR_E_INVALID, "no strict bound for this call's chunk (not a multiple of 16)");
  plan->strict_mode = saved;
  if (rc) return rc;
  HIP_TRY(launch_fsk_split(dtype, xs, n, B, plan->mem.z.as<double2>(), p, plan->f, sp, plan->stream));
  HIP_TRY(hipMemcpyAsync(z_out, plan->mem.z.as<double2>(), (size_t)(B * n * 16), hipMemcpyDeviceToHost, plan->stream));
  std::vector<unsigned long long> hb((size_t)B * 16), hp((size_t)B);
  HIP_TRY(hipMemcpyAsync(hb.data(), sp.bnd, hb.size() * 8, hipMemcpyDeviceToHost, plan->stream));
  HIP_TRY(hipMemcpyAsync(hp.data(), sp.peak, hp.size() * 8, hipMemcpyDeviceToHost, plan->stream));
  HIP_TRY(hipStreamSynchronize(plan->stream));
  std::memcpy(bnd_out, hb.data(), hb.size() * 8);
  std::memcpy(peak_out, hp.data(), hp.size() * 8);
  return AMR_OK;
}

int amr_fsk_split_bandpass_host(amr_fsk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                                int64_t chunk, double* out) {
  if (!plan || (B && (!x || !out))) return fail(AMR_E_INVALID, "amr_fsk_split_bandpass_host: NULL argument");
  if (!dtype_size(dtype)) return fail(AMR_E_INVALID, "unknown dtype");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  if (!plan->split_ok) return fail(AMR_E_INVALID, "the plan's filters have no time-split design");
  if (B > plan->max_streams || B > 65535) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < plan->p.n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  // FS0's start states are B x 2 x ceil(m1 / L) x 48 B (outside split_reserved's
  // L >= kFskSplitConvMinL estimate): a smaller chunk is refused
  if (chunk < 0 || (chunk > 0 && chunk < kFskSplitConvMinL && fsk_split_conv_on(plan)))
    return fail(AMR_E_INVALID, "amr_fsk_split_bandpass_host: chunk must be 0 (the plan's) or >= 128 with the convolution starts");
  if (B == 0) return AMR_OK;
  const int64_t n = plan->p.n;
  void* xs = nullptr;
  if (int rc = stage_input(plan, x, dtype, B, x_stride, &xs)) return rc;
  if (int rc = ensure_split_buffers(plan, B)) return rc;
  FskParams p = plan->p;
  p.lc = LiveCols{};                         // natural order for the caller
  p.amb = nullptr;
  FskSplit sp = fsk_split_params(plan, B, chunk);
  if (int rc = ensure_split_conv(plan, sp, B)) return rc;
  HIP_TRY(launch_fsk_split(dtype, xs, n, B, plan->mem.z.as<double2>(), p, plan->f, sp, plan->stream));
  HIP_TRY(hipMemcpyAsync(out, plan->mem.z.as<double2>(), (size_t)(B * n * 16), hipMemcpyDeviceToHost, plan->stream));
  HIP_TRY(hipStreamSynchronize(plan->stream));
  return AMR_OK;
}

int amr_fsk_plan_synchronize(amr_fsk_plan* plan) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_synchronize(*plan);
}

int amr_fsk_plan_enable_timing(amr_fsk_plan* plan, int on) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_enable_timing(*plan, on);
}

int amr_fsk_plan_set_exact_mode(amr_fsk_plan* plan, int mode) {
  if (!plan || mode < 0 || mode > 2) return fail(AMR_E_INVALID, "amr_fsk_plan_set_exact_mode: bad argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (mode != 0 && !plan->exact_on) return fail(AMR_E_INVALID, "this plan has no exact path (no decisions, or AMR_FSK_EXACT=0)");
  plan->exact_mode = mode;
  // F3 reads a flagged stream's bits from xbits only while the exact path runs
  plan->p.xflags = mode ? plan->mem.xflags.as<uint32_t>() : nullptr;
  return AMR_OK;
}

int amr_fsk_plan_exact_streams(amr_fsk_plan* plan, int64_t* count) {
  if (!plan || !count) return fail(AMR_E_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  HIP_TRY(hipStreamSynchronize(plan->stream));
  *count = 0;
  if (!plan->exact_on || !plan->ran_exact) return AMR_OK;
  int32_t c = 0;
  HIP_TRY(hipMemcpy(&c, plan->mem.xlist.as<int32_t>() + plan->max_streams, 4, hipMemcpyDeviceToHost));
  *count = c;
  return AMR_OK;
}

int amr_fsk_plan_timings(amr_fsk_plan* plan, float* ms, int count) {
  if (!plan || !ms) return fail(AMR_E_INVALID, "NULL argument");
  return core_timings(*plan, ms, count);
}

int amr_fsk_allgather(amr_comm* comm, const void* d_send, void* d_recv, int64_t bytes_per_rank, amr_fsk_plan* plan) {
  if (!plan) return allgather_after(comm, d_send, d_recv, bytes_per_rank, nullptr, nullptr);
  std::lock_guard<std::mutex> lk(plan->mu);
  return allgather_after(comm, d_send, d_recv, bytes_per_rank, plan->stream, &plan->gate,
                         plan->timing && plan->ev_used[AMR_TF_LAUNCH] ? plan->ev[AMR_TF_LAUNCH][1] : nullptr);
}

int amr_fsk_demod_device(amr_fsk_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                         uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx) {
  if (!plan || (n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx)))
    return fail(AMR_E_INVALID, "amr_fsk_demod_device: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_fsk(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx});
}

int amr_fsk_demod_device_edges(amr_fsk_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                               const double* d_edges, uint8_t* d_out, int64_t out_stride, int64_t* d_out_len,
                               int64_t* d_sync_idx) {
  if (!plan || (n_streams && (!d_x || !d_edges || !d_out || !d_out_len || !d_sync_idx)))
    return fail(AMR_E_INVALID, "amr_fsk_demod_device_edges: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_fsk(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx}, d_edges);
}

}  // extern "C"

namespace {
// A host entry (plan_core.h host_round_trip), blocking or queued; edges: the
// raw-integer capture's table, staged in d_edge
int fsk_demod_host(amr_fsk_plan* plan, const char* who, const DemodIo& h, Copy how, const double* edges = nullptr) {
  return host_round_trip(plan, who, h, how, [&]() -> int {
    amr_fsk_plan::Mem& m = plan->mem;
    if (int rc = ensure_out_staging(plan)) return rc;
    DemodIo d{nullptr, h.dtype, h.B, plan->p.n, m.d_out.as<uint8_t>(), plan->out_cap, m.d_len.as<int64_t>(),
              m.d_sync.as<int64_t>()};
    core_clear_used(*plan);
    // no decision window: the empty outputs, and no input staged
    if (plan->p.n_bits == 0) return fsk_empty_outputs(plan, h.B, d.len, d.sync);
    void* xs = nullptr;
    if (int rc = stage_input(plan, h.x, h.dtype, h.B, h.x_stride, &xs, how)) return rc;
    d.x = xs;
    if (edges)
      HIP_TRY(hipMemcpyAsync(m.d_edge.get(), edges, (size_t)(h.B * 2 * (int64_t)plan->p.pad * 8), hipMemcpyHostToDevice,
                             plan->stream));
    // a blocking call waits anyway: the exact path sized by the batch's own count
    plan->count_sync = how == Copy::sync;
    const int rc = run_fsk(plan, d, edges ? m.d_edge.as<double>() : nullptr);
    plan->count_sync = false;
    return rc;
  });
}
}  // namespace

extern "C" {

int amr_fsk_demod_host(amr_fsk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, uint8_t* out,
                       int64_t out_stride, int64_t* out_len, int64_t* sync_idx) {
  return fsk_demod_host(plan, "amr_fsk_demod_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx},
                        Copy::sync);
}

int amr_fsk_demod_host_edges(amr_fsk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                             const double* edges, uint8_t* out, int64_t out_stride, int64_t* out_len,
                             int64_t* sync_idx) {
  if (B && !edges) return fail(AMR_E_INVALID, "amr_fsk_demod_host_edges: NULL edges");
  return fsk_demod_host(plan, "amr_fsk_demod_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx},
                        Copy::sync, edges);
}

// Queued host entry (as amr_psk_demod_host_async): upload, demod, download on
// the plan's stream, no wait; host buffers untouched until amr_fsk_plan_synchronize.
int amr_fsk_demod_host_async(amr_fsk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                             uint8_t* out, int64_t out_stride, int64_t* out_len, int64_t* sync_idx) {
  return fsk_demod_host(plan, "amr_fsk_demod_host_async",
                        {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx}, Copy::async);
}

int amr_fsk_envelopes_host(amr_fsk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                           double* mark_env, double* space_env) {
  if (!plan || (B && (!x || !mark_env || !space_env))) return fail(AMR_E_INVALID, "NULL argument");
  if (!dtype_size(dtype)) return fail(AMR_E_INVALID, "unknown dtype");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  if (B > plan->max_streams) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < plan->p.n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  if (B == 0) return AMR_OK;
  const int64_t n = plan->p.n;
  std::vector<double> h((size_t)(B * n * 2));
  if (plan->p.lc.on) {
    // the envelopes at every sample need the natural layout's full passes: run
    // them on temporary buffers (a diagnostic entry, tests/test_gpu_fsk.py)
    const int64_t M = plan->fft.M;
    const int64_t ub = std::max(B * M * 16, fsk_bandpass_scratch_bytes(B, n, plan->p.pad));
    const auto nomem = [](hipError_t e) {
      return fail(AMR_E_NOMEM, std::string("envelope buffers: ") + hipGetErrorString(e));
    };
    DevBuf z, u, v, xs;
    HIP_TRY_ELSE(z.reserve(B * n * 16, nullptr), nomem);
    HIP_TRY_ELSE(u.reserve(ub, nullptr), nomem);
    HIP_TRY_ELSE(v.reserve(B * M * 16, nullptr), nomem);
    HIP_TRY_ELSE(xs.reserve(B * n * 8, nullptr), nomem);
    if (int rc = copy_batch_h2d(xs.get(), x, n * dtype_size(dtype), x_stride * dtype_size(dtype), B, plan->stream))
      return rc;
    amr_fsk_plan::Mem& m = plan->mem;
    FskParams pn = plan->p;
    pn.lc = LiveCols{};
    const auto exchange = [&] {                  // the plan's z / u / v and geometry <-> the temporaries
      m.z.swap(z);
      m.u.swap(u);
      m.v.swap(v);
      std::swap(plan->p, pn);
    };
    exchange();
    const int rc = run_fsk_front(plan, xs.get(), dtype, B, n, true);
    hipError_t e = hipSuccess;
    if (rc == AMR_OK)
      e = hipMemcpyAsync(h.data(), hilbert_out(plan->fft, m.u.as<double2>(), m.v.as<double2>()), h.size() * 8,
                         hipMemcpyDeviceToHost, plan->stream);
    // the wait whatever happened: the temporaries are freed when this block ends
    const hipError_t es = hipStreamSynchronize(plan->stream);
    exchange();
    if (rc) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(AMR_E_HIP, std::string("envelopes: ") + hipGetErrorString(e));
  } else {
    void* xs = nullptr;
    if (int rc = stage_input(plan, x, dtype, B, x_stride, &xs)) return rc;
    if (int rc = run_fsk_front(plan, xs, dtype, B, n, true)) return rc;
    HIP_TRY(hipMemcpyAsync(h.data(), hilbert_out(plan->fft, plan->mem.u.as<double2>(), plan->mem.v.as<double2>()),
                           h.size() * 8, hipMemcpyDeviceToHost, plan->stream));
    HIP_TRY(hipStreamSynchronize(plan->stream));
  }
  for (int64_t i = 0; i < B * n; ++i) {
    mark_env[i] = h[(size_t)(2 * i)];
    space_env[i] = h[(size_t)(2 * i + 1)];
  }
  return AMR_OK;
}

// The one-shot entries below declare their buffers first and their stream
// last: the StreamScope is then synchronised and destroyed before any buffer
// is freed, on every return path.
int amr_fft_c2c_host(const double* in, double* out, int64_t n, int64_t batch, int inverse, int device) {
  if (!in || !out || n < 1 || batch < 0) return fail(AMR_E_INVALID, "amr_fft_c2c_host: bad argument");
  if (batch == 0) return AMR_OK;
  HIP_TRY(hipSetDevice(device));
  DevBuf x, u, v;
  FftPlan f{};
  StreamScope st;
  HIP_TRY(StreamScope::create(st));
  if (int rc = fft_plan_init(f, n, st.get(), batch)) return rc;
  HIP_TRY(x.reserve(batch * n * 16, nullptr));
  HIP_TRY(u.reserve(batch * f.M * 16, nullptr));
  HIP_TRY(v.reserve(batch * f.M * 16, nullptr));
  HIP_TRY(hipMemcpyAsync(x.get(), in, (size_t)(batch * n * 16), hipMemcpyHostToDevice, st.get()));
  double2* const xd = x.as<double2>();
  HIP_TRY(fft_c2c(f, xd, u.as<double2>(), v.as<double2>(), xd, batch, inverse != 0, st.get()));
  HIP_TRY(hipMemcpyAsync(out, x.get(), (size_t)(batch * n * 16), hipMemcpyDeviceToHost, st.get()));
  HIP_TRY(hipStreamSynchronize(st.get()));
  return AMR_OK;
}

int amr_hilbert_host(const double* xr, double* analytic, int64_t n, int64_t batch, int device) {
  if (!xr || !analytic || n < 1 || batch < 0) return fail(AMR_E_INVALID, "amr_hilbert_host: bad argument");
  if (batch == 0) return AMR_OK;
  HIP_TRY(hipSetDevice(device));
  DevBuf x, u, v;
  FftPlan f{};
  StreamScope st;
  HIP_TRY(StreamScope::create(st));
  if (int rc = fft_plan_init(f, n, st.get(), batch)) return rc;
  std::vector<double> h((size_t)(batch * n * 2), 0.0);
  for (int64_t i = 0; i < batch * n; ++i) h[(size_t)(2 * i)] = xr[i];
  HIP_TRY(x.reserve(batch * n * 16, nullptr));
  HIP_TRY(u.reserve(batch * f.M * 16, nullptr));
  HIP_TRY(v.reserve(batch * f.M * 16, nullptr));
  HIP_TRY(hipMemcpyAsync(x.get(), h.data(), h.size() * 8, hipMemcpyHostToDevice, st.get()));
  FftEpi store{};
  store.mode = kStore;
  HIP_TRY(fft_hilbert(f, x.as<double2>(), u.as<double2>(), v.as<double2>(), batch, store, st.get()));
  HIP_TRY(hipMemcpyAsync(h.data(), hilbert_out(f, u.as<double2>(), v.as<double2>()), h.size() * 8,
                         hipMemcpyDeviceToHost, st.get()));
  HIP_TRY(hipStreamSynchronize(st.get()));
  for (int64_t i = 0; i < batch * n; ++i) {
    analytic[2 * i] = xr[i];
    analytic[2 * i + 1] = h[(size_t)(2 * i)];
  }
  return AMR_OK;
}

// pocketfft plans of one length on the device (plan struct + tables), for the
// one-shot host entries below
struct PfDev {
  PfLen L{};
  DevBuf dL, pool;
};
int pf_dev_init(PfDev& D, int64_t n, double* tmp, hipStream_t st) {
  std::vector<double> pool;
  if (!pf_len_build(n, D.L, pool)) return fail(AMR_E_INVALID, "no pocketfft plan for length " + std::to_string(n));
  HIP_TRY(D.pool.reserve((int64_t)pool.size() * 8 + 16, nullptr));
  HIP_TRY(D.dL.reserve(sizeof(PfLen), nullptr));
  HIP_TRY(hipMemcpy(D.pool.get(), pool.data(), pool.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(D.dL.get(), &D.L, sizeof(PfLen), hipMemcpyHostToDevice));
  HIP_TRY(pf_finish(D.L, D.dL.as<PfLen>(), D.pool.as<double>(), tmp, st));
  return AMR_OK;
}

int amr_resample_host(const double* x, int64_t nx, int64_t num, int64_t batch, double* y, int device) {
  if (!x || !y || nx < 1 || num < 1 || batch < 0) return fail(AMR_E_INVALID, "amr_resample_host: bad argument");
  if (batch == 0) return AMR_OK;
  HIP_TRY(hipSetDevice(device));
  const auto nomem = [](hipError_t e) {
    return fail(AMR_E_NOMEM, std::string("resample buffers: ") + hipGetErrorString(e));
  };
  const auto bad = [](hipError_t e) { return fail(AMR_E_HIP, std::string("resample: ") + hipGetErrorString(e)); };
  PfDev Dx, Dy;
  DevBuf xd, yd, slots;
  StreamScope st;
  HIP_TRY(StreamScope::create(st));
  const int n_slots = (int)std::min<int64_t>(batch, 64);
  // scratch for the slots, and for pf_finish's transform before that
  const int64_t sd = std::max(pf_scratch_doubles_n(nx), pf_scratch_doubles_n(num)) + pf_even(std::max(nx, num));
  HIP_TRY_ELSE(slots.reserve(n_slots * sd * 8, nullptr), nomem);
  HIP_TRY_ELSE(xd.reserve(batch * nx * 8, nullptr), nomem);
  HIP_TRY_ELSE(yd.reserve(batch * num * 8, nullptr), nomem);
  if (int rc = pf_dev_init(Dx, nx, slots.as<double>(), st.get())) return rc;
  if (int rc = pf_dev_init(Dy, num, slots.as<double>(), st.get())) return rc;
  const int64_t slot = pf_resample_slot_doubles(Dx.L, Dy.L);
  HIP_TRY_ELSE(hipMemcpyAsync(xd.get(), x, (size_t)(batch * nx * 8), hipMemcpyHostToDevice, st.get()), bad);
  // irfft's 1/num (pocketfft: double(1 / long double num)), then numpy's y *= num / nx
  HIP_TRY_ELSE(launch_pf_resample(Dx.dL.as<PfLen>(), Dx.pool.as<double>(), Dy.dL.as<PfLen>(), Dy.pool.as<double>(),
                                  xd.as<double>(), nx, yd.as<double>(), num, batch, slots.as<double>(), slot, n_slots,
                                  (double)(1.0L / (long double)num), (double)num / (double)nx, st.get()),
               bad);
  HIP_TRY_ELSE(hipMemcpyAsync(y, yd.get(), (size_t)(batch * num * 8), hipMemcpyDeviceToHost, st.get()), bad);
  HIP_TRY_ELSE(hipStreamSynchronize(st.get()), bad);
  return AMR_OK;
}

int amr_hilbert_env_exact_host(const double* x, int64_t n, int64_t batch, double* env, int device) {
  if (!x || !env || n < 1 || batch < 0) return fail(AMR_E_INVALID, "amr_hilbert_env_exact_host: bad argument");
  if (batch == 0) return AMR_OK;
  HIP_TRY(hipSetDevice(device));
  const auto nomem = [](hipError_t e) {
    return fail(AMR_E_NOMEM, std::string("envelope buffers: ") + hipGetErrorString(e));
  };
  const auto bad = [](hipError_t e) {
    return fail(AMR_E_HIP, std::string("exact envelopes: ") + hipGetErrorString(e));
  };
  PfDev D;
  DevBuf xd, slots;
  StreamScope st;
  HIP_TRY(StreamScope::create(st));
  const int64_t sd = pf_even(n) + pf_scratch_doubles_n(n);   // the fused envelope keeps the spectrum in its slot
  // as the FSK exact path: up to 512 persistent workgroups within 2 GiB
  const int n_slots = (int)std::max<int64_t>(1, std::min<int64_t>({batch, 512, ((int64_t)1 << 31) / (sd * 8)}));
  HIP_TRY_ELSE(slots.reserve(n_slots * sd * 8, nullptr), nomem);
  HIP_TRY_ELSE(xd.reserve(batch * n * 8, nullptr), nomem);
  if (int rc = pf_dev_init(D, n, slots.as<double>(), st.get())) return rc;
  HIP_TRY_ELSE(hipMemcpyAsync(xd.get(), x, (size_t)(batch * n * 8), hipMemcpyHostToDevice, st.get()), bad);
  HIP_TRY_ELSE(launch_pf_hilbert_env(D.dL.as<PfLen>(), D.pool.as<double>(), xd.as<double>(), n, batch,
                                     slots.as<double>(), sd, n_slots, (double)(1.0L / (long double)n),
                                     pf_hilbert_lean(D.L), st.get()),
               bad);
  HIP_TRY_ELSE(hipMemcpyAsync(env, xd.get(), (size_t)(batch * n * 8), hipMemcpyDeviceToHost, st.get()), bad);
  HIP_TRY_ELSE(hipStreamSynchronize(st.get()), bad);
  return AMR_OK;
}

}  // extern "C"
