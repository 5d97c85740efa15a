// ofdm_api.cpp -- C ABI of the multi-carrier DQPSK modem (include/amr.h,
// DESIGN.md §3j): amr_ofdm_plan on sym_plan.h's shared host core, the
// demodulation entries in the PSK entries' shape, the stage entries the tests
// pin the kernels with, the modulator, and acquisition (§3k: the work buffers,
// the stage entries and the acquired demodulation).  Here: the geometry, the
// W table, run_ofdm and each entry's own checks.  The kernels are
// ofdm_kernels.hip and ofdm_acq_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "ofdm.h"
#include "sym_plan.h"
#include "tx_host.h"

using namespace amr;

namespace {
// the plan's own buffers: W [nu][K][2]; acquisition, one group with mem.off from the
// first acquiring call on: gq [ms][segments][L], G [ms][L], E [ms][L], dhat [ms]
enum { kW, kGq, kG, kE, kDhat, kOfdmBufs };
}  // namespace

struct amr_ofdm_plan : SymPlan<AMR_TO_COUNT, kOfdmBufs> {
  OfdmParams p{};
};

namespace {

constexpr const char* kCapFn = "amr_ofdm_plan_out_capacity";

// the geometry of include/amr.h; an AMR_E_INVALID (message set) when it is not valid
int ofdm_geometry(int64_t sps, int K, int64_t bin0, int64_t* L, int64_t* ncp, int64_t* nu) {
  if (K < 1 || K > kOfdmMaxK) return fail(AMR_E_INVALID, "ofdm: num_subcarriers must be 1..64");
  if (sps < 1) return fail(AMR_E_INVALID, "ofdm: fewer than one sample per dibit");
  if (sps > (1 << 24)) return fail(AMR_E_INVALID, "ofdm: samples per dibit out of range (> 2^24)");
  *L = K * sps;
  *ncp = *L / 8;
  *nu = *L - *ncp;
  if (bin0 < 1) return fail(AMR_E_INVALID, "ofdm: lowest subcarrier below bin 1");
  if (2 * (bin0 + K - 1) >= *nu) return fail(AMR_E_INVALID, "ofdm: highest subcarrier at or above Nu / 2");
  return AMR_OK;
}

int ofdm_params(int64_t n, int64_t sps, int K, int64_t bin0, OfdmParams* p) {
  if (n < 0) return fail(AMR_E_INVALID, "ofdm: n_samples < 0");
  *p = OfdmParams{};
  if (int rc = ofdm_geometry(sps, K, bin0, &p->L, &p->ncp, &p->nu)) return rc;
  p->n = n;
  p->sps = sps;
  p->K = K;
  p->bin0 = (int)bin0;
  ofdm_counts(*p);
  return AMR_OK;
}

int64_t y_bytes(const OfdmParams& p, int64_t streams) {
  return std::max<int64_t>(streams * p.n_sym * p.K * 16, 16);
}
int64_t plan_bytes(const OfdmParams& p, int64_t ms) {   // W, Y, words
  return p.nu * p.K * 16 + y_bytes(p, ms) + ms * p.n_words * 4;
}
int64_t staging_bytes(const OfdmParams& p, int64_t ms) {
  return std::max<int64_t>(ms * p.n * 8, 8) + ms * (p.n_bits / 8 + 1) + 2 * ms * 8;
}

// what the acquisition group holds: the fold's segment sums, G, E, dhat and the offsets
int64_t acq_bytes(const OfdmParams& p, int64_t ms) {
  return std::max<int64_t>(ms * ofdm_acq_segments(p) * p.L * 8, 8) + 2 * ms * p.L * 8 + 2 * ms * 8;
}

// the acquisition kernels of one batch on the plan's stream, into E / dhat / mem.off; the
// group is allocated on the first acquiring call (all or nothing)
int run_acquire(amr_ofdm_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride) {
  const int64_t ms = pl->max_streams, L = pl->p.L;
  auto& m = pl->mem;
  HIP_TRY((reserve_all({{m.own[kGq], std::max<int64_t>(ms * ofdm_acq_segments(pl->p) * L * 8, 8)},
                        {m.own[kG], ms * L * 8},
                        {m.own[kE], ms * L * 8},
                        {m.own[kDhat], ms * 8},
                        {m.off, ms * 8}},
                       pl->stream)));
  const OfdmAcq a{m.own[kGq].as<double>(), m.own[kG].as<double>(), m.own[kE].as<double>(), m.own[kDhat].as<int64_t>(),
                  m.off.as<int64_t>()};
  HIP_TRY_TIMED(*pl, AMR_TO_ACQUIRE, launch_ofdm_acquire(d_x, dtype, x_stride, B, pl->p, a, pl->stream));
  return AMR_OK;
}

// One batch on the plan's stream (device pointers; the caller holds mu and
// has set the device).  soft: non-null, k_ofdm_soft behind the sync search.
// acquire: the streams' offsets first (run_acquire), the DFT at them; d_offset
// (device, or null) receives them.
int run_ofdm(amr_ofdm_plan* pl, const DemodIo& io, int8_t* soft, int64_t soft_stride, bool acquire = false,
             int64_t* d_offset = nullptr) {
  if (int rc = check_demod_args(pl, io, ArgOrder::device)) return rc;
  core_clear_used(*pl);
  if (io.B == 0) return AMR_OK;
  const OfdmParams& p = pl->p;
  hipStream_t st = pl->stream;
  return timed(*pl, AMR_TO_LAUNCH, [&]() -> int {
    if (acquire) {
      if (int rc = run_acquire(pl, io.x, io.dtype, io.B, io.x_stride)) return rc;
      if (d_offset)
        HIP_TRY(hipMemcpyAsync(d_offset, pl->mem.off.get(), (size_t)io.B * 8, hipMemcpyDeviceToDevice, st));
    }
    if (p.n_sym < 2) {                               // fewer than two symbols: b"", sync -1
      HIP_TRY(hipMemsetAsync(io.len, 0, (size_t)io.B * 8, st));
      HIP_TRY(hipMemsetAsync(io.sync, 0xFF, (size_t)io.B * 8, st));
      return AMR_OK;
    }
    const double* W = pl->mem.own[kW].as<double>();
    double* Y = pl->mem.Y.as<double>();
    uint32_t* words = pl->mem.words.as<uint32_t>();
    if (acquire)
      HIP_TRY_TIMED(*pl, AMR_TO_DFT, launch_ofdm_dft_at(io.x, io.dtype, io.x_stride, io.B, p, W,
                                                        pl->mem.off.as<int64_t>(), Y, st));
    else
      HIP_TRY_TIMED(*pl, AMR_TO_DFT, launch_ofdm_dft(io.x, io.dtype, io.x_stride, io.B, p, W, Y, st));
    HIP_TRY_TIMED(*pl, AMR_TO_SLICE, launch_ofdm_slice(Y, io.B, p, words, st));
    return timed(*pl, AMR_TO_SYNC_PACK, [&]() -> int {
      HIP_TRY(launch_sync_pack(words, p.n_words, p.n_bits, io.B, io.out, io.out_stride, io.len, io.sync, st));
      if (soft) HIP_TRY(launch_ofdm_soft(Y, io.B, p, words, io.sync, io.len, soft, soft_stride, st));
      return AMR_OK;
    });
  });
}

// a host entry: sym_plan.h's round trip around run_ofdm
int ofdm_demod_host(amr_ofdm_plan* plan, const char* who, const DemodIo& h, int8_t* soft, int64_t soft_stride,
                    bool acquire = false, int64_t* offset = nullptr) {
  return demod_host(plan, who, h, soft, soft_stride, offset, acquire,
                    [&](const DemodIo& d, int8_t* d_soft, int64_t sv) { return run_ofdm(plan, d, d_soft, sv, acquire); });
}

// the stage entries: k_ofdm_slice on given Y (the words to `words`, or null), with `soft` k_ofdm_soft
int ofdm_symbol_stages(const char* who, const double* Y, int64_t n_streams, int64_t n_sym, int K, uint32_t* words,
                       int8_t* soft) {
  if (K < 1 || K > kOfdmMaxK) return fail(AMR_E_INVALID, std::string(who) + ": num_subcarriers must be 1..64");
  OfdmParams p{};
  p.K = K;
  return symbol_stages(
      who, p, K, 2 * (int64_t)K, Y, n_streams, n_sym, words, soft,
      [&](const double* y, const OfdmParams& q, uint32_t* w) { return launch_ofdm_slice(y, n_streams, q, w, nullptr); },
      [&](const double* y, const OfdmParams& q, const uint32_t* w, int8_t* s) {
        return launch_ofdm_soft(y, n_streams, q, w, nullptr, nullptr, s, q.n_bits, nullptr);
      });
}

// amr_ofdm_acquire_host / _device (sym_plan.h acquire_entry): the offsets, dhat and E
int ofdm_acquire_entry(amr_ofdm_plan* plan, const char* who, bool host, const void* x, int dtype, int64_t B,
                       int64_t x_stride, int64_t* offset, int64_t* dhat, double* E) {
  if (!plan) return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  return acquire_entry(plan, who, host, x, dtype, B, x_stride, offset,
                       {{dhat, &plan->mem.own[kDhat], 8}, {E, &plan->mem.own[kE], plan->p.L * 8}},
                       [&](const void* d_x, int64_t stride) { return run_acquire(plan, d_x, dtype, B, stride); });
}

}  // namespace

extern "C" {

int amr_ofdm_plan_create(amr_ofdm_plan** out, int device, int64_t n_samples, int64_t sps, int K, const int32_t* bins,
                         const double* W, int64_t max_streams) {
  if (!out || !bins || !W) return fail(AMR_E_INVALID, "amr_ofdm_plan_create: NULL argument");
  *out = nullptr;
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_ofdm_plan_create: max_streams < 1");
  if (K < 1 || K > kOfdmMaxK) return fail(AMR_E_INVALID, "ofdm: num_subcarriers must be 1..64");
  OfdmParams p;
  if (int rc = ofdm_params(n_samples, sps, K, bins[0], &p)) return rc;
  for (int k = 1; k < K; ++k)
    if (bins[k] != bins[0] + k) return fail(AMR_E_INVALID, "ofdm: bins must be consecutive");
  // [K][nu][2] -> [nu][K][2]: a group of subcarriers at one m contiguous (k_ofdm_dft's uniform loads)
  std::vector<double> w((size_t)(p.nu * K * 2));
  for (int k = 0; k < K; ++k)
    for (int64_t i = 0; i < p.nu; ++i)
      for (int c = 0; c < 2; ++c) w[(size_t)((i * K + k) * 2 + c)] = W[(size_t)((k * p.nu + i) * 2 + c)];
  auto* pl = new amr_ofdm_plan();
  pl->p = p;
  auto& m = pl->mem;
  return sym_plan_setup(pl, device, max_streams,
                        {{&m.own[kW], p.nu * K * 16, w.data()},
                         {&m.Y, y_bytes(p, max_streams), nullptr},
                         {&m.words, max_streams * p.n_words * 4, nullptr}},
                        out);
}

int amr_ofdm_plan_destroy(amr_ofdm_plan* plan) {
  sym_plan_free(plan);
  return AMR_OK;
}

int amr_ofdm_plan_synchronize(amr_ofdm_plan* plan) { return sym_plan_synchronize(plan); }
int amr_ofdm_plan_enable_timing(amr_ofdm_plan* plan, int on) { return sym_plan_enable_timing(plan, on); }
int amr_ofdm_plan_timings(amr_ofdm_plan* plan, float* ms, int count) { return sym_plan_timings(plan, ms, count); }
int64_t amr_ofdm_plan_out_capacity(const amr_ofdm_plan* plan) { return plan ? plan->out_cap : -1; }
int64_t amr_ofdm_plan_scratch_bytes(const amr_ofdm_plan* plan) { return plan ? plan->mem.bytes() : -1; }

int64_t amr_ofdm_acquire_bytes_estimate(int64_t n_samples, int64_t sps, int K, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_ofdm_acquire_bytes_estimate: max_streams < 1");
  OfdmParams p;
  if (int rc = ofdm_params(n_samples, sps, K, 1, &p)) return rc;
  return acq_bytes(p, max_streams);
}

int64_t amr_ofdm_plan_bytes_estimate(int64_t n_samples, int64_t sps, int K, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_ofdm_plan_bytes_estimate: max_streams < 1");
  OfdmParams p;
  // the byte counts depend on (sps, K) alone; bin 1 is valid wherever any bin is
  if (int rc = ofdm_params(n_samples, sps, K, 1, &p)) return rc;
  return plan_bytes(p, max_streams) + staging_bytes(p, max_streams);
}

int amr_ofdm_demod_device(amr_ofdm_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                          uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx) {
  if (!plan || (n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx)))
    return fail(AMR_E_INVALID, "amr_ofdm_demod_device: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_ofdm(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx}, nullptr, 0);
}

int amr_ofdm_demod_soft_device(amr_ofdm_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                               uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx,
                               int8_t* d_soft, int64_t soft_stride) {
  if (int rc = demod_precheck(plan, "amr_ofdm_demod_soft_device", kCapFn, n_streams, x_stride, out_stride, true,
                              soft_stride, n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx || !d_soft)))
    return rc;
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_ofdm(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx}, d_soft,
                  soft_stride);
}

int amr_ofdm_demod_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, uint8_t* out,
                        int64_t out_stride, int64_t* out_len, int64_t* sync_idx) {
  return ofdm_demod_host(plan, "amr_ofdm_demod_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx},
                         nullptr, 0);
}

int amr_ofdm_demod_soft_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, uint8_t* out,
                             int64_t out_stride, int64_t* out_len, int64_t* sync_idx, int8_t* soft,
                             int64_t soft_stride) {
  if (int rc = demod_precheck(plan, "amr_ofdm_demod_soft_host", kCapFn, B, x_stride, out_stride, true, soft_stride,
                              B && !soft))
    return rc;
  return ofdm_demod_host(plan, "amr_ofdm_demod_soft_host",
                         {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx}, soft, soft_stride);
}

int amr_ofdm_symbols_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, double* Y) {
  if (!plan || (B && (!x || !Y))) return fail(AMR_E_INVALID, "amr_ofdm_symbols_host: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (int rc = batch_check(plan, dtype, B, x_stride)) return rc;
  const OfdmParams& p = plan->p;
  return symbols_round_trip(plan, x, dtype, B, x_stride, nullptr, Y, B * p.n_sym * p.K * 16,
                            [&](const void* d_x, const int64_t*) {
                              return launch_ofdm_dft(d_x, dtype, p.n, B, p, plan->mem.own[kW].as<double>(),
                                                     plan->mem.Y.as<double>(), plan->stream);
                            });
}

int amr_ofdm_symbols_at_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                             const int64_t* offset, double* Y) {
  if (!plan || (B && (!x || !offset || !Y))) return fail(AMR_E_INVALID, "amr_ofdm_symbols_at_host: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (int rc = batch_check(plan, dtype, B, x_stride)) return rc;
  const OfdmParams& p = plan->p;
  for (int64_t i = 0; i < B; ++i)
    if (offset[i] < -p.ncp || offset[i] > p.L - 1 - p.ncp)
      return fail(AMR_E_INVALID, "amr_ofdm_symbols_at_host: offset outside [-Ncp, L - 1 - Ncp]");
  return symbols_round_trip(plan, x, dtype, B, x_stride, offset, Y, B * p.n_sym * p.K * 16,
                            [&](const void* d_x, const int64_t* d_off) {
                              return launch_ofdm_dft_at(d_x, dtype, p.n, B, p, plan->mem.own[kW].as<double>(), d_off,
                                                        plan->mem.Y.as<double>(), plan->stream);
                            });
}

int amr_ofdm_acquire_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, int64_t* offset,
                          int64_t* dhat, double* E) {
  return ofdm_acquire_entry(plan, "amr_ofdm_acquire_host", true, x, dtype, B, x_stride, offset, dhat, E);
}

int amr_ofdm_acquire_device(amr_ofdm_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                            int64_t* d_offset, int64_t* d_dhat, double* d_E) {
  return ofdm_acquire_entry(plan, "amr_ofdm_acquire_device", false, d_x, dtype, n_streams, x_stride, d_offset, d_dhat,
                            d_E);
}

int amr_ofdm_demod_acq_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, uint8_t* out,
                            int64_t out_stride, int64_t* out_len, int64_t* sync_idx, int8_t* soft, int64_t soft_stride,
                            int64_t* offset) {
  if (int rc = demod_precheck(plan, "amr_ofdm_demod_acq_host", kCapFn, B, x_stride, out_stride, soft != nullptr,
                              soft_stride))
    return rc;
  return ofdm_demod_host(plan, "amr_ofdm_demod_acq_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx},
                         soft, soft_stride, true, offset);
}

int amr_ofdm_demod_acq_device(amr_ofdm_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                              uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx,
                              int8_t* d_soft, int64_t soft_stride, int64_t* d_offset) {
  if (int rc = demod_precheck(plan, "amr_ofdm_demod_acq_device", kCapFn, n_streams, x_stride, out_stride,
                              d_soft != nullptr, soft_stride))
    return rc;
  if (n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx))
    return fail(AMR_E_INVALID, "amr_ofdm_demod_acq_device: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_ofdm(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx}, d_soft,
                  soft_stride, true, d_offset);
}

int amr_ofdm_slice_host(const double* Y, int64_t n_streams, int64_t n_sym, int K, uint32_t* words) {
  if (n_streams > 0 && n_sym > 0 && !words) return fail(AMR_E_INVALID, "amr_ofdm_slice_host: bad argument");
  return ofdm_symbol_stages("amr_ofdm_slice_host", Y, n_streams, n_sym, K, words, nullptr);
}

int amr_ofdm_soft_host(const double* Y, int64_t n_streams, int64_t n_sym, int K, int8_t* soft) {
  if (n_streams > 0 && n_sym > 0 && !soft) return fail(AMR_E_INVALID, "amr_ofdm_soft_host: bad argument");
  return ofdm_symbol_stages("amr_ofdm_soft_host", Y, n_streams, n_sym, K, nullptr, soft);
}

int amr_ofdm_modulate_host(double baud, double carrier, double sample_rate, int K, const uint8_t* data,
                           int64_t data_stride, const int64_t* n_bytes, int64_t n, float* out, int64_t out_stride,
                           int64_t n_out, int16_t* pcm, int64_t pcm_stride) {
  constexpr const char* who = "amr_ofdm_modulate_host";
  if (n < 0 || n_out < 0 || data_stride < 0 || out_stride < n_out || (pcm && pcm_stride < n_out))
    return fail(AMR_E_INVALID, "amr_ofdm_modulate_host: bad argument");
  if (n && (!n_bytes || (n_out && !out))) return fail(AMR_E_INVALID, "amr_ofdm_modulate_host: NULL buffer");
  if (baud == 0.0) return fail(AMR_E_INVALID, "float division by zero");
  if (!std::isfinite(baud) || !std::isfinite(sample_rate) || !std::isfinite(carrier))
    return fail(AMR_E_INVALID, "ofdm: baud, carrier and sample_rate must be finite");
  if (K < 1 || K > kOfdmMaxK) return fail(AMR_E_INVALID, "ofdm: num_subcarriers must be 1..64");
  const double q = sample_rate / baud;
  if (!(std::fabs(q) < 2147483648.0)) return fail(AMR_E_INVALID, "ofdm: samples per dibit out of range (> 2^24)");
  const int64_t sps = (int64_t)q;                              // int(samp_rate / baud)
  if (sps < 1) return fail(AMR_E_INVALID, "ofdm: fewer than one sample per dibit");
  if (sps > (1 << 24)) return fail(AMR_E_INVALID, "ofdm: samples per dibit out of range (> 2^24)");
  OfdmTx t{};
  t.K = K;
  t.L = K * sps;
  t.ncp = t.L / 8;
  t.nu = t.L - t.ncp;
  const double c0 = std::floor(carrier * (double)t.nu / sample_rate + 0.5);   // floor(carrier * Nu / samp_rate + 0.5)
  if (!(std::fabs(c0) < 1073741824.0)) return fail(AMR_E_INVALID, "ofdm: highest subcarrier at or above Nu / 2");
  const int64_t bin0 = (int64_t)c0 - K / 2;
  int64_t L, ncp, nu;
  if (int rc = ofdm_geometry(sps, K, bin0, &L, &ncp, &nu)) return rc;
  t.bin0 = (int)bin0;
  t.n_out = n_out;
  if (n > 65535) return fail(AMR_E_INVALID, "amr_ofdm_modulate_host: at most 65535 streams per call");
  if (n_out > 0x7fffffffLL) return fail(AMR_E_INVALID, "amr_ofdm_modulate_host: n_out >= 2^31");
  t.sym_stride = (n_out + t.L - 1) / t.L;
  DevBuf d_work;                                   // freed after the round trip has drained the device
  return modulate_round_trip(who, data, data_stride, n_bytes, n, out, out_stride, n_out, pcm, pcm_stride,
                             [&](const TxDev& d) -> int {
    HIP_TRY_ELSE(d_work.reserve(n * t.sym_stride * K * 8, nullptr), hip_fail_as(who));
    HIP_TRY_ELSE(launch_ofdm_tx(t, d.data, d.stride, d.n_bytes, n, d_work.as<double>(), d.out, n_out, d.pcm, n_out,
                                nullptr),
                 hip_fail_as(who));
    return AMR_OK;
  });
}

}  // extern "C"
