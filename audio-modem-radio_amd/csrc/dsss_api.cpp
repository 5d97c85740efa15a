// dsss_api.cpp -- C ABI of spread, the direct-sequence DBPSK modem
// (include/amr.h): amr_dsss_plan on sym_plan.h's shared host
// core, the demodulation entries in the PSK entries' shape (soft values,
// offsets and acquisition optional), the stage entries the tests pin the
// kernels with, and the modulator.  Here: the geometry, the sign check,
// run_dsss and each entry's own checks.  The kernels are dsss_kernels.hip and
// dsss_acq_kernels.hip.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "dsss.h"
#include "sym_plan.h"
#include "tx_host.h"

using namespace amr;

namespace {
// the plan's own buffers: the tables Wc [L][2], T [L][2], cs [C]; acquisition, one group with
// mem.off from the first acquiring call on: gq [ms][segments][L], P [ms][L]
enum { kWc, kT, kCs, kGq, kP, kDsssBufs };
}  // namespace

struct amr_dsss_plan : SymPlan<AMR_TD_COUNT, kDsssBufs> {
  DsssParams p{};
};

namespace {

constexpr const char* kCapFn = "amr_dsss_plan_out_capacity";

// the geometry of include/amr.h; an AMR_E_INVALID (message set) when it is not valid
int dsss_geometry(int64_t spc, int C, int64_t cyc, int64_t* L) {
  if (C < 2 || C > kDsssMaxC) return fail(AMR_E_INVALID, "dsss: the code must have 2..64 chips");
  if (spc < 1) return fail(AMR_E_INVALID, "dsss: fewer than one sample per chip");
  if (spc > (1 << 24) || C * spc > (1 << 24)) return fail(AMR_E_INVALID, "dsss: samples per bit out of range (> 2^24)");
  *L = C * spc;
  if (cyc < 1) return fail(AMR_E_INVALID, "dsss: less than one carrier cycle per bit");
  if (2 * cyc >= *L) return fail(AMR_E_INVALID, "dsss: carrier at or above half the sample rate");
  return AMR_OK;
}

int dsss_params(int64_t n, int64_t spc, int C, int64_t cyc, DsssParams* p) {
  if (n < 0) return fail(AMR_E_INVALID, "dsss: n_samples < 0");
  *p = DsssParams{};
  if (int rc = dsss_geometry(spc, C, cyc, &p->L)) return rc;
  p->n = n;
  p->spc = spc;
  p->C = C;
  dsss_counts(*p);
  return AMR_OK;
}

int dsss_signs(const double* cs, int C) {
  for (int j = 0; j < C; ++j)
    if (!(cs[j] == 1.0 || cs[j] == -1.0)) return fail(AMR_E_INVALID, "dsss: a chip sign is not +-1.0");
  return AMR_OK;
}

int64_t y_bytes(const DsssParams& p, int64_t streams) { return std::max<int64_t>(streams * p.n_sym * 16, 16); }
int64_t plan_bytes(const DsssParams& p, int64_t ms) {    // Wc, T, cs, Y, words
  return 2 * p.L * 16 + p.C * 8 + y_bytes(p, ms) + ms * p.n_words * 4;
}
int64_t staging_bytes(const DsssParams& p, int64_t ms) {
  return std::max<int64_t>(ms * p.n * 8, 8) + ms * (p.n_bits / 8 + 1) + 2 * ms * 8;
}
// what the acquisition group holds: the segments' sums, P and the offsets
int64_t acq_bytes(const DsssParams& p, int64_t ms) {
  return std::max<int64_t>(ms * dsss_acq_segments(p) * p.L * 8, 8) + ms * p.L * 8 + ms * 8;
}

// the acquisition kernels of one batch on the plan's stream, into P / mem.off; the
// group is allocated on the first acquiring call (all or nothing)
int run_acquire(amr_dsss_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride) {
  const int64_t ms = pl->max_streams, L = pl->p.L;
  auto& m = pl->mem;
  HIP_TRY((reserve_all({{m.own[kGq], std::max<int64_t>(ms * dsss_acq_segments(pl->p) * L * 8, 8)},
                        {m.own[kP], ms * L * 8},
                        {m.off, ms * 8}},
                       pl->stream)));
  const DsssAcq a{m.own[kGq].as<double>(), m.own[kP].as<double>(), m.off.as<int64_t>()};
  HIP_TRY_TIMED(*pl, AMR_TD_ACQUIRE,
                launch_dsss_acquire(d_x, dtype, x_stride, B, pl->p, m.own[kWc].as<double>(), m.own[kCs].as<double>(), a,
                                    pl->stream));
  return AMR_OK;
}

// One batch on the plan's stream (device pointers; the caller holds mu and has
// set the device).  soft: non-null, k_dsss_soft behind the sync search.
// acquire: the streams' offsets first (run_acquire), the despreader at them;
// d_offset (device, or null) receives them, zeros when nothing was acquired.
int run_dsss(amr_dsss_plan* pl, const DemodIo& io, int8_t* soft, int64_t soft_stride, bool acquire,
             int64_t* d_offset) {
  if (int rc = check_demod_args(pl, io, ArgOrder::device)) return rc;
  core_clear_used(*pl);
  if (io.B == 0) return AMR_OK;
  const DsssParams& p = pl->p;
  hipStream_t st = pl->stream;
  return timed(*pl, AMR_TD_LAUNCH, [&]() -> int {
    if (acquire) {
      if (int rc = run_acquire(pl, io.x, io.dtype, io.B, io.x_stride)) return rc;
      if (d_offset)
        HIP_TRY(hipMemcpyAsync(d_offset, pl->mem.off.get(), (size_t)io.B * 8, hipMemcpyDeviceToDevice, st));
    } else if (d_offset) {
      HIP_TRY(hipMemsetAsync(d_offset, 0, (size_t)io.B * 8, st));
    }
    if (p.n_sym < 2) {                               // fewer than two bits' worth: b"", sync -1
      HIP_TRY(hipMemsetAsync(io.len, 0, (size_t)io.B * 8, st));
      HIP_TRY(hipMemsetAsync(io.sync, 0xFF, (size_t)io.B * 8, st));
      return AMR_OK;
    }
    double* Y = pl->mem.Y.as<double>();
    uint32_t* words = pl->mem.words.as<uint32_t>();
    HIP_TRY_TIMED(*pl, AMR_TD_DESPREAD,
                  launch_dsss_despread(io.x, io.dtype, io.x_stride, io.B, p, pl->mem.own[kT].as<double>(),
                                       acquire ? pl->mem.off.as<int64_t>() : nullptr, Y, st));
    HIP_TRY_TIMED(*pl, AMR_TD_SLICE, launch_dsss_slice(Y, io.B, p, words, st));
    return timed(*pl, AMR_TD_SYNC_PACK, [&]() -> int {
      HIP_TRY(launch_sync_pack(words, p.n_words, p.n_bits, io.B, io.out, io.out_stride, io.len, io.sync, st));
      if (soft) HIP_TRY(launch_dsss_soft(Y, io.B, p, words, io.sync, io.len, soft, soft_stride, st));
      return AMR_OK;
    });
  });
}

// amr_dsss_acquire_host / _device (sym_plan.h acquire_entry): the offsets and P
int dsss_acquire_entry(amr_dsss_plan* plan, const char* who, bool host, const void* x, int dtype, int64_t B,
                       int64_t x_stride, int64_t* offset, double* P) {
  if (!plan) return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  return acquire_entry(plan, who, host, x, dtype, B, x_stride, offset, {{P, &plan->mem.own[kP], plan->p.L * 8}},
                       [&](const void* d_x, int64_t stride) { return run_acquire(plan, d_x, dtype, B, stride); });
}

// the stage entries: k_dsss_slice on given Y (the words to `words`, or null), with `soft` k_dsss_soft
int dsss_symbol_stages(const char* who, const double* Y, int64_t n_streams, int64_t n_sym, uint32_t* words,
                       int8_t* soft) {
  return symbol_stages(
      who, DsssParams{}, 1, 1, Y, n_streams, n_sym, words, soft,
      [&](const double* y, const DsssParams& q, uint32_t* w) { return launch_dsss_slice(y, n_streams, q, w, nullptr); },
      [&](const double* y, const DsssParams& q, const uint32_t* w, int8_t* s) {
        return launch_dsss_soft(y, n_streams, q, w, nullptr, nullptr, s, q.n_bits, nullptr);
      });
}

}  // namespace

extern "C" {

int amr_dsss_plan_create(amr_dsss_plan** out, int device, int64_t n_samples, int64_t spc, int C, int64_t cyc,
                         const double* Wc, const double* T, const double* cs, int64_t max_streams) {
  if (!out || !Wc || !T || !cs) return fail(AMR_E_INVALID, "amr_dsss_plan_create: NULL argument");
  *out = nullptr;
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_dsss_plan_create: max_streams < 1");
  DsssParams p;
  if (int rc = dsss_params(n_samples, spc, C, cyc, &p)) return rc;
  if (int rc = dsss_signs(cs, C)) return rc;
  auto* pl = new amr_dsss_plan();
  pl->p = p;
  auto& m = pl->mem;
  return sym_plan_setup(pl, device, max_streams,
                        {{&m.own[kWc], p.L * 16, Wc},
                         {&m.own[kT], p.L * 16, T},
                         {&m.own[kCs], (int64_t)C * 8, cs},
                         {&m.Y, y_bytes(p, max_streams), nullptr},
                         {&m.words, max_streams * p.n_words * 4, nullptr}},
                        out);
}

int amr_dsss_plan_destroy(amr_dsss_plan* plan) {
  sym_plan_free(plan);
  return AMR_OK;
}

int amr_dsss_plan_synchronize(amr_dsss_plan* plan) { return sym_plan_synchronize(plan); }
int amr_dsss_plan_enable_timing(amr_dsss_plan* plan, int on) { return sym_plan_enable_timing(plan, on); }
int amr_dsss_plan_timings(amr_dsss_plan* plan, float* ms, int count) { return sym_plan_timings(plan, ms, count); }
int64_t amr_dsss_plan_out_capacity(const amr_dsss_plan* plan) { return plan ? plan->out_cap : -1; }
int64_t amr_dsss_plan_scratch_bytes(const amr_dsss_plan* plan) { return plan ? plan->mem.bytes() : -1; }

int64_t amr_dsss_plan_bytes_estimate(int64_t n_samples, int64_t spc, int C, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_dsss_plan_bytes_estimate: max_streams < 1");
  DsssParams p;
  // the byte counts depend on (spc, C) alone; one cycle per bit is valid wherever any carrier is (L >= 3)
  if (int rc = dsss_params(n_samples, spc, C, 1, &p)) return rc;
  return plan_bytes(p, max_streams) + staging_bytes(p, max_streams);
}

int64_t amr_dsss_acquire_bytes_estimate(int64_t n_samples, int64_t spc, int C, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_dsss_acquire_bytes_estimate: max_streams < 1");
  DsssParams p;
  if (int rc = dsss_params(n_samples, spc, C, 1, &p)) return rc;
  return acq_bytes(p, max_streams);
}

int amr_dsss_demod_device(amr_dsss_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                          uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx, int8_t* d_soft,
                          int64_t soft_stride, int64_t* d_offset, int acquire) {
  if (int rc = demod_precheck(plan, "amr_dsss_demod_device", kCapFn, n_streams, x_stride, out_stride,
                              d_soft != nullptr, soft_stride))
    return rc;
  if (n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx))
    return fail(AMR_E_INVALID, "amr_dsss_demod_device: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_dsss(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx}, d_soft,
                  soft_stride, acquire != 0, d_offset);
}

int amr_dsss_demod_host(amr_dsss_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, uint8_t* out,
                        int64_t out_stride, int64_t* out_len, int64_t* sync_idx, int8_t* soft, int64_t soft_stride,
                        int64_t* offset, int acquire) {
  if (int rc = demod_precheck(plan, "amr_dsss_demod_host", kCapFn, B, x_stride, out_stride, soft != nullptr,
                              soft_stride))
    return rc;
  return demod_host(plan, "amr_dsss_demod_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx}, soft,
                    soft_stride, offset, acquire != 0, [&](const DemodIo& d, int8_t* d_soft, int64_t sv) {
                      return run_dsss(plan, d, d_soft, sv, acquire != 0, nullptr);
                    });
}

int amr_dsss_acquire_host(amr_dsss_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, int64_t* offset,
                          double* P) {
  return dsss_acquire_entry(plan, "amr_dsss_acquire_host", true, x, dtype, B, x_stride, offset, P);
}

int amr_dsss_acquire_device(amr_dsss_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                            int64_t* d_offset, double* d_P) {
  return dsss_acquire_entry(plan, "amr_dsss_acquire_device", false, d_x, dtype, n_streams, x_stride, d_offset, d_P);
}

int amr_dsss_symbols_at_host(amr_dsss_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                             const int64_t* offset, double* Y) {
  if (!plan || (B && (!x || !offset || !Y))) return fail(AMR_E_INVALID, "amr_dsss_symbols_at_host: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (int rc = batch_check(plan, dtype, B, x_stride)) return rc;
  const DsssParams& p = plan->p;
  for (int64_t i = 0; i < B; ++i)
    if (offset[i] < 0 || offset[i] > p.L - 1)
      return fail(AMR_E_INVALID, "amr_dsss_symbols_at_host: offset outside [0, L - 1]");
  return symbols_round_trip(plan, x, dtype, B, x_stride, offset, Y, B * p.n_sym * 16,
                            [&](const void* d_x, const int64_t* d_off) {
                              return launch_dsss_despread(d_x, dtype, p.n, B, p, plan->mem.own[kT].as<double>(), d_off,
                                                          plan->mem.Y.as<double>(), plan->stream);
                            });
}

int amr_dsss_slice_host(const double* Y, int64_t n_streams, int64_t n_sym, uint32_t* words) {
  if (n_streams > 0 && n_sym > 0 && !words) return fail(AMR_E_INVALID, "amr_dsss_slice_host: bad argument");
  return dsss_symbol_stages("amr_dsss_slice_host", Y, n_streams, n_sym, words, nullptr);
}

int amr_dsss_soft_host(const double* Y, int64_t n_streams, int64_t n_sym, int8_t* soft) {
  if (n_streams > 0 && n_sym > 0 && !soft) return fail(AMR_E_INVALID, "amr_dsss_soft_host: bad argument");
  return dsss_symbol_stages("amr_dsss_soft_host", Y, n_streams, n_sym, nullptr, soft);
}

int amr_dsss_modulate_host(int64_t spc, int C, int64_t cyc, const double* cs, const double* Sn, const uint8_t* data,
                           int64_t data_stride, const int64_t* n_bytes, int64_t n, float* out, int64_t out_stride,
                           int64_t n_out, int16_t* pcm, int64_t pcm_stride) {
  constexpr const char* who = "amr_dsss_modulate_host";
  if (n < 0 || n_out < 0 || data_stride < 0 || out_stride < n_out || (pcm && pcm_stride < n_out))
    return fail(AMR_E_INVALID, "amr_dsss_modulate_host: bad argument");
  if (!cs || !Sn) return fail(AMR_E_INVALID, "amr_dsss_modulate_host: NULL table");
  if (n && (!n_bytes || (n_out && !out))) return fail(AMR_E_INVALID, "amr_dsss_modulate_host: NULL buffer");
  DsssTx t{};
  if (int rc = dsss_geometry(spc, C, cyc, &t.L)) return rc;
  if (int rc = dsss_signs(cs, C)) return rc;
  t.spc = spc;
  t.C = C;
  t.n_out = n_out;
  if (n > 65535) return fail(AMR_E_INVALID, "amr_dsss_modulate_host: at most 65535 streams per call");
  if (n_out > 0x7fffffffLL) return fail(AMR_E_INVALID, "amr_dsss_modulate_host: n_out >= 2^31");
  t.sym_stride = (n_out + t.L - 1) / t.L;
  DevBuf d_tab, d_sign;                            // freed after the round trip has drained the device
  return modulate_round_trip(who, data, data_stride, n_bytes, n, out, out_stride, n_out, pcm, pcm_stride,
                             [&](const TxDev& d) -> int {
    const auto bad = hip_fail_as(who);
    std::vector<double> tab((size_t)t.L);          // sg[i] * Sn[i], an exact sign flip
    for (int64_t i = 0; i < t.L; ++i) tab[(size_t)i] = cs[i / spc] * Sn[i];
    HIP_TRY_ELSE(d_tab.reserve(t.L * 8, nullptr), bad);
    HIP_TRY_ELSE(d_sign.reserve(n * t.sym_stride, nullptr), bad);
    HIP_TRY_ELSE(hipMemcpy(d_tab.get(), tab.data(), (size_t)t.L * 8, hipMemcpyHostToDevice), bad);
    HIP_TRY_ELSE(launch_dsss_tx(t, d_tab.as<double>(), d.data, d.stride, d.n_bytes, n, d_sign.as<int8_t>(), d.out,
                                n_out, d.pcm, n_out, nullptr),
                 bad);
    return AMR_OK;
  });
}

}  // extern "C"
