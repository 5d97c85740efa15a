// msk_api.cpp -- C ABI of minshift, the MSK modem (include/amr.h, DESIGN.md
// §3m): amr_msk_plan on sym_plan.h's shared host core, the demodulation entries
// in the PSK entries' shape (soft values, offsets and bit timing optional), the
// stage entries the tests pin the kernels with, and the modulator.  Here: the
// geometry, run_msk and each entry's own checks.  The kernels are
// msk_kernels.hip and msk_acq_kernels.hip.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "msk.h"
#include "sym_plan.h"
#include "tx_host.h"

using namespace amr;

namespace {
// the plan's own buffers: the tables U [L][2], E0, E1 [2 L][2], R [L][2]; bit timing, one group with
// mem.off from the first acquiring call on: seg [ms][segments][4], q [ms][2]
enum { kU, kE0, kE1, kR, kSeg, kQ, kMskBufs };
}  // namespace

struct amr_msk_plan : SymPlan<AMR_TD_COUNT, kMskBufs> {
  MskParams p{};
};

namespace {

constexpr const char* kCapFn = "amr_msk_plan_out_capacity";

// the geometry of include/amr.h; an AMR_E_INVALID (message set) when it is not valid
int msk_geometry(int64_t L, int64_t cyc4) {
  if (L < 4) return fail(AMR_E_INVALID, "msk: fewer than four samples per bit");
  if (L > (1 << 24)) return fail(AMR_E_INVALID, "msk: samples per bit out of range (> 2^24)");
  if (cyc4 < 2) return fail(AMR_E_INVALID, "msk: less than half a carrier cycle per bit");
  if (cyc4 + 1 >= 2 * L) return fail(AMR_E_INVALID, "msk: the upper tone at or above half the sample rate");
  return AMR_OK;
}

int msk_params(int64_t n, int64_t L, int64_t cyc4, MskParams* p) {
  if (n < 0) return fail(AMR_E_INVALID, "msk: n_samples < 0");
  if (int rc = msk_geometry(L, cyc4)) return rc;
  *p = MskParams{};
  p->n = n;
  p->L = L;
  p->cyc4 = cyc4;
  msk_counts(*p);
  return AMR_OK;
}

int64_t w_bytes(const MskParams& p, int64_t streams) { return std::max<int64_t>(streams * p.n_sym * 16, 16); }
int64_t plan_bytes(const MskParams& p, int64_t ms) {     // U, E0, E1, R, W, words
  return 6 * p.L * 16 + w_bytes(p, ms) + ms * p.n_words * 4;
}
int64_t staging_bytes(const MskParams& p, int64_t ms) {
  return std::max<int64_t>(ms * p.n * 8, 8) + ms * (p.n_bits / 8 + 1) + 2 * ms * 8;
}
int64_t seg_bytes(const MskParams& p, int64_t ms) { return std::max<int64_t>(ms * msk_acq_segments(p.n) * 32, 32); }
// what the bit-timing group holds: the segments' sums, q and the offsets
int64_t acq_bytes(const MskParams& p, int64_t ms) { return seg_bytes(p, ms) + ms * 16 + ms * 8; }

// the bit-timing kernels of one batch on the plan's stream, into q / mem.off; the
// group is allocated on the first acquiring call (all or nothing)
int run_acquire(amr_msk_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride) {
  const int64_t ms = pl->max_streams;
  auto& m = pl->mem;
  HIP_TRY((reserve_all({{m.own[kSeg], seg_bytes(pl->p, ms)}, {m.own[kQ], ms * 16}, {m.off, ms * 8}}, pl->stream)));
  return timed(*pl, AMR_TD_ACQUIRE, [&]() -> int {
    HIP_TRY(launch_msk_lines(d_x, dtype, x_stride, B, pl->p, m.own[kE0].as<double>(), m.own[kE1].as<double>(),
                             m.own[kSeg].as<double>(), pl->stream));
    HIP_TRY(launch_msk_acq_max(pl->p.L, msk_acq_segments(pl->p.n), B, m.own[kSeg].as<double>(),
                               m.own[kR].as<double>(), m.off.as<int64_t>(), m.own[kQ].as<double>(), pl->stream));
    return AMR_OK;
  });
}

// One batch on the plan's stream (device pointers; the caller holds mu and has
// set the device).  soft: non-null, k_msk_soft behind the sync search.
// acquire: the streams' offsets first (run_acquire), the correlator at them;
// d_offset (device, or null) receives them, zeros when nothing was acquired.
int run_msk(amr_msk_plan* pl, const DemodIo& io, int8_t* soft, int64_t soft_stride, bool acquire,
            int64_t* d_offset) {
  if (int rc = check_demod_args(pl, io, ArgOrder::device)) return rc;
  core_clear_used(*pl);
  if (io.B == 0) return AMR_OK;
  const MskParams& p = pl->p;
  hipStream_t st = pl->stream;
  return timed(*pl, AMR_TD_LAUNCH, [&]() -> int {
    if (acquire) {
      if (int rc = run_acquire(pl, io.x, io.dtype, io.B, io.x_stride)) return rc;
      if (d_offset)
        HIP_TRY(hipMemcpyAsync(d_offset, pl->mem.off.get(), (size_t)io.B * 8, hipMemcpyDeviceToDevice, st));
    } else if (d_offset) {
      HIP_TRY(hipMemsetAsync(d_offset, 0, (size_t)io.B * 8, st));
    }
    if (p.n_sym < 2) {                               // fewer than two windows: b"", sync -1
      HIP_TRY(hipMemsetAsync(io.len, 0, (size_t)io.B * 8, st));
      HIP_TRY(hipMemsetAsync(io.sync, 0xFF, (size_t)io.B * 8, st));
      return AMR_OK;
    }
    double* W = pl->mem.Y.as<double>();
    uint32_t* words = pl->mem.words.as<uint32_t>();
    HIP_TRY_TIMED(*pl, AMR_TD_DESPREAD,
                  launch_msk_corr(io.x, io.dtype, io.x_stride, io.B, p, pl->mem.own[kU].as<double>(),
                                  acquire ? pl->mem.off.as<int64_t>() : nullptr, W, st));
    HIP_TRY_TIMED(*pl, AMR_TD_SLICE, launch_msk_slice(W, io.B, p, words, st));
    return timed(*pl, AMR_TD_SYNC_PACK, [&]() -> int {
      HIP_TRY(launch_sync_pack(words, p.n_words, p.n_bits, io.B, io.out, io.out_stride, io.len, io.sync, st));
      if (soft) HIP_TRY(launch_msk_soft(W, io.B, p, words, io.sync, io.len, soft, soft_stride, st));
      return AMR_OK;
    });
  });
}

// amr_msk_acquire_host / _device (sym_plan.h acquire_entry): the offsets and q
int msk_acquire_entry(amr_msk_plan* plan, const char* who, bool host, const void* x, int dtype, int64_t B,
                      int64_t x_stride, int64_t* offset, double* q) {
  if (!plan) return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  return acquire_entry(plan, who, host, x, dtype, B, x_stride, offset, {{q, &plan->mem.own[kQ], 16}},
                       [&](const void* d_x, int64_t stride) { return run_acquire(plan, d_x, dtype, B, stride); });
}

// the stage entries: k_msk_slice on given W (the words to `words`, or null), with `soft` k_msk_soft
int msk_symbol_stages(const char* who, const double* W, int64_t n_streams, int64_t n_win, int64_t cyc4,
                      uint32_t* words, int8_t* soft) {
  if (cyc4 < 0) return fail(AMR_E_INVALID, std::string(who) + ": bad argument");
  MskParams p{};
  p.cyc4 = cyc4;
  return symbol_stages(
      who, p, 1, 1, W, n_streams, n_win, words, soft,
      [&](const double* y, const MskParams& q, uint32_t* w) { return launch_msk_slice(y, n_streams, q, w, nullptr); },
      [&](const double* y, const MskParams& q, const uint32_t* w, int8_t* s) {
        return launch_msk_soft(y, n_streams, q, w, nullptr, nullptr, s, q.n_bits, nullptr);
      });
}

}  // namespace

extern "C" {

int amr_msk_plan_create(amr_msk_plan** out, int device, int64_t n_samples, int64_t L, int64_t cyc4, const double* U,
                        const double* E0, const double* E1, const double* R, int64_t max_streams) {
  if (!out || !U || !E0 || !E1 || !R) return fail(AMR_E_INVALID, "amr_msk_plan_create: NULL argument");
  *out = nullptr;
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_msk_plan_create: max_streams < 1");
  MskParams p;
  if (int rc = msk_params(n_samples, L, cyc4, &p)) return rc;
  auto* pl = new amr_msk_plan();
  pl->p = p;
  auto& m = pl->mem;
  return sym_plan_setup(pl, device, max_streams,
                        {{&m.own[kU], p.L * 16, U},
                         {&m.own[kE0], 2 * p.L * 16, E0},
                         {&m.own[kE1], 2 * p.L * 16, E1},
                         {&m.own[kR], p.L * 16, R},
                         {&m.Y, w_bytes(p, max_streams), nullptr},
                         {&m.words, max_streams * p.n_words * 4, nullptr}},
                        out);
}

int amr_msk_plan_destroy(amr_msk_plan* plan) {
  sym_plan_free(plan);
  return AMR_OK;
}

int amr_msk_plan_synchronize(amr_msk_plan* plan) { return sym_plan_synchronize(plan); }
int amr_msk_plan_enable_timing(amr_msk_plan* plan, int on) { return sym_plan_enable_timing(plan, on); }
int amr_msk_plan_timings(amr_msk_plan* plan, float* ms, int count) { return sym_plan_timings(plan, ms, count); }
int64_t amr_msk_plan_out_capacity(const amr_msk_plan* plan) { return plan ? plan->out_cap : -1; }
int64_t amr_msk_plan_scratch_bytes(const amr_msk_plan* plan) { return plan ? plan->mem.bytes() : -1; }

int64_t amr_msk_plan_bytes_estimate(int64_t n_samples, int64_t L, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_msk_plan_bytes_estimate: max_streams < 1");
  MskParams p;
  // the byte counts depend on L alone; two quarter-cycles per bit are valid wherever any carrier is (L >= 4)
  if (int rc = msk_params(n_samples, L, 2, &p)) return rc;
  return plan_bytes(p, max_streams) + staging_bytes(p, max_streams);
}

int64_t amr_msk_acquire_bytes_estimate(int64_t n_samples, int64_t L, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_msk_acquire_bytes_estimate: max_streams < 1");
  MskParams p;
  if (int rc = msk_params(n_samples, L, 2, &p)) return rc;
  return acq_bytes(p, max_streams);
}

int amr_msk_demod_device(amr_msk_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                         uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx, int8_t* d_soft,
                         int64_t soft_stride, int64_t* d_offset, int acquire) {
  if (int rc = demod_precheck(plan, "amr_msk_demod_device", kCapFn, n_streams, x_stride, out_stride,
                              d_soft != nullptr, soft_stride))
    return rc;
  if (n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx))
    return fail(AMR_E_INVALID, "amr_msk_demod_device: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_msk(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx}, d_soft,
                 soft_stride, acquire != 0, d_offset);
}

int amr_msk_demod_host(amr_msk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, uint8_t* out,
                       int64_t out_stride, int64_t* out_len, int64_t* sync_idx, int8_t* soft, int64_t soft_stride,
                       int64_t* offset, int acquire) {
  if (int rc = demod_precheck(plan, "amr_msk_demod_host", kCapFn, B, x_stride, out_stride, soft != nullptr,
                              soft_stride))
    return rc;
  return demod_host(plan, "amr_msk_demod_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx}, soft,
                    soft_stride, offset, acquire != 0, [&](const DemodIo& d, int8_t* d_soft, int64_t sv) {
                      return run_msk(plan, d, d_soft, sv, acquire != 0, nullptr);
                    });
}

int amr_msk_acquire_host(amr_msk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, int64_t* offset,
                         double* q) {
  return msk_acquire_entry(plan, "amr_msk_acquire_host", true, x, dtype, B, x_stride, offset, q);
}

int amr_msk_acquire_device(amr_msk_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                           int64_t* d_offset, double* d_q) {
  return msk_acquire_entry(plan, "amr_msk_acquire_device", false, d_x, dtype, n_streams, x_stride, d_offset, d_q);
}

int amr_msk_symbols_at_host(amr_msk_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                            const int64_t* offset, double* W) {
  if (!plan || (B && (!x || !offset || !W))) return fail(AMR_E_INVALID, "amr_msk_symbols_at_host: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (int rc = batch_check(plan, dtype, B, x_stride)) return rc;
  const MskParams& p = plan->p;
  for (int64_t i = 0; i < B; ++i)
    if (offset[i] < 0 || offset[i] > p.L - 1)
      return fail(AMR_E_INVALID, "amr_msk_symbols_at_host: offset outside [0, L - 1]");
  return symbols_round_trip(plan, x, dtype, B, x_stride, offset, W, B * p.n_sym * 16,
                            [&](const void* d_x, const int64_t* d_off) {
                              return launch_msk_corr(d_x, dtype, p.n, B, p, plan->mem.own[kU].as<double>(), d_off,
                                                     plan->mem.Y.as<double>(), plan->stream);
                            });
}

int amr_msk_offset_host(int64_t L, const double* R, const double* c, int64_t n_streams, int64_t* offset, double* q) {
  constexpr const char* who = "amr_msk_offset_host";
  if (n_streams < 0 || !R || (n_streams && (!c || !offset)))
    return fail(AMR_E_INVALID, "amr_msk_offset_host: bad argument");
  if (int rc = msk_geometry(L, 2)) return rc;
  if (n_streams == 0) return AMR_OK;
  const auto bad = hip_fail_as(who);
  DevBuf d_r, d_c, d_off, d_q;
  HIP_TRY_ELSE(d_r.reserve(L * 16, nullptr), bad);
  HIP_TRY_ELSE(d_c.reserve(n_streams * 32, nullptr), bad);
  HIP_TRY_ELSE(d_off.reserve(n_streams * 8, nullptr), bad);
  HIP_TRY_ELSE(d_q.reserve(n_streams * 16, nullptr), bad);
  HIP_TRY_ELSE(hipMemcpy(d_r.get(), R, (size_t)L * 16, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(hipMemcpy(d_c.get(), c, (size_t)n_streams * 32, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(launch_msk_acq_max(L, 1, n_streams, d_c.as<double>(), d_r.as<double>(), d_off.as<int64_t>(),
                                  d_q.as<double>(), nullptr),
               bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  HIP_TRY_ELSE(hipMemcpy(offset, d_off.get(), (size_t)n_streams * 8, hipMemcpyDeviceToHost), bad);
  if (q) HIP_TRY_ELSE(hipMemcpy(q, d_q.get(), (size_t)n_streams * 16, hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

int amr_msk_slice_host(const double* W, int64_t n_streams, int64_t n_win, int64_t cyc4, uint32_t* words) {
  if (n_streams > 0 && n_win > 0 && !words) return fail(AMR_E_INVALID, "amr_msk_slice_host: bad argument");
  return msk_symbol_stages("amr_msk_slice_host", W, n_streams, n_win, cyc4, words, nullptr);
}

int amr_msk_soft_host(const double* W, int64_t n_streams, int64_t n_win, int64_t cyc4, int8_t* soft) {
  if (n_streams > 0 && n_win > 0 && !soft) return fail(AMR_E_INVALID, "amr_msk_soft_host: bad argument");
  return msk_symbol_stages("amr_msk_soft_host", W, n_streams, n_win, cyc4, nullptr, soft);
}

int amr_msk_modulate_host(int64_t L, int64_t cyc4, const double* Sn, const uint8_t* data, int64_t data_stride,
                          const int64_t* n_bytes, int64_t n, float* out, int64_t out_stride, int64_t n_out,
                          int16_t* pcm, int64_t pcm_stride) {
  constexpr const char* who = "amr_msk_modulate_host";
  if (n < 0 || n_out < 0 || data_stride < 0 || out_stride < n_out || (pcm && pcm_stride < n_out))
    return fail(AMR_E_INVALID, "amr_msk_modulate_host: bad argument");
  if (!Sn) return fail(AMR_E_INVALID, "amr_msk_modulate_host: NULL table");
  if (n && (!n_bytes || (n_out && !out))) return fail(AMR_E_INVALID, "amr_msk_modulate_host: NULL buffer");
  if (int rc = msk_geometry(L, cyc4)) return rc;
  MskTx t{};
  t.L = L;
  t.cyc4 = cyc4;
  t.n_out = n_out;
  if (n > 65535) return fail(AMR_E_INVALID, "amr_msk_modulate_host: at most 65535 streams per call");
  if (n_out > 0x7fffffffLL) return fail(AMR_E_INVALID, "amr_msk_modulate_host: n_out >= 2^31");
  t.bit_stride = (n_out + L - 1) / L;
  DevBuf d_sn, d_quad;                             // freed after the round trip has drained the device
  return modulate_round_trip(who, data, data_stride, n_bytes, n, out, out_stride, n_out, pcm, pcm_stride,
                             [&](const TxDev& d) -> int {
    const auto bad = hip_fail_as(who);
    HIP_TRY_ELSE(d_sn.reserve(4 * L * 8, nullptr), bad);
    HIP_TRY_ELSE(d_quad.reserve(n * t.bit_stride, nullptr), bad);
    HIP_TRY_ELSE(hipMemcpy(d_sn.get(), Sn, (size_t)(4 * L) * 8, hipMemcpyHostToDevice), bad);
    HIP_TRY_ELSE(launch_msk_tx(t, d_sn.as<double>(), d.data, d.stride, d.n_bytes, n, d_quad.as<uint8_t>(), d.out,
                               n_out, d.pcm, n_out, nullptr),
                 bad);
    return AMR_OK;
  });
}

}  // extern "C"
