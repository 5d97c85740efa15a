// tone8_api.cpp -- C ABI of tone8, the 8-FSK modem with Costas sync
// (include/amr.h): amr_tone8_plan on sym_plan.h's shared host
// core, the demodulation entries in the minshift entries' shape (soft values,
// start, shift and acquisition optional), the stage entries the tests pin the
// kernels with, and the modulator.  Here: the geometry, run_tone8 and each
// entry's own checks.  The kernels are tone8_kernels.hip and
// tone8_acq_kernels.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "sym_plan.h"
#include "tone8.h"
#include "tx_host.h"

using namespace amr;

namespace {
// the plan's own buffers: the table E [2 L][2]; acquisition, one group with mem.off (the starts) from the
// first acquiring call on: cand [ms][chunks], shift [ms], score [ms]
enum { kE, kCand, kShift, kScore, kTone8Bufs };
}  // namespace

struct amr_tone8_plan : SymPlan<AMR_TD_COUNT, kTone8Bufs> {
  Tone8Params p{};
};

namespace {

constexpr const char* kCapFn = "amr_tone8_plan_out_capacity";

// the geometry of include/amr.h; an AMR_E_INVALID (message set) when it is not valid
int tone8_geometry(int64_t L, int64_t c2, int64_t G) {
  if (G < 0 || G > kTone8MaxSearch) return fail(AMR_E_INVALID, "tone8: search outside [0, 16]");
  if (L < 8 || L % 8 != 0) return fail(AMR_E_INVALID, "tone8: samples per symbol not a positive multiple of 8");
  if (L > (1 << 24)) return fail(AMR_E_INVALID, "tone8: samples per symbol out of range (> 2^24)");
  if (c2 - G < 2) return fail(AMR_E_INVALID, "tone8: the lowest searched line below one carrier cycle per symbol");
  if (c2 + 14 + G >= L) return fail(AMR_E_INVALID, "tone8: the highest searched line at or above half the sample rate");
  return AMR_OK;
}

int tone8_params(int64_t n, int64_t L, int64_t c2, int64_t G, Tone8Params* p) {
  if (n < 0) return fail(AMR_E_INVALID, "tone8: n_samples < 0");
  if (int rc = tone8_geometry(L, c2, G)) return rc;
  *p = Tone8Params{};
  p->n = n;
  p->L = L;
  p->c2 = c2;
  p->G = G;
  tone8_counts(*p);
  return AMR_OK;
}

// the least (c2, G = 0) valid wherever any geometry of L is: the byte counts depend on L and G alone
int tone8_size_params(int64_t n, int64_t L, int64_t G, Tone8Params* p) {
  if (G < 0 || G > kTone8MaxSearch) return fail(AMR_E_INVALID, "tone8: search outside [0, 16]");
  if (int rc = tone8_params(n, L, 2, 0, p)) return rc;
  p->G = G;
  tone8_counts(*p);
  return AMR_OK;
}

int64_t y_bytes(const Tone8Params& p, int64_t streams) { return std::max<int64_t>(streams * p.n_sym * 128, 16); }
int64_t plan_bytes(const Tone8Params& p, int64_t ms) {   // E, Y, words
  return 2 * p.L * 16 + y_bytes(p, ms) + ms * p.n_words * 4;
}
int64_t staging_bytes(const Tone8Params& p, int64_t ms) {
  return std::max<int64_t>(ms * p.n * 8, 8) + ms * (p.n_bits / 8 + 1) + 2 * ms * 8;
}
int64_t cand_bytes(const Tone8Params& p, int64_t ms) {
  return std::max<int64_t>(ms * tone8_acq_chunks(p) * (int64_t)sizeof(Tone8Cand), 32);
}
// what the acquisition group holds: the chunks' maxima, the shifts, the scores and the starts
int64_t acq_bytes(const Tone8Params& p, int64_t ms) { return cand_bytes(p, ms) + 3 * ms * 8; }

// the acquisition kernels of one batch on the plan's stream, into mem.off / shift / score; the
// group is allocated on the first acquiring call (all or nothing)
int run_acquire(amr_tone8_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride) {
  const int64_t ms = pl->max_streams;
  auto& m = pl->mem;
  HIP_TRY((reserve_all({{m.own[kCand], cand_bytes(pl->p, ms)}, {m.own[kShift], ms * 8}, {m.own[kScore], ms * 8},
                        {m.off, ms * 8}},
                       pl->stream)));
  return timed(*pl, AMR_TD_ACQUIRE, [&]() -> int {
    HIP_TRY(launch_tone8_acquire(d_x, dtype, x_stride, B, pl->p, m.own[kE].as<double>(), m.own[kCand].as<Tone8Cand>(),
                                 m.off.as<int64_t>(), m.own[kShift].as<int64_t>(), m.own[kScore].as<double>(),
                                 pl->stream));
    return AMR_OK;
  });
}

// One batch on the plan's stream (device pointers; the caller holds mu and has
// set the device).  soft: non-null, k_tone8_soft behind the sync search.
// acquire: the streams' (start, shift) first (run_acquire), the DFT at them;
// d_start / d_shift (device, or null) receive them, zeros when nothing was acquired.
int run_tone8(amr_tone8_plan* pl, const DemodIo& io, int8_t* soft, int64_t soft_stride, bool acquire,
              int64_t* d_start, int64_t* d_shift) {
  if (int rc = check_demod_args(pl, io, ArgOrder::device)) return rc;
  core_clear_used(*pl);
  if (io.B == 0) return AMR_OK;
  const Tone8Params& p = pl->p;
  hipStream_t st = pl->stream;
  auto& m = pl->mem;
  return timed(*pl, AMR_TD_LAUNCH, [&]() -> int {
    if (acquire) {
      if (int rc = run_acquire(pl, io.x, io.dtype, io.B, io.x_stride)) return rc;
      if (d_start) HIP_TRY(hipMemcpyAsync(d_start, m.off.get(), (size_t)io.B * 8, hipMemcpyDeviceToDevice, st));
      if (d_shift)
        HIP_TRY(hipMemcpyAsync(d_shift, m.own[kShift].get(), (size_t)io.B * 8, hipMemcpyDeviceToDevice, st));
    } else {
      if (d_start) HIP_TRY(hipMemsetAsync(d_start, 0, (size_t)io.B * 8, st));
      if (d_shift) HIP_TRY(hipMemsetAsync(d_shift, 0, (size_t)io.B * 8, st));
    }
    if (p.n_sym < 1) {                               // no symbol: b"", sync -1
      HIP_TRY(hipMemsetAsync(io.len, 0, (size_t)io.B * 8, st));
      HIP_TRY(hipMemsetAsync(io.sync, 0xFF, (size_t)io.B * 8, st));
      return AMR_OK;
    }
    double* Y = m.Y.as<double>();
    uint32_t* words = m.words.as<uint32_t>();
    HIP_TRY_TIMED(*pl, AMR_TD_DESPREAD,
                  launch_tone8_dft(io.x, io.dtype, io.x_stride, io.B, p, m.own[kE].as<double>(),
                                   acquire ? m.off.as<int64_t>() : nullptr,
                                   acquire ? m.own[kShift].as<int64_t>() : nullptr, Y, st));
    HIP_TRY_TIMED(*pl, AMR_TD_SLICE, launch_tone8_slice(Y, io.B, p, words, st));
    return timed(*pl, AMR_TD_SYNC_PACK, [&]() -> int {
      HIP_TRY(launch_sync_pack(words, p.n_words, p.n_bits, io.B, io.out, io.out_stride, io.len, io.sync, st));
      if (soft) HIP_TRY(launch_tone8_soft(Y, io.B, p, words, io.sync, io.len, soft, soft_stride, st));
      return AMR_OK;
    });
  });
}

// amr_tone8_acquire_host / _device (sym_plan.h acquire_entry): the starts, shifts and scores
int tone8_acquire_entry(amr_tone8_plan* plan, const char* who, bool host, const void* x, int dtype, int64_t B,
                        int64_t x_stride, int64_t* start, int64_t* shift, double* score) {
  if (!plan || (B && !shift)) return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  return acquire_entry(plan, who, host, x, dtype, B, x_stride, start,
                       {{shift, &plan->mem.own[kShift], 8}, {score, &plan->mem.own[kScore], 8}},
                       [&](const void* d_x, int64_t stride) { return run_acquire(plan, d_x, dtype, B, stride); });
}

// the stage entries: k_tone8_slice on given Y (the words to `words`, or null), with `soft` k_tone8_soft
int tone8_symbol_stages(const char* who, const double* Y, int64_t n_streams, int64_t n_sym, uint32_t* words,
                        int8_t* soft) {
  Tone8Params p{};
  return symbol_stages(
      who, p, 8, 3, Y, n_streams, n_sym, words, soft,
      [&](const double* y, const Tone8Params& q, uint32_t* w) { return launch_tone8_slice(y, n_streams, q, w, nullptr); },
      [&](const double* y, const Tone8Params& q, const uint32_t* w, int8_t* s) {
        return launch_tone8_soft(y, n_streams, q, w, nullptr, nullptr, s, q.n_bits, nullptr);
      },
      0);
}

}  // namespace

extern "C" {

int64_t amr_tone8_chunk(int64_t search) {
  if (search < 0 || search > kTone8MaxSearch) return fail(AMR_E_INVALID, "amr_tone8_chunk: search outside [0, 16]");
  return tone8_chunk(search);
}

int amr_tone8_plan_create(amr_tone8_plan** out, int device, int64_t n_samples, int64_t L, int64_t c2, int64_t search,
                          const double* E, int64_t max_streams) {
  if (!out || !E) return fail(AMR_E_INVALID, "amr_tone8_plan_create: NULL argument");
  *out = nullptr;
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_tone8_plan_create: max_streams < 1");
  Tone8Params p;
  if (int rc = tone8_params(n_samples, L, c2, search, &p)) return rc;
  auto* pl = new amr_tone8_plan();
  pl->p = p;
  auto& m = pl->mem;
  return sym_plan_setup(pl, device, max_streams,
                        {{&m.own[kE], 2 * p.L * 16, E},
                         {&m.Y, y_bytes(p, max_streams), nullptr},
                         {&m.words, max_streams * p.n_words * 4, nullptr}},
                        out);
}

int amr_tone8_plan_destroy(amr_tone8_plan* plan) {
  sym_plan_free(plan);
  return AMR_OK;
}

int amr_tone8_plan_synchronize(amr_tone8_plan* plan) { return sym_plan_synchronize(plan); }
int amr_tone8_plan_enable_timing(amr_tone8_plan* plan, int on) { return sym_plan_enable_timing(plan, on); }
int amr_tone8_plan_timings(amr_tone8_plan* plan, float* ms, int count) { return sym_plan_timings(plan, ms, count); }
int64_t amr_tone8_plan_out_capacity(const amr_tone8_plan* plan) { return plan ? plan->out_cap : -1; }
int64_t amr_tone8_plan_scratch_bytes(const amr_tone8_plan* plan) { return plan ? plan->mem.bytes() : -1; }

int64_t amr_tone8_plan_bytes_estimate(int64_t n_samples, int64_t L, int64_t search, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_tone8_plan_bytes_estimate: max_streams < 1");
  Tone8Params p;
  if (int rc = tone8_size_params(n_samples, L, search, &p)) return rc;
  return plan_bytes(p, max_streams) + staging_bytes(p, max_streams);
}

int64_t amr_tone8_acquire_bytes_estimate(int64_t n_samples, int64_t L, int64_t search, int64_t max_streams) {
  if (max_streams < 1) return fail(AMR_E_INVALID, "amr_tone8_acquire_bytes_estimate: max_streams < 1");
  Tone8Params p;
  if (int rc = tone8_size_params(n_samples, L, search, &p)) return rc;
  return acq_bytes(p, max_streams);
}

int amr_tone8_demod_device(amr_tone8_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                           uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx, int8_t* d_soft,
                           int64_t soft_stride, int64_t* d_start, int64_t* d_shift, int acquire) {
  if (int rc = demod_precheck(plan, "amr_tone8_demod_device", kCapFn, n_streams, x_stride, out_stride,
                              d_soft != nullptr, soft_stride))
    return rc;
  if (n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx))
    return fail(AMR_E_INVALID, "amr_tone8_demod_device: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  return run_tone8(plan, {d_x, dtype, n_streams, x_stride, d_out, out_stride, d_out_len, d_sync_idx}, d_soft,
                   soft_stride, acquire != 0, d_start, d_shift);
}

int amr_tone8_demod_host(amr_tone8_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, uint8_t* out,
                         int64_t out_stride, int64_t* out_len, int64_t* sync_idx, int8_t* soft, int64_t soft_stride,
                         int64_t* start, int64_t* shift, int acquire) {
  if (int rc = demod_precheck(plan, "amr_tone8_demod_host", kCapFn, B, x_stride, out_stride, soft != nullptr,
                              soft_stride))
    return rc;
  return demod_host(plan, "amr_tone8_demod_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx}, soft,
                    soft_stride, start, acquire != 0, [&](const DemodIo& d, int8_t* d_soft, int64_t sv) -> int {
                      if (int rc = run_tone8(plan, d, d_soft, sv, acquire != 0, nullptr, nullptr)) return rc;
                      // queued like the round trip's own downloads, which wait for the stream
                      if (shift && acquire)
                        HIP_TRY(hipMemcpyAsync(shift, plan->mem.own[kShift].get(), (size_t)B * 8,
                                               hipMemcpyDeviceToHost, plan->stream));
                      if (shift && !acquire) std::memset(shift, 0, (size_t)B * 8);
                      return AMR_OK;
                    });
}

int amr_tone8_acquire_host(amr_tone8_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, int64_t* start,
                           int64_t* shift, double* score) {
  return tone8_acquire_entry(plan, "amr_tone8_acquire_host", true, x, dtype, B, x_stride, start, shift, score);
}

int amr_tone8_acquire_device(amr_tone8_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                             int64_t* d_start, int64_t* d_shift, double* d_score) {
  return tone8_acquire_entry(plan, "amr_tone8_acquire_device", false, d_x, dtype, n_streams, x_stride, d_start,
                             d_shift, d_score);
}

int amr_tone8_symbols_at_host(amr_tone8_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                              const int64_t* offset, const int64_t* shift, double* Y) {
  if (!plan || (B && (!x || !offset || !shift || !Y)))
    return fail(AMR_E_INVALID, "amr_tone8_symbols_at_host: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (int rc = batch_check(plan, dtype, B, x_stride)) return rc;
  const Tone8Params& p = plan->p;
  for (int64_t i = 0; i < B; ++i) {
    if (offset[i] < 0 || offset[i] > p.L - 1)
      return fail(AMR_E_INVALID, "amr_tone8_symbols_at_host: offset outside [0, L - 1]");
    if (shift[i] < -p.G || shift[i] > p.G)
      return fail(AMR_E_INVALID, "amr_tone8_symbols_at_host: shift outside [-search, search]");
  }
  DevBuf d_shift;                                  // this call's own; the round trip drains the stream before it goes
  if (B && p.n_sym) {
    HIP_TRY(hipSetDevice(plan->device));
    HIP_TRY(d_shift.reserve(B * 8, nullptr));
    HIP_TRY(hipMemcpy(d_shift.get(), shift, (size_t)B * 8, hipMemcpyHostToDevice));
  }
  return symbols_round_trip(plan, x, dtype, B, x_stride, offset, Y, B * p.n_sym * 128,
                            [&](const void* d_x, const int64_t* d_off) {
                              return launch_tone8_dft(d_x, dtype, p.n, B, p, plan->mem.own[kE].as<double>(), d_off,
                                                      d_shift.as<int64_t>(), plan->mem.Y.as<double>(), plan->stream);
                            });
}

int amr_tone8_peak_host(int64_t T, int64_t search, const double* P, int64_t n_streams, int64_t n_win, int64_t* start,
                        int64_t* shift, double* score) {
  constexpr const char* who = "amr_tone8_peak_host";
  if (n_streams < 0 || n_win < 0 || T < 1 || search < 0 || search > kTone8MaxSearch ||
      (n_streams && (!start || !shift || (n_win && !P))))
    return fail(AMR_E_INVALID, "amr_tone8_peak_host: bad argument");
  if (n_streams == 0) return AMR_OK;
  const auto bad = hip_fail_as(who);
  const int64_t NB = tone8_lines(search), C = tone8_chunk(search);
  const int64_t nj = n_win > kTone8Span ? n_win - kTone8Span : 0;
  const int64_t pb = n_streams * n_win * NB * 8;
  DevBuf d_p, d_cand, d_start, d_shift, d_score;
  HIP_TRY_ELSE(d_p.reserve(std::max<int64_t>(pb, 8), nullptr), bad);
  HIP_TRY_ELSE(d_cand.reserve(std::max<int64_t>(n_streams * ((nj + C - 1) / C) * (int64_t)sizeof(Tone8Cand), 32), nullptr),
               bad);
  HIP_TRY_ELSE(d_start.reserve(n_streams * 8, nullptr), bad);
  HIP_TRY_ELSE(d_shift.reserve(n_streams * 8, nullptr), bad);
  HIP_TRY_ELSE(d_score.reserve(n_streams * 8, nullptr), bad);
  if (pb) HIP_TRY_ELSE(hipMemcpy(d_p.get(), P, (size_t)pb, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(launch_tone8_peak(d_p.as<double>(), n_streams, n_win, T, search, d_cand.as<Tone8Cand>(),
                                 d_start.as<int64_t>(), d_shift.as<int64_t>(), d_score.as<double>(), nullptr),
               bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  HIP_TRY_ELSE(hipMemcpy(start, d_start.get(), (size_t)n_streams * 8, hipMemcpyDeviceToHost), bad);
  HIP_TRY_ELSE(hipMemcpy(shift, d_shift.get(), (size_t)n_streams * 8, hipMemcpyDeviceToHost), bad);
  if (score) HIP_TRY_ELSE(hipMemcpy(score, d_score.get(), (size_t)n_streams * 8, hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

int amr_tone8_slice_host(const double* Y, int64_t n_streams, int64_t n_sym, uint32_t* words) {
  if (n_streams > 0 && n_sym > 0 && !words) return fail(AMR_E_INVALID, "amr_tone8_slice_host: bad argument");
  return tone8_symbol_stages("amr_tone8_slice_host", Y, n_streams, n_sym, words, nullptr);
}

int amr_tone8_soft_host(const double* Y, int64_t n_streams, int64_t n_sym, int8_t* soft) {
  if (n_streams > 0 && n_sym > 0 && !soft) return fail(AMR_E_INVALID, "amr_tone8_soft_host: bad argument");
  return tone8_symbol_stages("amr_tone8_soft_host", Y, n_streams, n_sym, nullptr, soft);
}

int amr_tone8_modulate_host(int64_t L, int64_t c2, const double* Sn, const uint8_t* data, int64_t data_stride,
                            const int64_t* n_bytes, int64_t n, float* out, int64_t out_stride, int64_t n_out,
                            int16_t* pcm, int64_t pcm_stride) {
  constexpr const char* who = "amr_tone8_modulate_host";
  if (n < 0 || n_out < 0 || data_stride < 0 || out_stride < n_out || (pcm && pcm_stride < n_out))
    return fail(AMR_E_INVALID, "amr_tone8_modulate_host: bad argument");
  if (!Sn) return fail(AMR_E_INVALID, "amr_tone8_modulate_host: NULL table");
  if (n && (!n_bytes || (n_out && !out))) return fail(AMR_E_INVALID, "amr_tone8_modulate_host: NULL buffer");
  if (int rc = tone8_geometry(L, c2, 0)) return rc;
  Tone8Tx t{};
  t.L = L;
  t.c2 = c2;
  t.n_out = n_out;
  if (n > 65535) return fail(AMR_E_INVALID, "amr_tone8_modulate_host: at most 65535 streams per call");
  if (n_out > 0x7fffffffLL) return fail(AMR_E_INVALID, "amr_tone8_modulate_host: n_out >= 2^31");
  t.sym_stride = (n_out + L - 1) / L;
  DevBuf d_sn, d_ph;                               // freed after the round trip has drained the device
  return modulate_round_trip(who, data, data_stride, n_bytes, n, out, out_stride, n_out, pcm, pcm_stride,
                             [&](const TxDev& d) -> int {
    const auto bad = hip_fail_as(who);
    HIP_TRY_ELSE(d_sn.reserve(2 * L * 8, nullptr), bad);
    HIP_TRY_ELSE(d_ph.reserve(n * t.sym_stride * 4, nullptr), bad);
    HIP_TRY_ELSE(hipMemcpy(d_sn.get(), Sn, (size_t)(2 * L) * 8, hipMemcpyHostToDevice), bad);
    HIP_TRY_ELSE(launch_tone8_tx(t, d_sn.as<double>(), d.data, d.stride, d.n_bytes, n, d_ph.as<uint32_t>(), d.out,
                                 n_out, d.pcm, n_out, nullptr),
                 bad);
    return AMR_OK;
  });
}

}  // extern "C"
