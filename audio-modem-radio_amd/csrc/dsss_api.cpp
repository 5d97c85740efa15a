// dsss_api.cpp -- C ABI of spread, the direct-sequence DBPSK modem
// (include/amr.h): amr_dsss_plan on PlanCore with dev_mem.h
// ownership, the demodulation entries in the PSK entries' shape (soft values,
// offsets and acquisition optional), the stage entries the tests pin the
// kernels with, and the modulator.  The kernels are dsss_kernels.hip and
// dsss_acq_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "dsss.h"
#include "plan_core.h"

namespace amr {
hipError_t launch_sync_pack(const uint32_t*, int64_t, int64_t, int64_t, uint8_t*, int64_t, int64_t*, int64_t*,
                            hipStream_t);
}  // namespace amr

using namespace amr;

struct amr_dsss_plan : PlanCore<AMR_TD_COUNT> {
  DsssParams p{};
  int64_t max_streams = 0;
  int64_t out_cap = 0;
  // every device buffer the plan owns; dsss_plan_free releases them together
  struct Mem {
    DevBuf Wc, T, cs;              // [L][2], [L][2], [C]
    DevBuf Y;                      // [max_streams][S][2]
    DevBuf words;                  // [max_streams][n_words]
    // staging for the host entries (lazily sized)
    DevBuf d_x;
    DevBuf d_out, d_len, d_sync;   // one group: all three or none (reserve_all)
    // acquisition, from the first acquiring call on: one group
    DevBuf gq, P, off;             // [ms][segments][L], [ms][L], [ms]
  } mem;
};

namespace {

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

// set device, drain the stream, drop the gather gate; then the buffers; then events and the stream
void dsss_plan_free(amr_dsss_plan* pl) {
  if (!pl) return;
  (void)hipSetDevice(pl->device);
  if (pl->stream) (void)hipStreamSynchronize(pl->stream);
  gate_free(pl->gate);
  pl->mem = amr_dsss_plan::Mem{};
  core_destroy_events(*pl);
  if (pl->stream) (void)hipStreamDestroy(pl->stream);
  delete pl;
}

// the acquisition kernels of one batch on the plan's stream, into mem.P / off; the
// group is allocated on the first acquiring call (all or nothing)
int run_acquire(amr_dsss_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride) {
  const int64_t ms = pl->max_streams, L = pl->p.L;
  amr_dsss_plan::Mem& m = pl->mem;
  HIP_TRY((reserve_all({{m.gq, std::max<int64_t>(ms * dsss_acq_segments(pl->p) * L * 8, 8)},
                        {m.P, ms * L * 8},
                        {m.off, ms * 8}},
                       pl->stream)));
  const DsssAcq a{m.gq.as<double>(), m.P.as<double>(), m.off.as<int64_t>()};
  HIP_TRY_TIMED(*pl, AMR_TD_ACQUIRE,
                launch_dsss_acquire(d_x, dtype, x_stride, B, pl->p, m.Wc.as<double>(), m.cs.as<double>(), a, pl->stream));
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
                  launch_dsss_despread(io.x, io.dtype, io.x_stride, io.B, p, pl->mem.T.as<double>(),
                                       acquire ? pl->mem.off.as<int64_t>() : nullptr, Y, st));
    HIP_TRY_TIMED(*pl, AMR_TD_SLICE, launch_dsss_slice(Y, io.B, p, words, st));
    return timed(*pl, AMR_TD_SYNC_PACK, [&]() -> int {
      HIP_TRY(launch_sync_pack(words, p.n_words, p.n_bits, io.B, io.out, io.out_stride, io.len, io.sync, st));
      if (soft) HIP_TRY(launch_dsss_soft(Y, io.B, p, words, io.sync, io.len, soft, soft_stride, st));
      return AMR_OK;
    });
  });
}

int dsss_host_staging(amr_dsss_plan* pl) {
  const int64_t ms = pl->max_streams;
  HIP_TRY(pl->mem.d_x.reserve(std::max<int64_t>(ms * pl->p.n * 8, 8), pl->stream));
  HIP_TRY((reserve_all({{pl->mem.d_out, ms * pl->out_cap}, {pl->mem.d_len, ms * 8}, {pl->mem.d_sync, ms * 8}},
                       pl->stream)));
  return AMR_OK;
}

// the checks the soft entries make before the shared contract, `soft` optional here
int demod_precheck(const amr_dsss_plan* plan, const char* who, int64_t B, int64_t x_stride, int64_t out_stride,
                   const int8_t* soft, int64_t soft_stride) {
  const std::string name(who);
  if (B < 0 || x_stride < 0 || out_stride < 0 || (soft && soft_stride < 0))
    return fail(AMR_E_INVALID, name + ": negative argument");
  if (!plan) return fail(AMR_E_INVALID, name + ": NULL argument");
  if (soft && soft_stride < 8 * plan->out_cap)
    return fail(AMR_E_INVALID, name + ": soft_stride < 8 * amr_dsss_plan_out_capacity()");
  return AMR_OK;
}

// the checks of an entry that reads a batch of x outside the demod contract
int batch_check(const amr_dsss_plan* plan, int dtype, int64_t B, int64_t x_stride) {
  if (dtype_size(dtype) == 0) return fail(AMR_E_INVALID, "unknown dtype");
  if (B < 0 || B > plan->max_streams) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < plan->p.n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  return AMR_OK;
}

// amr_dsss_acquire_host / _device: the acquisition stage alone.  host: x, offset and P are host memory
// (x staged in mem.d_x, the call waits); else device memory, the copies queued on the plan's stream.
int dsss_acquire_entry(amr_dsss_plan* plan, const char* who, bool host, const void* x, int dtype, int64_t B,
                       int64_t x_stride, int64_t* offset, double* P) {
  if (!plan || (B && (!x || !offset))) return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (int rc = batch_check(plan, dtype, B, x_stride)) return rc;
  const DsssParams& p = plan->p;
  const int64_t es = dtype_size(dtype), n = p.n;
  HIP_TRY(hipSetDevice(plan->device));
  core_clear_used(*plan);
  if (B == 0) return AMR_OK;
  amr_dsss_plan::Mem& m = plan->mem;
  hipStream_t st = plan->stream;
  const void* d_x = x;
  int64_t stride = x_stride;
  if (host) {
    HIP_TRY(m.d_x.reserve(std::max<int64_t>(plan->max_streams * n * 8, 8), st));
    if (n > 0)
      if (int rc = upload_batch(Copy::sync, m.d_x.get(), x, n * es, x_stride * es, B, st)) return rc;
    d_x = m.d_x.get();
    stride = n;
  }
  if (int rc = run_acquire(plan, d_x, dtype, B, stride)) return rc;
  const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIP_TRY(hipMemcpyAsync(offset, m.off.get(), (size_t)B * 8, kind, st));
  if (P) HIP_TRY(hipMemcpyAsync(P, m.P.get(), (size_t)(B * p.L) * 8, kind, st));
  if (host) HIP_TRY(hipStreamSynchronize(st));
  return AMR_OK;
}

// the stage entries: k_dsss_slice on given Y (the words to `words`, or null), with `soft` k_dsss_soft, every bit from 0
int dsss_symbol_stages(const char* who, const double* Y, int64_t n_streams, int64_t n_sym, uint32_t* words,
                       int8_t* soft) {
  const std::string name(who);
  if (n_streams < 0 || n_sym < 0 || (n_streams && n_sym && (!Y || (!words && !soft))))
    return fail(AMR_E_INVALID, name + ": bad argument");
  DsssParams p{};
  p.n_sym = n_sym;
  p.n_bits = n_sym >= 2 ? n_sym - 1 : 0;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
  if (n_streams == 0 || p.n_bits == 0) return AMR_OK;
  const auto bad = [&name](hipError_t e) { return fail(AMR_E_HIP, name + ": " + hipGetErrorString(e)); };
  const int64_t yb = n_streams * n_sym * 16;
  DevBuf d_y, d_words, d_soft;
  HIP_TRY_ELSE(d_y.reserve(yb, nullptr), bad);
  HIP_TRY_ELSE(d_words.reserve(n_streams * p.n_words * 4, nullptr), bad);
  if (soft) HIP_TRY_ELSE(d_soft.reserve(n_streams * p.n_bits, nullptr), bad);
  HIP_TRY_ELSE(hipMemcpy(d_y.get(), Y, (size_t)yb, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(launch_dsss_slice(d_y.as<double>(), n_streams, p, d_words.as<uint32_t>(), nullptr), bad);
  if (soft)
    HIP_TRY_ELSE(launch_dsss_soft(d_y.as<double>(), n_streams, p, d_words.as<uint32_t>(), nullptr, nullptr,
                                  d_soft.as<int8_t>(), p.n_bits, nullptr),
                 bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  if (words)
    HIP_TRY_ELSE(hipMemcpy(words, d_words.get(), (size_t)(n_streams * p.n_words) * 4, hipMemcpyDeviceToHost), bad);
  if (soft) HIP_TRY_ELSE(hipMemcpy(soft, d_soft.get(), (size_t)(n_streams * p.n_bits), hipMemcpyDeviceToHost), bad);
  return AMR_OK;
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
  pl->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete pl;
    return fail(AMR_E_NODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  }
  pl->p = p;
  pl->max_streams = max_streams;
  pl->out_cap = p.n_bits / 8 + 1;
  amr_dsss_plan::Mem& m = pl->mem;
  const struct { DevBuf* buf; int64_t bytes; const void* src; } allocs[] = {
      {&m.Wc, p.L * 16, Wc},          {&m.T, p.L * 16, T}, {&m.cs, (int64_t)C * 8, cs},
      {&m.Y, y_bytes(p, max_streams), nullptr}, {&m.words, max_streams * p.n_words * 4, nullptr}};
  for (const auto& a : allocs) {
    e = a.buf->reserve(a.bytes, nullptr);
    if (e != hipSuccess) {
      dsss_plan_free(pl);
      return fail(AMR_E_NOMEM, "hipMalloc(" + std::to_string(a.bytes) + " B): " + hipGetErrorString(e));
    }
    if (a.src) e = hipMemcpy(a.buf->get(), a.src, (size_t)a.bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) break;
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    dsss_plan_free(pl);
    return fail(AMR_E_HIP, std::string("plan setup: ") + hipGetErrorString(e));
  }
  *out = pl;
  return AMR_OK;
}

int amr_dsss_plan_destroy(amr_dsss_plan* plan) {
  dsss_plan_free(plan);
  return AMR_OK;
}

int amr_dsss_plan_synchronize(amr_dsss_plan* plan) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_synchronize(*plan);
}

int amr_dsss_plan_enable_timing(amr_dsss_plan* plan, int on) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_enable_timing(*plan, on);
}

int amr_dsss_plan_timings(amr_dsss_plan* plan, float* ms, int count) {
  if (!plan || !ms) return fail(AMR_E_INVALID, "NULL argument");
  return core_timings(*plan, ms, count);
}

int64_t amr_dsss_plan_out_capacity(const amr_dsss_plan* plan) { return plan ? plan->out_cap : -1; }

int64_t amr_dsss_plan_scratch_bytes(const amr_dsss_plan* plan) {
  if (!plan) return -1;
  const amr_dsss_plan::Mem& m = plan->mem;
  return m.Wc.bytes() + m.T.bytes() + m.cs.bytes() + m.Y.bytes() + m.words.bytes() + m.d_x.bytes() +
         m.d_out.bytes() + m.d_len.bytes() + m.d_sync.bytes() + m.gq.bytes() + m.P.bytes() + m.off.bytes();
}

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
  if (int rc = demod_precheck(plan, "amr_dsss_demod_device", n_streams, x_stride, out_stride, d_soft, soft_stride))
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
  if (int rc = demod_precheck(plan, "amr_dsss_demod_host", B, x_stride, out_stride, soft, soft_stride)) return rc;
  const DemodIo h{x, dtype, B, x_stride, out, out_stride, out_len, sync_idx};
  DevBuf d_soft, d_off;                          // this call's own; the round trip waits for the stream
  int64_t sv = 0;
  const int rc = host_round_trip(plan, "amr_dsss_demod_host", h, Copy::sync, [&]() -> int {
    amr_dsss_plan::Mem& m = plan->mem;
    const int64_t n = plan->p.n, es = dtype_size(h.dtype);
    if (int rc = dsss_host_staging(plan)) return rc;
    if (n > 0)
      if (int rc = upload_batch(Copy::sync, m.d_x.get(), h.x, n * es, h.x_stride * es, h.B, plan->stream)) return rc;
    const DemodIo d{m.d_x.get(), h.dtype, h.B, n, m.d_out.as<uint8_t>(), plan->out_cap, m.d_len.as<int64_t>(),
                    m.d_sync.as<int64_t>()};
    if (soft) {
      sv = std::max<int64_t>(plan->p.n_bits, 1);
      HIP_TRY(d_soft.reserve(h.B * sv, nullptr));
    }
    if (offset) HIP_TRY(d_off.reserve(h.B * 8, nullptr));
    if (int rc = run_dsss(plan, d, soft ? d_soft.as<int8_t>() : nullptr, sv, acquire != 0, d_off.as<int64_t>()))
      return rc;
    if (offset)                                // queued like the round trip's own downloads, which wait for the stream
      HIP_TRY(hipMemcpyAsync(offset, d_off.get(), (size_t)h.B * 8, hipMemcpyDeviceToHost, plan->stream));
    return AMR_OK;
  });
  if (rc || !soft || B == 0) return rc;
  // only the values of the stream's bytes reach the caller's row
  std::vector<int8_t> tmp((size_t)(B * sv));
  HIP_TRY(hipMemcpy(tmp.data(), d_soft.get(), tmp.size(), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < B; ++i)
    std::memcpy(soft + i * soft_stride, tmp.data() + i * sv, (size_t)std::min(8 * out_len[i], soft_stride));
  return AMR_OK;
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
  const int64_t es = dtype_size(dtype), n = p.n;
  for (int64_t i = 0; i < B; ++i)
    if (offset[i] < 0 || offset[i] > p.L - 1)
      return fail(AMR_E_INVALID, "amr_dsss_symbols_at_host: offset outside [0, L - 1]");
  HIP_TRY(hipSetDevice(plan->device));
  const int64_t yb = B * p.n_sym * 16;
  if (B == 0 || yb == 0) return AMR_OK;
  DevBuf d_off;                                  // this call's own; the stream is drained before it goes
  HIP_TRY(d_off.reserve(B * 8, nullptr));
  HIP_TRY(plan->mem.d_x.reserve(std::max<int64_t>(plan->max_streams * n * 8, 8), plan->stream));
  if (int rc = upload_batch(Copy::sync, plan->mem.d_x.get(), x, n * es, x_stride * es, B, plan->stream)) return rc;
  HIP_TRY(hipMemcpy(d_off.get(), offset, (size_t)B * 8, hipMemcpyHostToDevice));
  const hipError_t e = launch_dsss_despread(plan->mem.d_x.get(), dtype, n, B, p, plan->mem.T.as<double>(),
                                            d_off.as<int64_t>(), plan->mem.Y.as<double>(), plan->stream);
  if (e == hipSuccess) (void)hipMemcpyAsync(Y, plan->mem.Y.get(), (size_t)yb, hipMemcpyDeviceToHost, plan->stream);
  const hipError_t e2 = hipStreamSynchronize(plan->stream);
  HIP_TRY(e);
  HIP_TRY(e2);
  return AMR_OK;
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
  int64_t maxlen = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (n_bytes[i] < 0 || n_bytes[i] > data_stride) return fail(AMR_E_INVALID, "n_bytes out of range");
    maxlen = n_bytes[i] > maxlen ? n_bytes[i] : maxlen;
  }
  if (maxlen > 0 && !data) return fail(AMR_E_INVALID, "amr_dsss_modulate_host: NULL data");
  if (n == 0 || n_out == 0) return AMR_OK;
  t.sym_stride = (n_out + t.L - 1) / t.L;
  const int64_t stride = maxlen > 0 ? maxlen : 1;
  std::vector<double> tab((size_t)t.L);          // sg[i] * Sn[i], an exact sign flip
  for (int64_t i = 0; i < t.L; ++i) tab[(size_t)i] = cs[i / spc] * Sn[i];
  const auto bad = [](hipError_t e) {
    return fail(AMR_E_HIP, std::string("amr_dsss_modulate_host: ") + hipGetErrorString(e));
  };
  DevBuf d_tab, d_data, d_nb, d_out, d_pcm, d_sign;
  HIP_TRY_ELSE(d_tab.reserve(t.L * 8, nullptr), bad);
  HIP_TRY_ELSE(d_data.reserve(n * stride, nullptr), bad);
  HIP_TRY_ELSE(d_nb.reserve(n * 8, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(n * n_out * 4, nullptr), bad);
  if (pcm) HIP_TRY_ELSE(d_pcm.reserve(n * n_out * 2, nullptr), bad);
  HIP_TRY_ELSE(d_sign.reserve(n * t.sym_stride, nullptr), bad);
  HIP_TRY_ELSE(hipMemcpy(d_tab.get(), tab.data(), (size_t)t.L * 8, hipMemcpyHostToDevice), bad);
  if (maxlen > 0)
    HIP_TRY_ELSE(memcpy_rows(d_data.get(), stride, data, data_stride, maxlen, n, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(hipMemcpy(d_nb.get(), n_bytes, (size_t)n * 8, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(launch_dsss_tx(t, d_tab.as<double>(), d_data.as<uint8_t>(), stride, d_nb.as<int64_t>(), n,
                              d_sign.as<int8_t>(), d_out.as<float>(), n_out, d_pcm.as<int16_t>(), n_out, nullptr),
               bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  HIP_TRY_ELSE(memcpy_rows(out, out_stride * 4, d_out.get(), n_out * 4, n_out * 4, n, hipMemcpyDeviceToHost), bad);
  if (pcm)
    HIP_TRY_ELSE(memcpy_rows(pcm, pcm_stride * 2, d_pcm.get(), n_out * 2, n_out * 2, n, hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

}  // extern "C"
