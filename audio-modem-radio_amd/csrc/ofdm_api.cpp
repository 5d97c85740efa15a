// ofdm_api.cpp -- C ABI of the multi-carrier DQPSK modem (include/amr.h,
// DESIGN.md §3j): amr_ofdm_plan on PlanCore with dev_mem.h ownership, the
// demodulation entries in the PSK entries' shape, the stage entries the tests
// pin the kernels with, the modulator, and acquisition (§3k: the work buffers,
// the stage entries and the acquired demodulation).  The kernels are
// ofdm_kernels.hip and ofdm_acq_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "ofdm.h"
#include "plan_core.h"

namespace amr {
hipError_t launch_sync_pack(const uint32_t*, int64_t, int64_t, int64_t, uint8_t*, int64_t, int64_t*, int64_t*,
                            hipStream_t);
}  // namespace amr

using namespace amr;

struct amr_ofdm_plan : PlanCore<AMR_TO_COUNT> {
  OfdmParams p{};
  int64_t max_streams = 0;
  int64_t out_cap = 0;
  // every device buffer the plan owns; ofdm_plan_free releases them together
  struct Mem {
    DevBuf W;                      // [nu][K][2]
    DevBuf Y;                      // [max_streams][S][K][2]
    DevBuf words;                  // [max_streams][n_words]
    // staging for the host entries (lazily sized)
    DevBuf d_x;
    DevBuf d_out, d_len, d_sync;   // one group: all three or none (reserve_all)
    // acquisition, from the first acquiring call on: one group
    DevBuf gq, G, E, dhat, off;    // [ms][segments][L], [ms][L], [ms][L], [ms], [ms]
  } mem;
};

namespace {

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

// set device, drain the stream, drop the gather gate; then the buffers; then events and the stream
void ofdm_plan_free(amr_ofdm_plan* pl) {
  if (!pl) return;
  (void)hipSetDevice(pl->device);
  if (pl->stream) (void)hipStreamSynchronize(pl->stream);
  gate_free(pl->gate);
  pl->mem = amr_ofdm_plan::Mem{};
  core_destroy_events(*pl);
  if (pl->stream) (void)hipStreamDestroy(pl->stream);
  delete pl;
}

// the acquisition group, allocated on the first acquiring call (all or nothing)
int ofdm_acq_reserve(amr_ofdm_plan* pl) {
  const int64_t ms = pl->max_streams, L = pl->p.L;
  amr_ofdm_plan::Mem& m = pl->mem;
  HIP_TRY((reserve_all({{m.gq, std::max<int64_t>(ms * ofdm_acq_segments(pl->p) * L * 8, 8)},
                        {m.G, ms * L * 8},
                        {m.E, ms * L * 8},
                        {m.dhat, ms * 8},
                        {m.off, ms * 8}},
                       pl->stream)));
  return AMR_OK;
}

// the acquisition kernels of one batch on the plan's stream, into mem.E / dhat / off
int run_acquire(amr_ofdm_plan* pl, const void* d_x, int dtype, int64_t B, int64_t x_stride) {
  if (int rc = ofdm_acq_reserve(pl)) return rc;
  amr_ofdm_plan::Mem& m = pl->mem;
  const OfdmAcq a{m.gq.as<double>(), m.G.as<double>(), m.E.as<double>(), m.dhat.as<int64_t>(), m.off.as<int64_t>()};
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
    double* Y = pl->mem.Y.as<double>();
    uint32_t* words = pl->mem.words.as<uint32_t>();
    if (acquire)
      HIP_TRY_TIMED(*pl, AMR_TO_DFT, launch_ofdm_dft_at(io.x, io.dtype, io.x_stride, io.B, p, pl->mem.W.as<double>(),
                                                        pl->mem.off.as<int64_t>(), Y, st));
    else
      HIP_TRY_TIMED(*pl, AMR_TO_DFT,
                    launch_ofdm_dft(io.x, io.dtype, io.x_stride, io.B, p, pl->mem.W.as<double>(), Y, st));
    HIP_TRY_TIMED(*pl, AMR_TO_SLICE, launch_ofdm_slice(Y, io.B, p, words, st));
    return timed(*pl, AMR_TO_SYNC_PACK, [&]() -> int {
      HIP_TRY(launch_sync_pack(words, p.n_words, p.n_bits, io.B, io.out, io.out_stride, io.len, io.sync, st));
      if (soft) HIP_TRY(launch_ofdm_soft(Y, io.B, p, words, io.sync, io.len, soft, soft_stride, st));
      return AMR_OK;
    });
  });
}

int ofdm_host_staging(amr_ofdm_plan* pl) {
  const int64_t ms = pl->max_streams;
  HIP_TRY(pl->mem.d_x.reserve(std::max<int64_t>(ms * pl->p.n * 8, 8), pl->stream));
  HIP_TRY((reserve_all({{pl->mem.d_out, ms * pl->out_cap}, {pl->mem.d_len, ms * 8}, {pl->mem.d_sync, ms * 8}},
                       pl->stream)));
  return AMR_OK;
}

// a host entry (plan_core.h host_round_trip); soft: the soft values too,
// through a staging block of this call's own; acquire: as run_ofdm, the
// offsets to `offset` (host, or null)
int ofdm_demod_host(amr_ofdm_plan* plan, const char* who, const DemodIo& h, int8_t* soft, int64_t soft_stride,
                    bool acquire = false, int64_t* offset = nullptr) {
  DevBuf d_soft;
  int64_t sv = 0;
  const int rc = host_round_trip(plan, who, h, Copy::sync, [&]() -> int {
    amr_ofdm_plan::Mem& m = plan->mem;
    const int64_t n = plan->p.n, es = dtype_size(h.dtype);
    if (int rc = ofdm_host_staging(plan)) return rc;
    if (n > 0)
      if (int rc = upload_batch(Copy::sync, m.d_x.get(), h.x, n * es, h.x_stride * es, h.B, plan->stream)) return rc;
    const DemodIo d{m.d_x.get(), h.dtype, h.B, n, m.d_out.as<uint8_t>(), plan->out_cap, m.d_len.as<int64_t>(),
                    m.d_sync.as<int64_t>()};
    if (soft) {
      sv = std::max<int64_t>(plan->p.n_bits, 1);
      HIP_TRY(d_soft.reserve(h.B * sv, nullptr));
    }
    if (int rc = run_ofdm(plan, d, soft ? d_soft.as<int8_t>() : nullptr, sv, acquire)) return rc;
    if (acquire && offset)                     // queued like the round trip's own downloads, which wait for the stream
      HIP_TRY(hipMemcpyAsync(offset, m.off.get(), (size_t)h.B * 8, hipMemcpyDeviceToHost, plan->stream));
    return AMR_OK;
  });
  if (rc || !soft || h.B == 0) return rc;
  // only the values of the stream's bytes reach the caller's row
  std::vector<int8_t> tmp((size_t)(h.B * sv));
  HIP_TRY(hipMemcpy(tmp.data(), d_soft.get(), tmp.size(), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < h.B; ++i)
    std::memcpy(soft + i * soft_stride, tmp.data() + i * sv, (size_t)std::min(8 * h.len[i], soft_stride));
  return AMR_OK;
}

// the stage entries: k_ofdm_slice on given Y (the words to `words`, or null), with `soft` k_ofdm_soft, every bit from 0
int ofdm_symbol_stages(const char* who, const double* Y, int64_t n_streams, int64_t n_sym, int K, uint32_t* words,
                       int8_t* soft) {
  const std::string name(who);
  if (K < 1 || K > kOfdmMaxK) return fail(AMR_E_INVALID, name + ": num_subcarriers must be 1..64");
  if (n_streams < 0 || n_sym < 0 || (n_streams && n_sym && (!Y || (!words && !soft))))
    return fail(AMR_E_INVALID, name + ": bad argument");
  OfdmParams p{};
  p.K = K;
  p.n_sym = n_sym;
  p.n_bits = n_sym >= 2 ? 2 * (int64_t)K * (n_sym - 1) : 0;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
  if (n_streams == 0 || p.n_bits == 0) return AMR_OK;
  const auto bad = [&name](hipError_t e) { return fail(AMR_E_HIP, name + ": " + hipGetErrorString(e)); };
  const int64_t yb = n_streams * n_sym * K * 16;
  DevBuf d_y, d_words, d_soft;
  HIP_TRY_ELSE(d_y.reserve(yb, nullptr), bad);
  HIP_TRY_ELSE(d_words.reserve(n_streams * p.n_words * 4, nullptr), bad);
  if (soft) HIP_TRY_ELSE(d_soft.reserve(n_streams * p.n_bits, nullptr), bad);
  HIP_TRY_ELSE(hipMemcpy(d_y.get(), Y, (size_t)yb, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(launch_ofdm_slice(d_y.as<double>(), n_streams, p, d_words.as<uint32_t>(), nullptr), bad);
  if (soft)
    HIP_TRY_ELSE(launch_ofdm_soft(d_y.as<double>(), n_streams, p, d_words.as<uint32_t>(), nullptr, nullptr,
                                  d_soft.as<int8_t>(), p.n_bits, nullptr),
                 bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  if (words)
    HIP_TRY_ELSE(hipMemcpy(words, d_words.get(), (size_t)(n_streams * p.n_words) * 4, hipMemcpyDeviceToHost), bad);
  if (soft) HIP_TRY_ELSE(hipMemcpy(soft, d_soft.get(), (size_t)(n_streams * p.n_bits), hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

// amr_ofdm_acquire_host / _device: the acquisition stage alone.  host: x, offset, dhat and E are host memory
// (x staged in mem.d_x, the call waits); else device memory, the copies queued on the plan's stream.
int ofdm_acquire_entry(amr_ofdm_plan* plan, const char* who, bool host, const void* x, int dtype, int64_t B,
                       int64_t x_stride, int64_t* offset, int64_t* dhat, double* E) {
  if (!plan || (B && (!x || !offset))) return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  const OfdmParams& p = plan->p;
  const int64_t es = dtype_size(dtype), n = p.n;
  if (es == 0) return fail(AMR_E_INVALID, "unknown dtype");
  if (B < 0 || B > plan->max_streams) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  HIP_TRY(hipSetDevice(plan->device));
  core_clear_used(*plan);
  if (B == 0) return AMR_OK;
  amr_ofdm_plan::Mem& m = plan->mem;
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
  if (dhat) HIP_TRY(hipMemcpyAsync(dhat, m.dhat.get(), (size_t)B * 8, kind, st));
  if (E) HIP_TRY(hipMemcpyAsync(E, m.E.get(), (size_t)(B * p.L) * 8, kind, st));
  if (host) HIP_TRY(hipStreamSynchronize(st));
  return AMR_OK;
}

// the checks amr_ofdm_demod_soft_* make before the shared contract, `soft` optional here
int demod_acq_precheck(const amr_ofdm_plan* plan, const char* who, int64_t B, int64_t x_stride, int64_t out_stride,
                       const int8_t* soft, int64_t soft_stride) {
  const std::string name(who);
  if (B < 0 || x_stride < 0 || out_stride < 0 || (soft && soft_stride < 0)) return fail(AMR_E_INVALID, name + ": negative argument");
  if (!plan) return fail(AMR_E_INVALID, name + ": NULL argument");
  if (soft && soft_stride < 8 * plan->out_cap)
    return fail(AMR_E_INVALID, name + ": soft_stride < 8 * amr_ofdm_plan_out_capacity()");
  return AMR_OK;
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
  auto* pl = new amr_ofdm_plan();
  pl->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete pl;
    return fail(AMR_E_NODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  }
  pl->p = p;
  pl->max_streams = max_streams;
  pl->out_cap = p.n_bits / 8 + 1;
  amr_ofdm_plan::Mem& m = pl->mem;
  const struct { DevBuf* buf; int64_t bytes; } allocs[] = {
      {&m.W, p.nu * K * 16}, {&m.Y, y_bytes(p, max_streams)}, {&m.words, max_streams * p.n_words * 4}};
  for (const auto& a : allocs) {
    e = a.buf->reserve(a.bytes, nullptr);
    if (e != hipSuccess) {
      ofdm_plan_free(pl);
      return fail(AMR_E_NOMEM, "hipMalloc(" + std::to_string(a.bytes) + " B): " + hipGetErrorString(e));
    }
  }
  {
    // [K][nu][2] -> [nu][K][2]: a group of subcarriers at one m contiguous (k_ofdm_dft's uniform loads)
    std::vector<double> w((size_t)(p.nu * K * 2));
    for (int k = 0; k < K; ++k)
      for (int64_t i = 0; i < p.nu; ++i)
        for (int c = 0; c < 2; ++c) w[(size_t)((i * K + k) * 2 + c)] = W[(size_t)((k * p.nu + i) * 2 + c)];
    e = hipMemcpy(m.W.get(), w.data(), w.size() * 8, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    ofdm_plan_free(pl);
    return fail(AMR_E_HIP, std::string("plan setup: ") + hipGetErrorString(e));
  }
  *out = pl;
  return AMR_OK;
}

int amr_ofdm_plan_destroy(amr_ofdm_plan* plan) {
  ofdm_plan_free(plan);
  return AMR_OK;
}

int amr_ofdm_plan_synchronize(amr_ofdm_plan* plan) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_synchronize(*plan);
}

int amr_ofdm_plan_enable_timing(amr_ofdm_plan* plan, int on) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_enable_timing(*plan, on);
}

int amr_ofdm_plan_timings(amr_ofdm_plan* plan, float* ms, int count) {
  if (!plan || !ms) return fail(AMR_E_INVALID, "NULL argument");
  return core_timings(*plan, ms, count);
}

int64_t amr_ofdm_plan_out_capacity(const amr_ofdm_plan* plan) { return plan ? plan->out_cap : -1; }

int64_t amr_ofdm_plan_scratch_bytes(const amr_ofdm_plan* plan) {
  if (!plan) return -1;
  const amr_ofdm_plan::Mem& m = plan->mem;
  return m.W.bytes() + m.Y.bytes() + m.words.bytes() + m.d_x.bytes() + m.d_out.bytes() + m.d_len.bytes() +
         m.d_sync.bytes() + m.gq.bytes() + m.G.bytes() + m.E.bytes() + m.dhat.bytes() + m.off.bytes();
}

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
  if (n_streams < 0 || x_stride < 0 || out_stride < 0 || soft_stride < 0)
    return fail(AMR_E_INVALID, "amr_ofdm_demod_soft_device: negative argument");
  if (!plan || (n_streams && (!d_x || !d_out || !d_out_len || !d_sync_idx || !d_soft)))
    return fail(AMR_E_INVALID, "amr_ofdm_demod_soft_device: NULL argument");
  if (soft_stride < 8 * plan->out_cap)
    return fail(AMR_E_INVALID, "amr_ofdm_demod_soft_device: soft_stride < 8 * amr_ofdm_plan_out_capacity()");
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
  if (B < 0 || x_stride < 0 || out_stride < 0 || soft_stride < 0)
    return fail(AMR_E_INVALID, "amr_ofdm_demod_soft_host: negative argument");
  if (!plan || (B && !soft)) return fail(AMR_E_INVALID, "amr_ofdm_demod_soft_host: NULL argument");
  if (soft_stride < 8 * plan->out_cap)
    return fail(AMR_E_INVALID, "amr_ofdm_demod_soft_host: soft_stride < 8 * amr_ofdm_plan_out_capacity()");
  return ofdm_demod_host(plan, "amr_ofdm_demod_soft_host",
                         {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx}, soft, soft_stride);
}

int amr_ofdm_symbols_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, double* Y) {
  if (!plan || (B && (!x || !Y))) return fail(AMR_E_INVALID, "amr_ofdm_symbols_host: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  const int64_t es = dtype_size(dtype), n = plan->p.n;
  if (es == 0) return fail(AMR_E_INVALID, "unknown dtype");
  if (B < 0 || B > plan->max_streams) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  const int64_t yb = B * plan->p.n_sym * plan->p.K * 16;
  if (B == 0 || yb == 0) return AMR_OK;
  HIP_TRY(plan->mem.d_x.reserve(std::max<int64_t>(plan->max_streams * n * 8, 8), plan->stream));
  if (int rc = upload_batch(Copy::sync, plan->mem.d_x.get(), x, n * es, x_stride * es, B, plan->stream)) return rc;
  HIP_TRY(launch_ofdm_dft(plan->mem.d_x.get(), dtype, n, B, plan->p, plan->mem.W.as<double>(),
                          plan->mem.Y.as<double>(), plan->stream));
  HIP_TRY(hipMemcpyAsync(Y, plan->mem.Y.get(), (size_t)yb, hipMemcpyDeviceToHost, plan->stream));
  HIP_TRY(hipStreamSynchronize(plan->stream));
  return AMR_OK;
}

int amr_ofdm_symbols_at_host(amr_ofdm_plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride,
                             const int64_t* offset, double* Y) {
  if (!plan || (B && (!x || !offset || !Y))) return fail(AMR_E_INVALID, "amr_ofdm_symbols_at_host: NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  const OfdmParams& p = plan->p;
  const int64_t es = dtype_size(dtype), n = p.n;
  if (es == 0) return fail(AMR_E_INVALID, "unknown dtype");
  if (B < 0 || B > plan->max_streams) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  for (int64_t i = 0; i < B; ++i)
    if (offset[i] < -p.ncp || offset[i] > p.L - 1 - p.ncp)
      return fail(AMR_E_INVALID, "amr_ofdm_symbols_at_host: offset outside [-Ncp, L - 1 - Ncp]");
  HIP_TRY(hipSetDevice(plan->device));
  const int64_t yb = B * p.n_sym * p.K * 16;
  if (B == 0 || yb == 0) return AMR_OK;
  DevBuf d_off;                                  // this call's own; the stream is drained before it goes
  HIP_TRY(d_off.reserve(B * 8, nullptr));
  HIP_TRY(plan->mem.d_x.reserve(std::max<int64_t>(plan->max_streams * n * 8, 8), plan->stream));
  if (int rc = upload_batch(Copy::sync, plan->mem.d_x.get(), x, n * es, x_stride * es, B, plan->stream)) return rc;
  HIP_TRY(hipMemcpy(d_off.get(), offset, (size_t)B * 8, hipMemcpyHostToDevice));
  const hipError_t e = launch_ofdm_dft_at(plan->mem.d_x.get(), dtype, n, B, p, plan->mem.W.as<double>(),
                                          d_off.as<int64_t>(), plan->mem.Y.as<double>(), plan->stream);
  if (e == hipSuccess) (void)hipMemcpyAsync(Y, plan->mem.Y.get(), (size_t)yb, hipMemcpyDeviceToHost, plan->stream);
  const hipError_t e2 = hipStreamSynchronize(plan->stream);
  HIP_TRY(e);
  HIP_TRY(e2);
  return AMR_OK;
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
  if (int rc = demod_acq_precheck(plan, "amr_ofdm_demod_acq_host", B, x_stride, out_stride, soft, soft_stride))
    return rc;
  return ofdm_demod_host(plan, "amr_ofdm_demod_acq_host", {x, dtype, B, x_stride, out, out_stride, out_len, sync_idx},
                         soft, soft_stride, true, offset);
}

int amr_ofdm_demod_acq_device(amr_ofdm_plan* plan, const void* d_x, int dtype, int64_t n_streams, int64_t x_stride,
                              uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int64_t* d_sync_idx,
                              int8_t* d_soft, int64_t soft_stride, int64_t* d_offset) {
  if (int rc = demod_acq_precheck(plan, "amr_ofdm_demod_acq_device", n_streams, x_stride, out_stride, d_soft,
                                  soft_stride))
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
  int64_t maxlen = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (n_bytes[i] < 0 || n_bytes[i] > data_stride) return fail(AMR_E_INVALID, "n_bytes out of range");
    maxlen = n_bytes[i] > maxlen ? n_bytes[i] : maxlen;
  }
  if (maxlen > 0 && !data) return fail(AMR_E_INVALID, "amr_ofdm_modulate_host: NULL data");
  if (n == 0 || n_out == 0) return AMR_OK;
  t.sym_stride = (n_out + t.L - 1) / t.L;
  const int64_t stride = maxlen > 0 ? maxlen : 1;
  const auto bad = [](hipError_t e) {
    return fail(AMR_E_HIP, std::string("amr_ofdm_modulate_host: ") + hipGetErrorString(e));
  };
  DevBuf d_data, d_nb, d_out, d_pcm, d_work;
  HIP_TRY_ELSE(d_data.reserve(n * stride, nullptr), bad);
  HIP_TRY_ELSE(d_nb.reserve(n * 8, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(n * n_out * 4, nullptr), bad);
  if (pcm) HIP_TRY_ELSE(d_pcm.reserve(n * n_out * 2, nullptr), bad);
  HIP_TRY_ELSE(d_work.reserve(n * t.sym_stride * K * 8, nullptr), bad);
  if (maxlen > 0)
    HIP_TRY_ELSE(memcpy_rows(d_data.get(), stride, data, data_stride, maxlen, n, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(hipMemcpy(d_nb.get(), n_bytes, (size_t)n * 8, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(launch_ofdm_tx(t, d_data.as<uint8_t>(), stride, d_nb.as<int64_t>(), n, d_work.as<double>(),
                              d_out.as<float>(), n_out, d_pcm.as<int16_t>(), n_out, nullptr),
               bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  HIP_TRY_ELSE(memcpy_rows(out, out_stride * 4, d_out.get(), n_out * 4, n_out * 4, n, hipMemcpyDeviceToHost), bad);
  if (pcm)
    HIP_TRY_ELSE(memcpy_rows(pcm, pcm_stride * 2, d_pcm.get(), n_out * 2, n_out * 2, n, hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

}  // extern "C"
