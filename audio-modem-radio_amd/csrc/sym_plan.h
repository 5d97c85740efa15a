// sym_plan.h -- the host core the symbol modems' plans share (amr_ofdm_plan,
// amr_dsss_plan): a plan base on PlanCore with the buffers
// every such plan has, plan setup and free, the host entries' checks and
// staging, the host demodulation round trip, the acquisition and symbol stage
// entries and the plan accessors.  What differs between the modems comes in as
// a callable.  Host code only: no kernel file includes it.
#pragma once
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "plan_core.h"
#include "tx_host.h"

namespace amr {

// A symbol modem's plan: N timing slots, NOwn buffers of the modem's own
// (tables and acquisition work, indexed by the modem's enum).  The plan type
// adds its params struct `p` (n, n_bits, L among its fields).
template <int N, int NOwn>
struct SymPlan : PlanCore<N> {
  int64_t max_streams = 0;
  int64_t out_cap = 0;
  // every device buffer the plan owns; sym_plan_free releases them together
  struct Mem {
    DevBuf Y;                      // [max_streams][S] symbols, the modem's layout
    DevBuf words;                  // [max_streams][n_words]
    // staging for the host entries (lazily sized)
    DevBuf d_x;
    DevBuf d_out, d_len, d_sync;   // one group: all three or none (reserve_all)
    DevBuf off;                    // [max_streams] acquired offsets, with the modem's acquisition group
    DevBuf own[NOwn];
    int64_t bytes() const {
      int64_t t = 0;
      for (const DevBuf* b : {&Y, &words, &d_x, &d_out, &d_len, &d_sync, &off}) t += b->bytes();
      for (const DevBuf& b : own) t += b.bytes();
      return t;
    }
  } mem;
};

// set device, drain the stream, drop the gather gate; then the buffers; then events and the stream
template <class Plan>
void sym_plan_free(Plan* pl) {
  if (!pl) return;
  (void)hipSetDevice(pl->device);
  if (pl->stream) (void)hipStreamSynchronize(pl->stream);
  gate_free(pl->gate);
  pl->mem = typename Plan::Mem{};
  core_destroy_events(*pl);
  if (pl->stream) (void)hipStreamDestroy(pl->stream);
  delete pl;
}

// one buffer a plan is created with; src (host, or null): its contents
struct SymAlloc {
  DevBuf* buf;
  int64_t bytes;
  const void* src;
};

// The device half of *_plan_create, `pl` new and its p set; takes `pl` over:
// *out on success, freed otherwise.
template <class Plan>
int sym_plan_setup(Plan* pl, int device, int64_t max_streams, std::initializer_list<SymAlloc> allocs, Plan** out) {
  pl->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete pl;
    return fail(AMR_E_NODEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  }
  pl->max_streams = max_streams;
  pl->out_cap = pl->p.n_bits / 8 + 1;
  for (const SymAlloc& a : allocs) {
    e = a.buf->reserve(a.bytes, nullptr);
    if (e != hipSuccess) {
      sym_plan_free(pl);
      return fail(AMR_E_NOMEM, "hipMalloc(" + std::to_string(a.bytes) + " B): " + hipGetErrorString(e));
    }
    if (a.src) e = hipMemcpy(a.buf->get(), a.src, (size_t)a.bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) break;
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    sym_plan_free(pl);
    return fail(AMR_E_HIP, std::string("plan setup: ") + hipGetErrorString(e));
  }
  *out = pl;
  return AMR_OK;
}

// ---- the plan accessors ------------------------------------------------------
template <class Plan>
int sym_plan_synchronize(Plan* plan) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_synchronize(*plan);
}
template <class Plan>
int sym_plan_enable_timing(Plan* plan, int on) {
  if (!plan) return fail(AMR_E_INVALID, "plan is NULL");
  return core_enable_timing(*plan, on);
}
template <class Plan>
int sym_plan_timings(Plan* plan, float* ms, int count) {
  if (!plan || !ms) return fail(AMR_E_INVALID, "NULL argument");
  return core_timings(*plan, ms, count);
}

// ---- checks and staging --------------------------------------------------------
// the checks of an entry that reads a batch of x outside the demod contract
template <class Plan>
int batch_check(const Plan* plan, int dtype, int64_t B, int64_t x_stride) {
  if (dtype_size(dtype) == 0) return fail(AMR_E_INVALID, "unknown dtype");
  if (B < 0 || B > plan->max_streams) return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (x_stride < plan->p.n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  return AMR_OK;
}

// The checks an entry with soft values makes before the shared contract.
// has_soft: soft_stride counts (an entry where `soft` is optional passes
// soft != null); null_arg: the entry's own NULL test besides the plan;
// cap_fn: the capacity function the message names.
template <class Plan>
int demod_precheck(const Plan* plan, const char* who, const char* cap_fn, int64_t B, int64_t x_stride,
                   int64_t out_stride, bool has_soft, int64_t soft_stride, bool null_arg = false) {
  const std::string name(who);
  if (B < 0 || x_stride < 0 || out_stride < 0 || (has_soft && soft_stride < 0))
    return fail(AMR_E_INVALID, name + ": negative argument");
  if (!plan || null_arg) return fail(AMR_E_INVALID, name + ": NULL argument");
  if (has_soft && soft_stride < 8 * plan->out_cap)
    return fail(AMR_E_INVALID, name + ": soft_stride < 8 * " + cap_fn + "()");
  return AMR_OK;
}

template <class Plan>
int stage_x(Plan* pl) {
  HIP_TRY(pl->mem.d_x.reserve(std::max<int64_t>(pl->max_streams * pl->p.n * 8, 8), pl->stream));
  return AMR_OK;
}
template <class Plan>
int host_staging(Plan* pl) {
  const int64_t ms = pl->max_streams;
  if (int rc = stage_x(pl)) return rc;
  HIP_TRY((reserve_all({{pl->mem.d_out, ms * pl->out_cap}, {pl->mem.d_len, ms * 8}, {pl->mem.d_sync, ms * 8}},
                       pl->stream)));
  return AMR_OK;
}

// ---- the host demodulation ------------------------------------------------------
// A host entry (plan_core.h host_round_trip).  run: int(const DemodIo& d,
// int8_t* d_soft, int64_t soft_stride), the plan's run_* on the staged batch.
// soft (or null): the soft values too, through a staging block of this call's
// own; offset (or null): the offsets an acquiring run left in mem.off, zeros
// when it did not acquire.
template <class Plan, class Run>
int demod_host(Plan* plan, const char* who, const DemodIo& h, int8_t* soft, int64_t soft_stride, int64_t* offset,
               bool acquire, Run&& run) {
  DevBuf d_soft;                                 // this call's own; the round trip waits for the stream
  int64_t sv = 0;
  const int rc = host_round_trip(plan, who, h, Copy::sync, [&]() -> int {
    auto& m = plan->mem;
    const int64_t n = plan->p.n, es = dtype_size(h.dtype);
    if (int rc = host_staging(plan)) return rc;
    if (n > 0)
      if (int rc = upload_batch(Copy::sync, m.d_x.get(), h.x, n * es, h.x_stride * es, h.B, plan->stream)) return rc;
    const DemodIo d{m.d_x.get(), h.dtype, h.B, n, m.d_out.template as<uint8_t>(), plan->out_cap,
                    m.d_len.template as<int64_t>(), m.d_sync.template as<int64_t>()};
    if (soft) {
      sv = std::max<int64_t>(plan->p.n_bits, 1);
      HIP_TRY(d_soft.reserve(h.B * sv, nullptr));
    }
    if (int rc = run(d, d_soft.as<int8_t>(), sv)) return rc;
    if (offset && acquire)                     // queued like the round trip's own downloads, which wait for the stream
      HIP_TRY(hipMemcpyAsync(offset, m.off.get(), (size_t)h.B * 8, hipMemcpyDeviceToHost, plan->stream));
    if (offset && !acquire) std::memset(offset, 0, (size_t)h.B * 8);
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

// ---- the stage entries ------------------------------------------------------------
// one output of an acquisition entry besides the offsets: dst (or null: not wanted), the plan's buffer, its row
struct AcqOut {
  void* dst;
  const DevBuf* src;
  int64_t row_bytes;
};

// *_acquire_host / _device: the acquisition stage alone.  host: x, offset and the outs are host memory (x staged
// in mem.d_x, the call waits); else device memory, the copies queued on the plan's stream.  run: int(d_x, x_stride),
// the plan's acquisition kernels, the offsets left in mem.off.
template <class Plan, class Run>
int acquire_entry(Plan* plan, const char* who, bool host, const void* x, int dtype, int64_t B, int64_t x_stride,
                  int64_t* offset, std::initializer_list<AcqOut> outs, Run&& run) {
  if (!plan || (B && (!x || !offset))) return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  if (int rc = batch_check(plan, dtype, B, x_stride)) return rc;
  const int64_t es = dtype_size(dtype), n = plan->p.n;
  HIP_TRY(hipSetDevice(plan->device));
  core_clear_used(*plan);
  if (B == 0) return AMR_OK;
  auto& m = plan->mem;
  hipStream_t st = plan->stream;
  const void* d_x = x;
  int64_t stride = x_stride;
  if (host) {
    if (int rc = stage_x(plan)) return rc;
    if (n > 0)
      if (int rc = upload_batch(Copy::sync, m.d_x.get(), x, n * es, x_stride * es, B, st)) return rc;
    d_x = m.d_x.get();
    stride = n;
  }
  if (int rc = run(d_x, stride)) return rc;
  const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIP_TRY(hipMemcpyAsync(offset, m.off.get(), (size_t)B * 8, kind, st));
  for (const AcqOut& o : outs)
    if (o.dst) HIP_TRY(hipMemcpyAsync(o.dst, o.src->get(), (size_t)(B * o.row_bytes), kind, st));
  if (host) HIP_TRY(hipStreamSynchronize(st));
  return AMR_OK;
}

// *_symbols_host / _symbols_at_host behind their checks (the caller holds mu): x staged in mem.d_x, offset
// (host, or null) in a block of this call's own, launch: hipError_t(d_x, d_offset) into mem.Y on the plan's
// stream, then the first y_bytes of mem.Y to Y.
template <class Plan, class Launch>
int symbols_round_trip(Plan* plan, const void* x, int dtype, int64_t B, int64_t x_stride, const int64_t* offset,
                       double* Y, int64_t y_bytes, Launch&& launch) {
  HIP_TRY(hipSetDevice(plan->device));
  if (B == 0 || y_bytes == 0) return AMR_OK;
  const int64_t es = dtype_size(dtype), n = plan->p.n;
  DevBuf d_off;                                  // this call's own; the stream is drained before it goes
  if (offset) HIP_TRY(d_off.reserve(B * 8, nullptr));
  if (int rc = stage_x(plan)) return rc;
  if (int rc = upload_batch(Copy::sync, plan->mem.d_x.get(), x, n * es, x_stride * es, B, plan->stream)) return rc;
  if (offset) HIP_TRY(hipMemcpy(d_off.get(), offset, (size_t)B * 8, hipMemcpyHostToDevice));
  const hipError_t e = launch(plan->mem.d_x.get(), d_off.as<int64_t>());
  if (e == hipSuccess) (void)hipMemcpyAsync(Y, plan->mem.Y.get(), (size_t)y_bytes, hipMemcpyDeviceToHost, plan->stream);
  const hipError_t e2 = hipStreamSynchronize(plan->stream);
  HIP_TRY(e);
  HIP_TRY(e2);
  return AMR_OK;
}

// *_slice_host / _soft_host: the slicer on given Y (the words to `words`, or null), with `soft` the soft kernel,
// every bit from 0.  p: the modem's params with its own fields set; a symbol is sym_vals complex values and
// sym_bits bits.  slice: hipError_t(Y, p, words), soft_k: hipError_t(Y, p, words, soft), device pointers.
// ref_syms: the symbols that carry no bits of their own: 1 for a differential modem (the first is the
// reference), 0 where every symbol carries bits (tone8).
template <class Params, class Slice, class SoftK>
int symbol_stages(const char* who, Params p, int64_t sym_vals, int64_t sym_bits, const double* Y, int64_t n_streams,
                  int64_t n_sym, uint32_t* words, int8_t* soft, Slice&& slice, SoftK&& soft_k, int64_t ref_syms = 1) {
  if (n_streams < 0 || n_sym < 0 || (n_streams && n_sym && (!Y || (!words && !soft))))
    return fail(AMR_E_INVALID, std::string(who) + ": bad argument");
  p.n_sym = n_sym;
  p.n_bits = n_sym > ref_syms ? sym_bits * (n_sym - ref_syms) : 0;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
  if (n_streams == 0 || p.n_bits == 0) return AMR_OK;
  const auto bad = hip_fail_as(who);
  const int64_t yb = n_streams * n_sym * sym_vals * 16;
  DevBuf d_y, d_words, d_soft;
  HIP_TRY_ELSE(d_y.reserve(yb, nullptr), bad);
  HIP_TRY_ELSE(d_words.reserve(n_streams * p.n_words * 4, nullptr), bad);
  if (soft) HIP_TRY_ELSE(d_soft.reserve(n_streams * p.n_bits, nullptr), bad);
  HIP_TRY_ELSE(hipMemcpy(d_y.get(), Y, (size_t)yb, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(slice(d_y.as<double>(), p, d_words.as<uint32_t>()), bad);
  if (soft) HIP_TRY_ELSE(soft_k(d_y.as<double>(), p, d_words.as<uint32_t>(), d_soft.as<int8_t>()), bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  if (words)
    HIP_TRY_ELSE(hipMemcpy(words, d_words.get(), (size_t)(n_streams * p.n_words) * 4, hipMemcpyDeviceToHost), bad);
  if (soft) HIP_TRY_ELSE(hipMemcpy(soft, d_soft.get(), (size_t)(n_streams * p.n_bits), hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

}  // namespace amr
