// plan_core.h -- what amr_psk_plan and amr_fsk_plan share: the lock, stream,
// gather gate and timing events (PlanCore), a demod call's argument contract
// and the host entries' round trip.  Host code only: no kernel file includes it.
#pragma once
#include <algorithm>
#include <cstdio>
#include <mutex>

#include "amr_internal.h"
#include "api_common.h"
#include "env_switch.h"

namespace amr {

// N timing slots (AMR_T_COUNT / AMR_TF_COUNT): ev[slot] = {start, end}
template <int N>
struct PlanCore {
  std::mutex mu;
  int device = 0;
  hipStream_t stream = nullptr;
  GatherGate gate;              // an all-gather still reading this plan's outputs
  bool timing = false;
  hipEvent_t ev[N][2]{};
  bool ev_used[N]{};
  // AMR_SYNC_EACH_KERNEL=1: the slots below n_sync_names synchronise at their
  // end, so a fault names its kernel (the PSK plan's stages; none by default)
  const char* const* sync_names = nullptr;
  int n_sync_names = 0;
};

template <int N>
void core_clear_used(PlanCore<N>& c) {
  for (bool& u : c.ev_used) u = false;
}

// start (which = 0) or end (1) of `slot`, on the plan's stream;
// kNoSlot: nothing (a stage that runs inside another's slot)
constexpr int kNoSlot = -1;
template <int N>
hipError_t core_mark(PlanCore<N>& c, int slot, int which) {
  if (slot == kNoSlot) return hipSuccess;
  const hipStream_t st = c.stream;
  if (which == 1 && slot < c.n_sync_names) {
    static const bool sync_each = env_on("AMR_SYNC_EACH_KERNEL");
    if (sync_each) {
      const hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) {
        std::fprintf(stderr, "[amr] kernel slot %s failed: %s\n", c.sync_names[slot], hipGetErrorString(e));
        return e;
      }
    }
  }
  if (!c.timing) return hipSuccess;
  c.ev_used[slot] = true;
  return hipEventRecord(c.ev[slot][which], st);
}

// `body` (int(), an AMR_* code) between the slot's two marks; a failure
// returns at once, the slot's end unrecorded
template <int N, class F>
int timed(PlanCore<N>& c, int slot, F&& body) {
  HIP_TRY(core_mark(c, slot, 0));
  if (int rc = body()) return rc;
  HIP_TRY(core_mark(c, slot, 1));
  return AMR_OK;
}
// the same for one launch (a hipError_t expression), in HIP_TRY's form
#define HIP_TRY_TIMED(core, slot, expr)                                           \
  do {                                                                            \
    const int slot_ = (slot);                                                     \
    HIP_TRY(core_mark(core, slot_, 0)); HIP_TRY(expr); HIP_TRY(core_mark(core, slot_, 1)); \
  } while (0)

template <int N>
int core_synchronize(PlanCore<N>& c) {
  std::lock_guard<std::mutex> lk(c.mu);
  HIP_TRY(hipSetDevice(c.device));
  HIP_TRY(hipStreamSynchronize(c.stream));
  HIP_TRY(gate_sync(c.gate));
  return AMR_OK;
}

template <int N>
int core_enable_timing(PlanCore<N>& c, int on) {
  std::lock_guard<std::mutex> lk(c.mu);
  HIP_TRY(hipSetDevice(c.device));
  if (on && !c.ev[0][0]) {
    for (auto& e : c.ev)
      for (auto& h : e) HIP_TRY(hipEventCreate(&h));
  }
  c.timing = on != 0;
  return AMR_OK;
}

// milliseconds of each slot in the last call (-1 = not run)
template <int N>
int core_timings(PlanCore<N>& c, float* ms, int count) {
  std::lock_guard<std::mutex> lk(c.mu);
  HIP_TRY(hipSetDevice(c.device));
  HIP_TRY(hipStreamSynchronize(c.stream));
  for (int i = 0; i < count && i < N; ++i) {
    ms[i] = -1.0f;
    if (!c.timing || !c.ev_used[i]) continue;
    HIP_TRY(hipEventSynchronize(c.ev[i][1]));   // the launch slot may end on a comm stream (a gather)
    HIP_TRY(hipEventElapsedTime(&ms[i], c.ev[i][0], c.ev[i][1]));
  }
  return AMR_OK;
}

template <int N>
void core_destroy_events(PlanCore<N>& c) {
  for (auto& e : c.ev)
    for (auto& h : e)
      if (h) (void)hipEventDestroy(h);
}

// a caller's coefficient arrays as the kernels' Iir (zi: nt - 1 values, or null for zeros)
inline Iir make_iir(const double* b, const double* a, const double* zi, int nt) {
  Iir f{};
  f.nt = nt;
  for (int i = 0; i < nt; ++i) { f.b[i] = b[i]; f.a[i] = a[i]; }
  for (int i = 0; zi && i < nt - 1; ++i) f.zi[i] = zi[i];
  return f;
}

// ---- the argument contract of a demod call ---------------------------------
// One batch as the caller handed it over (host or device pointers)
struct DemodIo {
  const void* x;
  int dtype;
  int64_t B, x_stride;
  uint8_t* out;
  int64_t out_stride;
  int64_t *len, *sync;
};
// The device entries (run_psk, run_fsk) test the capacity first (a negative
// B there too), the host entries the dtype: the codes two bad arguments always had.
enum class ArgOrder { device, host };
template <class Plan>
int check_demod_args(const Plan* pl, const DemodIo& io, ArgOrder order) {
  const bool dtype_bad = dtype_size(io.dtype) == 0;
  if (order == ArgOrder::host && dtype_bad) return fail(AMR_E_INVALID, "unknown dtype");
  if ((order == ArgOrder::device && io.B < 0) || io.B > pl->max_streams)
    return fail(AMR_E_CAPACITY, "batch exceeds plan max_streams");
  if (dtype_bad) return fail(AMR_E_INVALID, "unknown dtype");
  if (io.x_stride < pl->p.n) return fail(AMR_E_INVALID, "x_stride < n_samples");
  if (io.out_stride < pl->out_cap - 1 || io.out_stride < 1) return fail(AMR_E_INVALID, "out_stride too small");
  return AMR_OK;
}

// ---- the host entries' round trip -----------------------------------------
// sync: api_common.h's blocking copies (their comments record why); async: queued on the stream, no wait
enum class Copy { sync, async };

// B rows of `row_bytes`, `src_pitch` apart on the host, into dense device rows
inline int upload_batch(Copy how, void* dst, const void* src, int64_t row_bytes, int64_t src_pitch, int64_t B,
                        hipStream_t st) {
  if (how == Copy::sync) return copy_batch_h2d(dst, src, row_bytes, src_pitch, B, st);
  if (src_pitch == row_bytes)
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)(B * row_bytes), hipMemcpyHostToDevice, st));
  else
    HIP_TRY(hipMemcpy2DAsync(dst, (size_t)row_bytes, src, (size_t)src_pitch, (size_t)row_bytes, (size_t)B,
                             hipMemcpyHostToDevice, st));
  return AMR_OK;
}

// the staged outputs [B][cap] to the caller's rows (cut to out_stride when
// that is shorter), the lengths and sync indices; sync waits for them
inline int download_batch(Copy how, const DemodIo& io, const void* d_out, int64_t cap, const void* d_len,
                          const void* d_sync, hipStream_t st) {
  const int64_t row = std::min(io.out_stride, cap);
  if (how == Copy::sync) {
    if (int rc = copy_batch_d2h(io.out, io.out_stride, d_out, cap, row, io.B, st)) return rc;
  } else if (io.out_stride == cap) {
    HIP_TRY(hipMemcpyAsync(io.out, d_out, (size_t)(io.B * cap), hipMemcpyDeviceToHost, st));
  } else {
    HIP_TRY(hipMemcpy2DAsync(io.out, (size_t)io.out_stride, d_out, (size_t)cap, (size_t)row, (size_t)io.B,
                             hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipMemcpyAsync(io.len, d_len, (size_t)io.B * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(io.sync, d_sync, (size_t)io.B * 8, hipMemcpyDeviceToHost, st));
  if (how == Copy::sync) HIP_TRY(hipStreamSynchronize(st));
  return AMR_OK;
}

// One host entry (`who` names it in the NULL message): the checks under the
// plan's lock, on its device; `launch` -- the plan's own staging, upload and
// kernels, the outputs left in mem.d_out / d_len / d_sync -- and the download.
template <class Plan, class F>
int host_round_trip(Plan* plan, const char* who, const DemodIo& io, Copy how, F&& launch) {
  if (!plan || (io.B && (!io.x || !io.out || !io.len || !io.sync)))
    return fail(AMR_E_INVALID, std::string(who) + ": NULL argument");
  std::lock_guard<std::mutex> lk(plan->mu);
  HIP_TRY(hipSetDevice(plan->device));
  // the same contract as the device entry, before any copy: a short
  // out_stride would cut rows while out_len still reports their full length
  if (int rc = check_demod_args(plan, io, ArgOrder::host)) return rc;
  if (io.B == 0) return AMR_OK;
  if (int rc = launch()) return rc;
  return download_batch(how, io, plan->mem.d_out.get(), plan->out_cap, plan->mem.d_len.get(), plan->mem.d_sync.get(),
                        plan->stream);
}

}  // namespace amr
