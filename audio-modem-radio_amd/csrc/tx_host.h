// tx_host.h -- the staged round trip the *_modulate_host entries share
// (tx_api.cpp, ofdm_api.cpp, dsss_api.cpp).  Host code only: no kernel file
// includes it.
#pragma once
#include <string>

#include "api_common.h"
#include "dev_mem.h"

namespace amr {

// an entry's own failure report: AMR_E_HIP, "<who>: <the HIP error>" (HIP_TRY_ELSE's on_fail)
inline auto hip_fail_as(const char* who) {
  return [who](hipError_t e) { return fail(AMR_E_HIP, std::string(who) + ": " + hipGetErrorString(e)); };
}

// one modulate call's staged buffers (device memory): data [n][stride], n_bytes [n],
// out [n][n_out], pcm [n][n_out] or null
struct TxDev {
  const uint8_t* data;
  int64_t stride;
  const int64_t* n_bytes;
  float* out;
  int16_t* pcm;
};

// After the entry's own checks: n_bytes against data_stride, the NULL-data
// rule, nothing to do for no stream or no sample; then the payloads staged,
// `launch` (int(const TxDev&), an AMR_* code: the entry's work buffers and its
// kernels on the null stream), the device drained, out and pcm copied back.
// Failures are reported under `who`.
template <class F>
int modulate_round_trip(const char* who, const uint8_t* data, int64_t data_stride, const int64_t* n_bytes, int64_t n,
                        float* out, int64_t out_stride, int64_t n_out, int16_t* pcm, int64_t pcm_stride, F&& launch) {
  int64_t maxlen = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (n_bytes[i] < 0 || n_bytes[i] > data_stride) return fail(AMR_E_INVALID, "n_bytes out of range");
    maxlen = n_bytes[i] > maxlen ? n_bytes[i] : maxlen;
  }
  if (maxlen > 0 && !data) return fail(AMR_E_INVALID, std::string(who) + ": NULL data");
  if (n == 0 || n_out == 0) return AMR_OK;
  const int64_t stride = maxlen > 0 ? maxlen : 1;
  const auto bad = hip_fail_as(who);
  DevBuf d_data, d_nb, d_out, d_pcm;
  HIP_TRY_ELSE(d_data.reserve(n * stride, nullptr), bad);
  HIP_TRY_ELSE(d_nb.reserve(n * 8, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(n * n_out * 4, nullptr), bad);
  if (pcm) HIP_TRY_ELSE(d_pcm.reserve(n * n_out * 2, nullptr), bad);
  if (maxlen > 0)
    HIP_TRY_ELSE(memcpy_rows(d_data.get(), stride, data, data_stride, maxlen, n, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(hipMemcpy(d_nb.get(), n_bytes, (size_t)n * 8, hipMemcpyHostToDevice), bad);
  if (int rc = launch(TxDev{d_data.as<uint8_t>(), stride, d_nb.as<int64_t>(), d_out.as<float>(), d_pcm.as<int16_t>()}))
    return rc;
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  HIP_TRY_ELSE(memcpy_rows(out, out_stride * 4, d_out.get(), n_out * 4, n_out * 4, n, hipMemcpyDeviceToHost), bad);
  if (pcm)
    HIP_TRY_ELSE(memcpy_rows(pcm, pcm_stride * 2, d_pcm.get(), n_out * 2, n_out * 2, n, hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

}  // namespace amr
