// viterbi_api.cpp -- C ABI of the convolutional code (include/amr.h): the batched
// encoder of fec.ConvolutionalEncoder.encode (fec.py:79-111) and a
// maximum-likelihood hard-decision Viterbi decoder for it, and
// the same decoder on int8 soft decisions.  The
// reference's own ViterbiDecoder.decode is a stub and has no entry here.
//
// Arguments are checked, with a message, before any device work.  The host
// entries know the lengths and refuse a bad one by stream index; the device
// entry's lengths live in HBM, so there a bad length costs only that stream
// (out_len 0, metric -1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "viterbi.h"

using namespace amr;

namespace {

const char* err_name(hipError_t e) { return hipGetErrorString(e); }

int hip_fail(const char* who, hipError_t e) {
  return fail(e == hipErrorOutOfMemory ? AMR_E_NOMEM : AMR_E_HIP, std::string(who) + ": " + err_name(e));
}

}  // namespace

extern "C" {

int64_t amr_conv_encoded_len(int64_t n_bytes) {
  if (n_bytes < 0) return fail(AMR_E_INVALID, "amr_conv_encoded_len: n_bytes < 0");
  if (n_bytes > (INT64_MAX - 2) / 2) return fail(AMR_E_INVALID, "amr_conv_encoded_len: n_bytes too large");
  return 2 * n_bytes + 2;
}

int64_t amr_viterbi_work_bytes(int64_t in_stride, int64_t n) {
  if (in_stride < 0 || n < 0) return fail(AMR_E_INVALID, "amr_viterbi_work_bytes: negative argument");
  const int64_t per = vit_work_words(in_stride) * 8;
  if (per > 0 && n > INT64_MAX / per) return fail(AMR_E_INVALID, "amr_viterbi_work_bytes: size overflows");
  return per * n;
}

int amr_conv_encode_host(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                         int64_t out_stride, int64_t* out_len) {
  if (n < 0 || in_stride < 0 || out_stride < 0) return fail(AMR_E_INVALID, "amr_conv_encode_host: negative argument");
  if (n == 0) return AMR_OK;
  if (!in_len || !out_len || !out) return fail(AMR_E_INVALID, "amr_conv_encode_host: NULL buffer");
  int64_t nmax = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (in_len[i] < 0 || in_len[i] > in_stride)
      return fail(AMR_E_INVALID, "amr_conv_encode_host: stream " + std::to_string(i) + ": length " +
                                     std::to_string(in_len[i]) + " outside [0, in_stride]");
    nmax = std::max(nmax, in_len[i]);
  }
  if (nmax > 0 && !in) return fail(AMR_E_INVALID, "amr_conv_encode_host: NULL buffer");
  const int64_t lmax = 2 * nmax + 2;
  if (out_stride < lmax) return fail(AMR_E_INVALID, "amr_conv_encode_host: out_stride < 2 * longest message + 2");
  if (n > ((int64_t)0x7fffffff * 256) / lmax)
    return fail(AMR_E_INVALID, "amr_conv_encode_host: messages x coded bytes exceeds one launch");
  const int64_t istr = std::max<int64_t>(nmax, 1);
  const auto bad = [](hipError_t e) { return hip_fail("amr_conv_encode_host", e); };
  DevBuf d_in, d_out, d_len;
  HIP_TRY_ELSE(d_in.reserve(n * istr, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(n * lmax, nullptr), bad);
  HIP_TRY_ELSE(d_len.reserve(n * 8, nullptr), bad);
  if (nmax > 0) HIP_TRY_ELSE(memcpy_rows(d_in.get(), istr, in, in_stride, nmax, n, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(hipMemcpy(d_len.get(), in_len, (size_t)n * 8, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(launch_conv_encode(d_in.as<uint8_t>(), istr, d_len.as<int64_t>(), n, d_out.as<uint8_t>(), lmax, lmax,
                                  nullptr), bad);
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  std::vector<uint8_t> tmp((size_t)(n * lmax));
  HIP_TRY_ELSE(hipMemcpy(tmp.data(), d_out.get(), tmp.size(), hipMemcpyDeviceToHost), bad);
  for (int64_t i = 0; i < n; ++i) {                // only the codeword's own bytes reach the caller's row
    out_len[i] = 2 * in_len[i] + 2;
    std::memcpy(out + i * out_stride, tmp.data() + i * lmax, (size_t)out_len[i]);
  }
  return AMR_OK;
}

int amr_viterbi_decode_device(amr_psk_plan* plan, const uint8_t* d_in, int64_t in_stride, const int64_t* d_in_len,
                              int64_t n, uint8_t* d_out, int64_t out_stride, int64_t* d_out_len, int32_t* d_metric,
                              void* d_work, int64_t work_bytes) {
  if (n < 0 || in_stride < 0 || out_stride < 0)
    return fail(AMR_E_INVALID, "amr_viterbi_decode_device: negative argument");
  if (n == 0) return AMR_OK;
  if (!d_in_len || !d_out_len || !d_metric) return fail(AMR_E_INVALID, "amr_viterbi_decode_device: NULL buffer");
  const int64_t lmax = vit_max_len(in_stride);     // the longest codeword a row can hold
  const int64_t nmax = lmax ? vit_msg_len(lmax) : 0;
  if ((lmax > 0 && !d_in) || (nmax > 0 && !d_out))
    return fail(AMR_E_INVALID, "amr_viterbi_decode_device: NULL buffer");
  if (out_stride < nmax)
    return fail(AMR_E_INVALID, "amr_viterbi_decode_device: out_stride < in_stride / 2 - 1 (the longest message a row holds)");
  if (n > (int64_t)0x7fffffff * (kVitThreads / 64))
    return fail(AMR_E_INVALID, "amr_viterbi_decode_device: codewords exceed one launch");
  const int64_t need = amr_viterbi_work_bytes(in_stride, n);
  if (need < 0) return (int)need;
  if (need > 0 && (!d_work || work_bytes < need))
    return fail(AMR_E_INVALID, "amr_viterbi_decode_device: work buffer smaller than amr_viterbi_work_bytes()");
  int dev = 0;
  hipStream_t st = nullptr;
  const int rc = plan_stream(plan, &dev, &st);
  if (rc) return rc;
  HIP_TRY(launch_viterbi(d_in, in_stride, d_in_len, n, d_out, out_stride, d_out_len, d_metric, d_work, st));
  return AMR_OK;
}

int amr_viterbi_decode_host(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                            int64_t out_stride, int64_t* out_len, int32_t* metric) {
  if (n < 0 || in_stride < 0 || out_stride < 0)
    return fail(AMR_E_INVALID, "amr_viterbi_decode_host: negative argument");
  if (n == 0) return AMR_OK;
  if (!in || !in_len || !out_len || !metric) return fail(AMR_E_INVALID, "amr_viterbi_decode_host: NULL buffer");
  int64_t lmax = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (!vit_is_codeword_len(in_len[i]) || in_len[i] > in_stride)
      return fail(AMR_E_INVALID, "amr_viterbi_decode_host: stream " + std::to_string(i) + ": length " +
                                     std::to_string(in_len[i]) +
                                     " is not a codeword length (even, 2 .. 2^24, <= in_stride)");
    lmax = std::max(lmax, in_len[i]);
  }
  const int64_t nmax = vit_msg_len(lmax);
  if (nmax > 0 && !out) return fail(AMR_E_INVALID, "amr_viterbi_decode_host: NULL buffer");
  if (out_stride < nmax) return fail(AMR_E_INVALID, "amr_viterbi_decode_host: out_stride < longest message");
  // the survivor workspace is 512 bytes per 64 steps and codeword: decode in chunks that keep it under the budget
  const int64_t per = vit_work_words(lmax) * 8;
  const int64_t chunk = std::min(n, std::max<int64_t>(1, kVitWorkBudget / per));
  const int64_t ocap = std::max<int64_t>(nmax, 1);
  const auto bad = [](hipError_t e) { return hip_fail("amr_viterbi_decode_host", e); };
  DevBuf d_in, d_out, d_len, d_olen, d_met, d_work;
  HIP_TRY_ELSE(d_in.reserve(chunk * lmax, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(chunk * ocap, nullptr), bad);
  HIP_TRY_ELSE(d_len.reserve(chunk * 8, nullptr), bad);
  HIP_TRY_ELSE(d_olen.reserve(chunk * 8, nullptr), bad);
  HIP_TRY_ELSE(d_met.reserve(chunk * 4, nullptr), bad);
  HIP_TRY_ELSE(d_work.reserve(chunk * per, nullptr), bad);
  std::vector<uint8_t> tmp((size_t)(chunk * ocap));
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t m = std::min(chunk, n - c0);
    HIP_TRY_ELSE(memcpy_rows(d_in.get(), lmax, in + c0 * in_stride, in_stride, lmax, m, hipMemcpyHostToDevice), bad);
    HIP_TRY_ELSE(hipMemcpy(d_len.get(), in_len + c0, (size_t)m * 8, hipMemcpyHostToDevice), bad);
    const int rc = amr_viterbi_decode_device(nullptr, d_in.as<uint8_t>(), lmax, d_len.as<int64_t>(), m,
                                             d_out.as<uint8_t>(), ocap, d_olen.as<int64_t>(), d_met.as<int32_t>(),
                                             d_work.get(), m * per);
    if (rc) return rc;
    HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
    HIP_TRY_ELSE(hipMemcpy(out_len + c0, d_olen.get(), (size_t)m * 8, hipMemcpyDeviceToHost), bad);
    HIP_TRY_ELSE(hipMemcpy(metric + c0, d_met.get(), (size_t)m * 4, hipMemcpyDeviceToHost), bad);
    if (nmax > 0) HIP_TRY_ELSE(hipMemcpy(tmp.data(), d_out.get(), (size_t)(m * ocap), hipMemcpyDeviceToHost), bad);
    for (int64_t i = 0; i < m; ++i)                // only the decoded bytes reach the caller's row
      if (out_len[c0 + i] > 0)
        std::memcpy(out + (c0 + i) * out_stride, tmp.data() + i * ocap, (size_t)out_len[c0 + i]);
  }
  return AMR_OK;
}

// ---- soft input (k_viterbi_soft) ------------------------------------
int64_t amr_viterbi_soft_work_bytes(int64_t in_stride_vals, int64_t n) {
  if (in_stride_vals < 0 || n < 0) return fail(AMR_E_INVALID, "amr_viterbi_soft_work_bytes: negative argument");
  const int64_t per = vit_soft_work_words(in_stride_vals) * 8;
  if (per > 0 && n > INT64_MAX / per) return fail(AMR_E_INVALID, "amr_viterbi_soft_work_bytes: size overflows");
  return per * n;
}

int amr_viterbi_decode_soft_device(amr_psk_plan* plan, const int8_t* d_in, int64_t in_stride, int64_t in_offset,
                                   const int64_t* d_in_len, int64_t n, uint8_t* d_out, int64_t out_stride,
                                   int64_t* d_out_len, int32_t* d_metric, void* d_work, int64_t work_bytes) {
  if (n < 0 || in_stride < 0 || in_offset < 0 || out_stride < 0)
    return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: negative argument");
  if (n == 0) return AMR_OK;
  if (!d_in_len || !d_out_len || !d_metric) return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: NULL buffer");
  if (in_offset > in_stride) return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: in_offset > in_stride");
  const int64_t tmax = vit_soft_max_steps(in_stride - in_offset);   // the longest row the stride holds past the offset
  const int64_t nmax = tmax ? (tmax - 6) / 8 : 0;
  if ((tmax > 0 && !d_in) || (nmax > 0 && !d_out))
    return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: NULL buffer");
  if (out_stride < nmax)
    return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: out_stride < the longest message a row holds");
  if (n > (int64_t)0x7fffffff * (kVitThreads / 64))
    return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: codewords exceed one launch");
  if (in_stride > 0 && n > INT64_MAX / in_stride)
    return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: size overflows");
  const int64_t need = amr_viterbi_soft_work_bytes(in_stride, n);
  if (need < 0) return (int)need;
  if (need > 0 && (!d_work || work_bytes < need))
    return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_device: work buffer smaller than amr_viterbi_soft_work_bytes()");
  int dev = 0;
  hipStream_t st = nullptr;
  const int rc = plan_stream(plan, &dev, &st);
  if (rc) return rc;
  HIP_TRY(launch_viterbi_soft(d_in, in_stride, in_offset, d_in_len, n, d_out, out_stride, d_out_len, d_metric, d_work,
                              st));
  return AMR_OK;
}

int amr_viterbi_decode_soft_host(const int8_t* in, int64_t in_stride, int64_t in_offset, const int64_t* in_len,
                                 int64_t n, uint8_t* out, int64_t out_stride, int64_t* out_len, int32_t* metric) {
  if (n < 0 || in_stride < 0 || in_offset < 0 || out_stride < 0)
    return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_host: negative argument");
  if (n == 0) return AMR_OK;
  if (!in || !in_len || !out_len || !metric) return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_host: NULL buffer");
  if (in_offset > in_stride) return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_host: in_offset > in_stride");
  int64_t vmax = 0, tmax = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t t = vit_soft_steps(in_len[i]);
    if (t == 0 || in_len[i] > in_stride - in_offset)
      return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_host: stream " + std::to_string(i) + ": length " +
                                     std::to_string(in_len[i]) +
                                     " is not a soft row length (16 k + 12, or 16 k >= 16; <= 2^21 - 4 and the stride)");
    vmax = std::max(vmax, in_len[i]);
    tmax = std::max(tmax, t);
  }
  const int64_t nmax = (tmax - 6) / 8;
  if (nmax > 0 && !out) return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_host: NULL buffer");
  if (out_stride < nmax) return fail(AMR_E_INVALID, "amr_viterbi_decode_soft_host: out_stride < longest message");
  // the device rows hold the values past the offset alone; chunks keep the survivor workspace under the budget
  const int64_t per = vit_soft_work_words(vmax) * 8;
  const int64_t chunk = std::min(n, std::max<int64_t>(1, kVitWorkBudget / per));
  const int64_t ocap = std::max<int64_t>(nmax, 1);
  const auto bad = [](hipError_t e) { return hip_fail("amr_viterbi_decode_soft_host", e); };
  DevBuf d_in, d_out, d_len, d_olen, d_met, d_work;
  HIP_TRY_ELSE(d_in.reserve(chunk * vmax, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(chunk * ocap, nullptr), bad);
  HIP_TRY_ELSE(d_len.reserve(chunk * 8, nullptr), bad);
  HIP_TRY_ELSE(d_olen.reserve(chunk * 8, nullptr), bad);
  HIP_TRY_ELSE(d_met.reserve(chunk * 4, nullptr), bad);
  HIP_TRY_ELSE(d_work.reserve(chunk * per, nullptr), bad);
  std::vector<uint8_t> tmp((size_t)(chunk * ocap));
  for (int64_t c0 = 0; c0 < n; c0 += chunk) {
    const int64_t m = std::min(chunk, n - c0);
    HIP_TRY_ELSE(memcpy_rows(d_in.get(), vmax, in + c0 * in_stride + in_offset, in_stride, vmax, m,
                             hipMemcpyHostToDevice), bad);
    HIP_TRY_ELSE(hipMemcpy(d_len.get(), in_len + c0, (size_t)m * 8, hipMemcpyHostToDevice), bad);
    const int rc = amr_viterbi_decode_soft_device(nullptr, d_in.as<int8_t>(), vmax, 0, d_len.as<int64_t>(), m,
                                                  d_out.as<uint8_t>(), ocap, d_olen.as<int64_t>(),
                                                  d_met.as<int32_t>(), d_work.get(), m * per);
    if (rc) return rc;
    HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
    HIP_TRY_ELSE(hipMemcpy(out_len + c0, d_olen.get(), (size_t)m * 8, hipMemcpyDeviceToHost), bad);
    HIP_TRY_ELSE(hipMemcpy(metric + c0, d_met.get(), (size_t)m * 4, hipMemcpyDeviceToHost), bad);
    if (nmax > 0) HIP_TRY_ELSE(hipMemcpy(tmp.data(), d_out.get(), (size_t)(m * ocap), hipMemcpyDeviceToHost), bad);
    for (int64_t i = 0; i < m; ++i)                // only the decoded bytes reach the caller's row
      if (out_len[c0 + i] > 0)
        std::memcpy(out + (c0 + i) * out_stride, tmp.data() + i * ocap, (size_t)out_len[c0 + i]);
  }
  return AMR_OK;
}

}  // extern "C"
