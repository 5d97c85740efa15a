// rs_api.cpp -- C ABI of the Reed-Solomon code (include/amr.h): the
// batched systematic encoder and the errors-and-erasures decoder of
// fec.ReedSolomonCodec.  The reference's "Reed-Solomon" is the parity stub of
// fec.ReedSolomonFEC (amr_fec_decode_host) and has no part in this file.
//
// Arguments are checked, with a message, before any device work.  The host
// entries know the lengths and refuse a bad one by row index; the device
// entries' lengths live in HBM, so there a bad length costs only that row
// (decode: out_len 0, corrected 0, failed -1; encode: out_len -1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "rs.h"

using namespace amr;

namespace {

int hip_fail(const char* who, hipError_t e) {
  return fail(e == hipErrorOutOfMemory ? AMR_E_NOMEM : AMR_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

// the code's two parameters; 0 or the failure's code
int check_code(const char* who, int nsym, int interleave) {
  if (nsym < kRsMinSym || nsym > kRsMaxSym)
    return fail(AMR_E_INVALID, std::string(who) + ": nsym " + std::to_string(nsym) + " outside [2, 64]");
  if (interleave < 1 || interleave > kRsMaxInterleave)
    return fail(AMR_E_INVALID, std::string(who) + ": interleave " + std::to_string(interleave) + " outside [1, 64]");
  return 0;
}

constexpr int64_t kRsMaxWaves = (int64_t)0x7fffffff * (kRsThreads / 64);

}  // namespace

extern "C" {

int64_t amr_rs_encoded_len(int64_t n, int nsym) {
  if (nsym < kRsMinSym || nsym > kRsMaxSym) return fail(AMR_E_INVALID, "amr_rs_encoded_len: nsym outside [2, 64]");
  if (n < 0) return fail(AMR_E_INVALID, "amr_rs_encoded_len: n < 0");
  if (n > INT64_MAX / 2) return fail(AMR_E_INVALID, "amr_rs_encoded_len: n too large");
  return rs_encoded_len(n, nsym);
}

int64_t amr_rs_decoded_len(int64_t L, int nsym) {
  if (nsym < kRsMinSym || nsym > kRsMaxSym) return fail(AMR_E_INVALID, "amr_rs_decoded_len: nsym outside [2, 64]");
  if (L < 0 || L > INT64_MAX / 2 || !rs_valid_len(L, nsym)) return -1;
  return rs_decoded_len(L, nsym);
}

int amr_rs_encode_device(amr_psk_plan* plan, const uint8_t* d_in, int64_t in_stride, const int64_t* d_in_len,
                         int64_t n, int nsym, int interleave, uint8_t* d_out, int64_t out_stride,
                         int64_t* d_out_len) {
  if (n < 0 || in_stride < 0 || out_stride < 0) return fail(AMR_E_INVALID, "amr_rs_encode_device: negative argument");
  if (const int rc = check_code("amr_rs_encode_device", nsym, interleave)) return rc;
  if (n == 0) return AMR_OK;
  if (!d_in_len || !d_out_len || (in_stride > 0 && (!d_in || !d_out)))
    return fail(AMR_E_INVALID, "amr_rs_encode_device: NULL buffer");
  if (in_stride > INT64_MAX / 2 || out_stride < rs_encoded_len(in_stride, nsym))
    return fail(AMR_E_INVALID, "amr_rs_encode_device: out_stride < amr_rs_encoded_len(in_stride) (the longest row)");
  if (n > kRsMaxWaves / std::max<int64_t>(1, rs_ceil_div(in_stride, kRsN - nsym)))
    return fail(AMR_E_INVALID, "amr_rs_encode_device: rows x blocks exceed one launch");
  int dev = 0;
  hipStream_t st = nullptr;
  const int rc = plan_stream(plan, &dev, &st);
  if (rc) return rc;
  HIP_TRY(launch_rs_encode(d_in, in_stride, d_in_len, n, nsym, interleave, d_out, out_stride, d_out_len, st));
  return AMR_OK;
}

int amr_rs_decode_device(amr_psk_plan* plan, const uint8_t* d_in, int64_t in_stride, const int64_t* d_in_len,
                         const uint8_t* d_erase, int64_t n, int nsym, int interleave, uint8_t* d_out,
                         int64_t out_stride, int64_t* d_out_len, int32_t* d_corrected, int32_t* d_failed) {
  if (n < 0 || in_stride < 0 || out_stride < 0) return fail(AMR_E_INVALID, "amr_rs_decode_device: negative argument");
  if (const int rc = check_code("amr_rs_decode_device", nsym, interleave)) return rc;
  if (n == 0) return AMR_OK;
  if (!d_in_len || !d_out_len || !d_corrected || !d_failed)
    return fail(AMR_E_INVALID, "amr_rs_decode_device: NULL buffer");
  const int64_t lmax = rs_max_len(in_stride, nsym);                // the longest received row the stride holds
  const int64_t nmax = rs_decoded_len(lmax, nsym);
  if ((lmax > 0 && !d_in) || (nmax > 0 && !d_out)) return fail(AMR_E_INVALID, "amr_rs_decode_device: NULL buffer");
  if (out_stride < nmax)
    return fail(AMR_E_INVALID, "amr_rs_decode_device: out_stride < the longest message a row of in_stride holds");
  if (n > kRsMaxWaves / std::max<int64_t>(1, rs_ceil_div(in_stride, kRsN)))
    return fail(AMR_E_INVALID, "amr_rs_decode_device: rows x blocks exceed one launch");
  int dev = 0;
  hipStream_t st = nullptr;
  const int rc = plan_stream(plan, &dev, &st);
  if (rc) return rc;
  HIP_TRY(launch_rs_decode(d_in, in_stride, d_in_len, d_erase, n, nsym, interleave, d_out, out_stride, d_out_len,
                           d_corrected, d_failed, st));
  return AMR_OK;
}

int amr_rs_encode_host(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, int nsym,
                       int interleave, uint8_t* out, int64_t out_stride, int64_t* out_len) {
  if (n < 0 || in_stride < 0 || out_stride < 0) return fail(AMR_E_INVALID, "amr_rs_encode_host: negative argument");
  if (const int rc = check_code("amr_rs_encode_host", nsym, interleave)) return rc;
  if (n == 0) return AMR_OK;
  if (!in_len || !out_len) return fail(AMR_E_INVALID, "amr_rs_encode_host: NULL buffer");
  int64_t nmax = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (in_len[i] < 0 || in_len[i] > in_stride)
      return fail(AMR_E_INVALID, "amr_rs_encode_host: row " + std::to_string(i) + ": length " +
                                     std::to_string(in_len[i]) + " outside [0, in_stride]");
    nmax = std::max(nmax, in_len[i]);
  }
  if (nmax > 0 && (!in || !out)) return fail(AMR_E_INVALID, "amr_rs_encode_host: NULL buffer");
  if (nmax > INT64_MAX / 2) return fail(AMR_E_INVALID, "amr_rs_encode_host: size overflows");
  const int64_t lmax = rs_encoded_len(nmax, nsym);
  if (out_stride < lmax)
    return fail(AMR_E_INVALID, "amr_rs_encode_host: out_stride < amr_rs_encoded_len(longest message)");
  const int64_t istr = std::max<int64_t>(nmax, 1), ostr = std::max<int64_t>(lmax, 1);
  if (n > INT64_MAX / ostr) return fail(AMR_E_INVALID, "amr_rs_encode_host: size overflows");
  const auto bad = [](hipError_t e) { return hip_fail("amr_rs_encode_host", e); };
  DevBuf d_in, d_out, d_len, d_olen;
  HIP_TRY_ELSE(d_in.reserve(n * istr, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(n * ostr, nullptr), bad);
  HIP_TRY_ELSE(d_len.reserve(n * 8, nullptr), bad);
  HIP_TRY_ELSE(d_olen.reserve(n * 8, nullptr), bad);
  if (nmax > 0) HIP_TRY_ELSE(memcpy_rows(d_in.get(), istr, in, in_stride, nmax, n, hipMemcpyHostToDevice), bad);
  HIP_TRY_ELSE(hipMemcpy(d_len.get(), in_len, (size_t)n * 8, hipMemcpyHostToDevice), bad);
  const int rc = amr_rs_encode_device(nullptr, d_in.as<uint8_t>(), nmax, d_len.as<int64_t>(), n, nsym, interleave,
                                      d_out.as<uint8_t>(), lmax, d_olen.as<int64_t>());
  if (rc) return rc;
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  std::vector<int64_t> olen((size_t)n);
  HIP_TRY_ELSE(hipMemcpy(olen.data(), d_olen.get(), (size_t)n * 8, hipMemcpyDeviceToHost), bad);
  std::vector<uint8_t> tmp((size_t)(n * ostr));
  if (lmax > 0) HIP_TRY_ELSE(hipMemcpy(tmp.data(), d_out.get(), (size_t)(n * lmax), hipMemcpyDeviceToHost), bad);
  for (int64_t i = 0; i < n; ++i) {                // only the codeword's own bytes reach the caller's row
    if (olen[(size_t)i] != rs_encoded_len(in_len[i], nsym))
      return fail(AMR_E_HIP, "amr_rs_encode_host: row " + std::to_string(i) + ": the kernel refused a checked length");
    out_len[i] = olen[(size_t)i];
    if (out_len[i] > 0) std::memcpy(out + i * out_stride, tmp.data() + i * lmax, (size_t)out_len[i]);
  }
  return AMR_OK;
}

int amr_rs_decode_host(const uint8_t* in, int64_t in_stride, const int64_t* in_len, const uint8_t* erase, int64_t n,
                       int nsym, int interleave, uint8_t* out, int64_t out_stride, int64_t* out_len,
                       int32_t* corrected, int32_t* failed) {
  if (n < 0 || in_stride < 0 || out_stride < 0) return fail(AMR_E_INVALID, "amr_rs_decode_host: negative argument");
  if (const int rc = check_code("amr_rs_decode_host", nsym, interleave)) return rc;
  if (n == 0) return AMR_OK;
  if (!in_len || !out_len || !corrected || !failed) return fail(AMR_E_INVALID, "amr_rs_decode_host: NULL buffer");
  int64_t lmax = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (in_len[i] < 0 || in_len[i] > in_stride || !rs_valid_len(in_len[i], nsym))
      return fail(AMR_E_INVALID, "amr_rs_decode_host: row " + std::to_string(i) + ": length " +
                                     std::to_string(in_len[i]) +
                                     " is not a received length (0, or a last block of at least nsym + 1 bytes; <= in_stride)");
    lmax = std::max(lmax, in_len[i]);
  }
  const int64_t nmax = rs_decoded_len(lmax, nsym);
  if ((lmax > 0 && !in) || (nmax > 0 && !out)) return fail(AMR_E_INVALID, "amr_rs_decode_host: NULL buffer");
  if (out_stride < nmax) return fail(AMR_E_INVALID, "amr_rs_decode_host: out_stride < longest message");
  const int64_t istr = std::max<int64_t>(lmax, 1), ocap = std::max<int64_t>(nmax, 1);
  if (n > INT64_MAX / istr) return fail(AMR_E_INVALID, "amr_rs_decode_host: size overflows");
  const auto bad = [](hipError_t e) { return hip_fail("amr_rs_decode_host", e); };
  DevBuf d_in, d_er, d_out, d_len, d_olen, d_cor, d_fail;
  HIP_TRY_ELSE(d_in.reserve(n * istr, nullptr), bad);
  if (erase) HIP_TRY_ELSE(d_er.reserve(n * istr, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(n * ocap, nullptr), bad);
  HIP_TRY_ELSE(d_len.reserve(n * 8, nullptr), bad);
  HIP_TRY_ELSE(d_olen.reserve(n * 8, nullptr), bad);
  HIP_TRY_ELSE(d_cor.reserve(n * 4, nullptr), bad);
  HIP_TRY_ELSE(d_fail.reserve(n * 4, nullptr), bad);
  if (lmax > 0) {
    HIP_TRY_ELSE(memcpy_rows(d_in.get(), istr, in, in_stride, lmax, n, hipMemcpyHostToDevice), bad);
    if (erase) HIP_TRY_ELSE(memcpy_rows(d_er.get(), istr, erase, in_stride, lmax, n, hipMemcpyHostToDevice), bad);
  }
  HIP_TRY_ELSE(hipMemcpy(d_len.get(), in_len, (size_t)n * 8, hipMemcpyHostToDevice), bad);
  const int rc = amr_rs_decode_device(nullptr, d_in.as<uint8_t>(), lmax, d_len.as<int64_t>(),
                                      erase && lmax > 0 ? d_er.as<uint8_t>() : nullptr, n, nsym, interleave,
                                      d_out.as<uint8_t>(), nmax, d_olen.as<int64_t>(), d_cor.as<int32_t>(),
                                      d_fail.as<int32_t>());
  if (rc) return rc;
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  HIP_TRY_ELSE(hipMemcpy(out_len, d_olen.get(), (size_t)n * 8, hipMemcpyDeviceToHost), bad);
  HIP_TRY_ELSE(hipMemcpy(corrected, d_cor.get(), (size_t)n * 4, hipMemcpyDeviceToHost), bad);
  HIP_TRY_ELSE(hipMemcpy(failed, d_fail.get(), (size_t)n * 4, hipMemcpyDeviceToHost), bad);
  std::vector<uint8_t> tmp((size_t)(n * ocap));
  if (nmax > 0) HIP_TRY_ELSE(hipMemcpy(tmp.data(), d_out.get(), (size_t)(n * nmax), hipMemcpyDeviceToHost), bad);
  for (int64_t i = 0; i < n; ++i)                  // only the decoded bytes reach the caller's row
    if (out_len[i] > 0) std::memcpy(out + i * out_stride, tmp.data() + i * nmax, (size_t)out_len[i]);
  return AMR_OK;
}

}  // extern "C"
