// hell_api.cpp -- C ABI of the Hellschreiber receiver (include/amr.h):
// hellschreiber_demodulate (hellschreiber.py:155-187) for a batch of captures.
//
// The host part is the reference's scalar set-up with the same IEEE double
// operations,
//   sps = int(round(samp_rate / baud))      hellschreiber.py:158 (round half even)
//   pixels = len(range(0, n - sps + 1, sps))
// and its error contract: sps == 0 is range()'s ValueError.  The sample work
// is hell_kernels.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "amr_internal.h"
#include "api_common.h"
#include "dev_mem.h"
#include "hell.h"
#include "hell_glyphs.h"

using namespace amr;

namespace {

int64_t elem_size(int elem) {
  switch (elem) {
    case AMR_HELL_ELEM_I8: case AMR_HELL_ELEM_U8: return 1;
    case AMR_HELL_ELEM_F16: case AMR_HELL_ELEM_I16: case AMR_HELL_ELEM_U16: case AMR_HELL_ELEM_PCM16: return 2;
    case AMR_HELL_ELEM_F32: case AMR_HELL_ELEM_I32: case AMR_HELL_ELEM_U32: return 4;
    case AMR_HELL_ELEM_F64: case AMR_HELL_ELEM_I64: case AMR_HELL_ELEM_U64: return 8;
    default: return 0;
  }
}

// int(round(samp_rate / baud)); an AMR_E_* code (message set) where the reference raises
int hell_sps(double baud, double fs, int64_t* sps) {
  if (baud == 0.0) return fail(AMR_E_INVALID, "float division by zero");
  if (!std::isfinite(baud) || !std::isfinite(fs)) return fail(AMR_E_INVALID, "baud and sample_rate must be finite");
  const double r = std::nearbyint(fs / baud);
  if (!(std::fabs(r) < 2147483648.0)) return fail(AMR_E_INVALID, "samples per pixel out of range (>= 2^31)");
  *sps = (int64_t)r;
  if (*sps == 0) return fail(AMR_E_INVALID, "range() arg 3 must not be zero");
  return AMR_OK;
}

}  // namespace

extern "C" {

int64_t amr_hell_pixels(int64_t n_samples, double baud, double sample_rate) {
  if (n_samples < 0) return fail(AMR_E_INVALID, "n_samples < 0");
  int64_t sps = 0;
  const int rc = hell_sps(baud, sample_rate, &sps);
  if (rc) return rc;
  return sps < 0 ? 0 : n_samples / sps;            // a negative step: range() is empty
}

int64_t amr_hell_work_bytes(double baud, double sample_rate) {
  int64_t sps = 0;
  const int rc = hell_sps(baud, sample_rate, &sps);
  if (rc) return rc;
  return hell_work_bytes(sps < 0 ? 0 : sps);
}

int amr_hell_glyph_rows(uint8_t* rows, uint8_t* rx_lookup) {
  if (rows)
    for (int g = 0; g < kHellGlyphs; ++g)
      for (int r = 0; r < kHellRows; ++r) rows[g * kHellRows + r] = kHellGlyphRows[g][r];
  if (rx_lookup) hell_rx_lookup(rx_lookup);
  return kHellGlyphs;
}

int amr_hell_demod_device(amr_psk_plan* plan, const void* d_x, int elem, int64_t n_streams, int64_t x_stride,
                          int64_t n_samples, double baud, double sample_rate, uint8_t* d_out, int64_t out_stride,
                          int64_t* d_out_len, double* d_energy, void* d_work, int64_t work_bytes) {
  if (elem_size(elem) == 0) return fail(AMR_E_INVALID, "amr_hell_demod_device: unknown element type");
  if (n_streams < 0 || n_samples < 0 || x_stride < n_samples || out_stride < 0)
    return fail(AMR_E_INVALID, "amr_hell_demod_device: bad argument");
  int64_t sps = 0;
  int rc = hell_sps(baud, sample_rate, &sps);
  if (rc) return rc;
  if (n_streams == 0) return AMR_OK;
  const int64_t n_pix = sps < 0 ? 0 : n_samples / sps;
  if (!d_out_len || (n_pix > 0 && !d_x) || (n_pix / 7 > 0 && !d_out))
    return fail(AMR_E_INVALID, "amr_hell_demod_device: NULL buffer");
  if (out_stride < n_pix / 7) return fail(AMR_E_INVALID, "amr_hell_demod_device: out_stride < pixels / 7");
  const int64_t groups = (n_pix + 6) / 7;
  if (groups > 0 && n_streams > (int64_t)0x7fffffff * 4 / groups)
    return fail(AMR_E_INVALID, "amr_hell_demod_device: streams x pixel groups exceeds one launch");
  if (n_pix > 0 && (!d_work || work_bytes < hell_work_bytes(sps)))
    return fail(AMR_E_INVALID, "amr_hell_demod_device: work buffer smaller than amr_hell_work_bytes()");
  int dev = 0;
  hipStream_t st = nullptr;
  rc = plan_stream(plan, &dev, &st);
  if (rc) return rc;
  HIP_TRY(launch_hell(elem, d_x, x_stride, n_streams, n_samples, sps < 0 ? 0 : sps, d_out, out_stride, d_out_len,
                      d_energy, d_work, st));
  return AMR_OK;
}

int amr_hell_demod_host(const void* x, int elem, int64_t n_streams, int64_t x_stride, int64_t n_samples, double baud,
                        double sample_rate, uint8_t* out, int64_t out_stride, int64_t* out_len, double* energy) {
  const int64_t es = elem_size(elem);
  if (es == 0) return fail(AMR_E_INVALID, "amr_hell_demod_host: unknown element type");
  if (n_streams < 0 || n_samples < 0 || x_stride < n_samples || out_stride < 0)
    return fail(AMR_E_INVALID, "amr_hell_demod_host: bad argument");
  int64_t sps = 0;
  int rc = hell_sps(baud, sample_rate, &sps);
  if (rc) return rc;
  if (n_streams == 0) return AMR_OK;
  if (!out_len) return fail(AMR_E_INVALID, "amr_hell_demod_host: NULL out_len");
  const int64_t n_pix = sps < 0 ? 0 : n_samples / sps;
  const int64_t n_out = n_pix / 7;
  if (n_pix == 0) {                                  // shorter than one pixel: no device work
    for (int64_t i = 0; i < n_streams; ++i) out_len[i] = 0;
    return AMR_OK;
  }
  if (!x || (n_out > 0 && !out)) return fail(AMR_E_INVALID, "amr_hell_demod_host: NULL buffer");
  if (out_stride < n_out) return fail(AMR_E_INVALID, "amr_hell_demod_host: out_stride < pixels / 7");
  const int64_t used = n_pix * sps;                  // the tail past the last whole pixel stays on the host
  const int64_t wb = hell_work_bytes(sps);
  const int64_t ocap = n_out > 0 ? n_out : 1;
  const auto bad = [](hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? AMR_E_NOMEM : AMR_E_HIP,
                std::string("amr_hell_demod_host: ") + hipGetErrorString(e));
  };
  DevBuf d_x, d_out, d_len, d_en, d_work;
  HIP_TRY_ELSE(d_x.reserve(n_streams * used * es, nullptr), bad);
  HIP_TRY_ELSE(d_out.reserve(n_streams * ocap, nullptr), bad);
  HIP_TRY_ELSE(d_len.reserve(n_streams * 8, nullptr), bad);
  if (energy) HIP_TRY_ELSE(d_en.reserve(n_streams * n_pix * 8, nullptr), bad);
  HIP_TRY_ELSE(d_work.reserve(wb, nullptr), bad);
  HIP_TRY_ELSE(memcpy_rows(d_x.get(), used * es, x, x_stride * es, used * es, n_streams, hipMemcpyHostToDevice), bad);
  rc = amr_hell_demod_device(nullptr, d_x.get(), elem, n_streams, used, used, baud, sample_rate, d_out.as<uint8_t>(),
                             ocap, d_len.as<int64_t>(), d_en.as<double>(), d_work.get(), wb);
  if (rc) return rc;
  HIP_TRY_ELSE(hipDeviceSynchronize(), bad);
  if (n_out > 0)
    HIP_TRY_ELSE(memcpy_rows(out, out_stride, d_out.get(), ocap, n_out, n_streams, hipMemcpyDeviceToHost), bad);
  HIP_TRY_ELSE(hipMemcpy(out_len, d_len.get(), (size_t)n_streams * 8, hipMemcpyDeviceToHost), bad);
  if (energy)
    HIP_TRY_ELSE(hipMemcpy(energy, d_en.get(), (size_t)(n_streams * n_pix) * 8, hipMemcpyDeviceToHost), bad);
  return AMR_OK;
}

}  // extern "C"
