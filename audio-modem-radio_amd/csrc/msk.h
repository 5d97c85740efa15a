// msk.h -- minshift, the MSK modem: what msk_kernels.hip,
// msk_acq_kernels.hip and msk_api.cpp share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amr {

// One plan's geometry, by value into the kernels
struct MskParams {
  int64_t n;          // samples per stream
  int64_t L;          // int(samp_rate / baud): samples per bit
  int64_t h;          // L / 2
  int64_t cyc4;       // quarter-cycles of carrier per bit
  int64_t n_sym;      // Sw = max(0, (n + h) / L - 1) windows
  int64_t n_bits;     // Sw - 1, 0 when Sw < 2
  int64_t n_words;    // 32-bit words per stream in the bit buffer (>= 1)
};

inline void msk_counts(MskParams& p) {
  p.h = p.L / 2;
  const int64_t s = p.L > 0 ? (p.n + p.h) / p.L - 1 : 0;
  p.n_sym = s > 0 ? s : 0;
  p.n_bits = p.n_sym >= 2 ? p.n_sym - 1 : 0;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
}

// U: device table [L][2] (cos th, -sin th).  offset: device array [n_streams]
// of values in [0, L - 1], or null for zeros; stream b's window k is read from
// sample offset[b] + (k + 1) L - h on, samples at or past n count as 0.0 and
// are not loaded.  W [n_streams][Sw][2].
hipError_t launch_msk_corr(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const MskParams& p,
                           const double* U, const int64_t* offset, double* W, hipStream_t st);
// the decision on D[k] = (W[k+1] * conj(W[k])) * (-i)^(cyc4 mod 4)
hipError_t launch_msk_slice(const double* W, int64_t n_streams, const MskParams& p, uint32_t* words, hipStream_t st);
// after launch_sync_pack on the same stream (sync_idx / out_len; both null: every bit from 0)
hipError_t launch_msk_soft(const double* W, int64_t n_streams, const MskParams& p, const uint32_t* words,
                           const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                           hipStream_t st);

// ---- bit timing (msk_acq_kernels.hip) ----------------------------------------
constexpr int kMskSeg = 4096;   // samples per segment of the line sums
inline int64_t msk_acq_segments(int64_t n) { return (n + kMskSeg - 1) / kMskSeg; }
// the plan's work buffers of one acquiring call, all device memory
struct MskAcq {
  double* seg;        // [n_streams][segments][4]: (c0.re, c0.im, c1.re, c1.im) of each segment
  double* q;          // [n_streams][2]
  int64_t* offset;    // [n_streams]: the first maximum of P
};
// E0, E1 [2 L][2] (cos th, -sin th): the segments' line sums
hipError_t launch_msk_lines(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const MskParams& p,
                            const double* E0, const double* E1, double* seg, hipStream_t st);
// R [L][2] (cos, +sin): the segment sums in order, q, P[d] and its first maximum; q may be null
hipError_t launch_msk_acq_max(int64_t L, int64_t segments, int64_t n_streams, const double* seg, const double* R,
                              int64_t* offset, double* q, hipStream_t st);

// ---- transmit ------------------------------------------------------------------
struct MskTx {
  int64_t L, cyc4;
  int64_t n_out;        // samples written per stream
  int64_t bit_stride;   // bit phases kept per stream
};
// bits of an n_bytes payload: the reference bit, 80 preamble bits, the payload's, the closing bit
__host__ __device__ inline int64_t msk_tx_bits(int64_t nb) { return 82 + 8 * nb; }
// Sn: device [4 L] doubles; quad: [n_streams][bit_stride] uint8 of work (p_k / L in the low bits, the bit above)
hipError_t launch_msk_tx(const MskTx& t, const double* Sn, const uint8_t* data, int64_t stride,
                         const int64_t* n_bytes, int64_t n_streams, uint8_t* quad, float* out, int64_t out_stride,
                         int16_t* pcm, int64_t pcm_stride, hipStream_t st);

}  // namespace amr
