// ofdm.h -- the multi-carrier DQPSK modem: what
// ofdm_kernels.hip, ofdm_acq_kernels.hip and ofdm_api.cpp share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amr {

constexpr int kOfdmMaxK = 64;

// One plan's geometry, by value into the kernels
struct OfdmParams {
  int64_t n;          // samples per stream
  int64_t sps;        // int(samp_rate / baud)
  int64_t L;          // K * sps: samples per OFDM symbol
  int64_t ncp;        // L / 8: cyclic prefix
  int64_t nu;         // L - ncp: useful samples (the DFT length)
  int64_t n_sym;      // S = n / L
  int64_t n_bits;     // 2 K (S - 1), 0 when S < 2
  int64_t n_words;    // 32-bit words per stream in the bit buffer (>= 1)
  int K;              // subcarriers
  int bin0;           // bins[k] = bin0 + k
};

// n_sym, n_bits, n_words of `p` from n, K, L (host and device)
inline void ofdm_counts(OfdmParams& p) {
  p.n_sym = p.L > 0 ? p.n / p.L : 0;
  p.n_bits = p.n_sym >= 2 ? 2 * (int64_t)p.K * (p.n_sym - 1) : 0;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
}

// W: device table [nu][K][2] (re, im) -- the caller's [K][nu][2] transposed,
// so that a group of subcarriers at one m is one contiguous uniform load
hipError_t launch_ofdm_dft(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const OfdmParams& p,
                           const double* W, double* Y, hipStream_t st);
hipError_t launch_ofdm_slice(const double* Y, int64_t n_streams, const OfdmParams& p, uint32_t* words,
                             hipStream_t st);
// after launch_sync_pack on the same stream (sync_idx / out_len; both null: every bit from 0)
hipError_t launch_ofdm_soft(const double* Y, int64_t n_streams, const OfdmParams& p, const uint32_t* words,
                            const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                            hipStream_t st);

// ---- acquisition (ofdm_acq_kernels.hip) -----------------------
constexpr int kAcqSeg = 64;   // periods per segment of the fold
// M = (n - Nu) / L periods take part in the fold (0 when n < Nu + L); its segments
inline int64_t ofdm_acq_periods(const OfdmParams& p) { return p.n >= p.nu + p.L ? (p.n - p.nu) / p.L : 0; }
inline int64_t ofdm_acq_segments(const OfdmParams& p) { return (ofdm_acq_periods(p) + kAcqSeg - 1) / kAcqSeg; }
// the plan's work buffers of one acquiring call, all device memory
struct OfdmAcq {
  double* gq;         // [n_streams][segments][L]: the fold's partial sums
  double* G;          // [n_streams][L]
  double* E;          // [n_streams][L]
  int64_t* dhat;      // [n_streams]: the first minimum of E
  int64_t* offset;    // [n_streams]: dhat backed off by Ncp / 2, in [-Ncp, L - 1 - Ncp]
};
// fold, segment sum, window sum, first minimum and back-off of every stream
hipError_t launch_ofdm_acquire(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const OfdmParams& p,
                               const OfdmAcq& a, hipStream_t st);
// launch_ofdm_dft with stream b read from sample offset[b] on (device array, each
// value in [-Ncp, L - 1 - Ncp]); samples at or past n count as 0.0 and are not loaded
hipError_t launch_ofdm_dft_at(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const OfdmParams& p,
                              const double* W, const int64_t* offset, double* Y, hipStream_t st);

// transmit: one modulate call
struct OfdmTx {
  int64_t L, ncp, nu;
  int64_t n_out;        // samples written per stream
  int64_t sym_stride;   // symbols' phases kept per stream
  int K;
  int bin0;
};
// symbols of an n_bytes payload: 1 + ceil((40 + 4 n_bytes) / K)
__host__ __device__ inline int64_t ofdm_tx_symbols(int64_t nb, int K) { return 1 + (40 + 4 * nb + K - 1) / K; }
// phase: [n_streams][sym_stride][K] doubles of work
hipError_t launch_ofdm_tx(const OfdmTx& t, const uint8_t* data, int64_t stride, const int64_t* n_bytes,
                          int64_t n_streams, double* phase, float* out, int64_t out_stride, int16_t* pcm,
                          int64_t pcm_stride, hipStream_t st);

}  // namespace amr
