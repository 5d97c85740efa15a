// dsss.h -- spread, the direct-sequence DBPSK modem: what
// dsss_kernels.hip, dsss_acq_kernels.hip and dsss_api.cpp share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amr {

constexpr int kDsssMaxC = 64;

// One plan's geometry, by value into the kernels
struct DsssParams {
  int64_t n;          // samples per stream
  int64_t spc;        // int(samp_rate / baud): samples per chip
  int64_t L;          // C * spc: samples per bit
  int64_t n_sym;      // S = n / L
  int64_t n_bits;     // S - 1, 0 when S < 2
  int64_t n_words;    // 32-bit words per stream in the bit buffer (>= 1)
  int C;              // chips per bit
};

inline void dsss_counts(DsssParams& p) {
  p.n_sym = p.L > 0 ? p.n / p.L : 0;
  p.n_bits = p.n_sym >= 2 ? p.n_sym - 1 : 0;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
}

// T: device table [L][2] (sg * cos th, -sg * sin th).  offset: device array
// [n_streams] of values in [0, L - 1], or null for zeros; stream b's bit s is
// read from sample offset[b] + s*L on, samples at or past n count as 0.0 and
// are not loaded.  Y [n_streams][S][2].
hipError_t launch_dsss_despread(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const DsssParams& p,
                                const double* T, const int64_t* offset, double* Y, hipStream_t st);
hipError_t launch_dsss_slice(const double* Y, int64_t n_streams, const DsssParams& p, uint32_t* words,
                             hipStream_t st);
// after launch_sync_pack on the same stream (sync_idx / out_len; both null: every bit from 0)
hipError_t launch_dsss_soft(const double* Y, int64_t n_streams, const DsssParams& p, const uint32_t* words,
                            const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                            hipStream_t st);

// ---- acquisition (dsss_acq_kernels.hip) -------------------------------------
constexpr int kDsssSeg = 64;    // bits per segment of the energy sum
// M = (n - L + 1) / L bits take part (0 when n < 2 L - 1); its segments
inline int64_t dsss_acq_bits(const DsssParams& p) { return p.n >= 2 * p.L - 1 ? (p.n - p.L + 1) / p.L : 0; }
inline int64_t dsss_acq_segments(const DsssParams& p) { return (dsss_acq_bits(p) + kDsssSeg - 1) / kDsssSeg; }
// the plan's work buffers of one acquiring call, all device memory
struct DsssAcq {
  double* gq;         // [n_streams][segments][L]: the segments' energy sums
  double* P;          // [n_streams][L]
  int64_t* offset;    // [n_streams]: the first maximum of P
};
// Wc [L][2] (cos th, -sin th), cs [C] (+-1.0): chip sums, code correlation,
// energy, segment sum and first maximum of every stream
hipError_t launch_dsss_acquire(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const DsssParams& p,
                               const double* Wc, const double* cs, const DsssAcq& a, hipStream_t st);

// ---- transmit ------------------------------------------------------------------
struct DsssTx {
  int64_t spc, L;
  int64_t n_out;        // samples written per stream
  int64_t sym_stride;   // symbol signs kept per stream
  int C;
};
// symbols of an n_bytes payload: the reference symbol, 80 preamble bits, the payload's
__host__ __device__ inline int64_t dsss_tx_symbols(int64_t nb) { return 81 + 8 * nb; }
// tab: device [L] doubles, sg[i] * Sn[i]; sign: [n_streams][sym_stride] int8 of work
hipError_t launch_dsss_tx(const DsssTx& t, const double* tab, const uint8_t* data, int64_t stride,
                          const int64_t* n_bytes, int64_t n_streams, int8_t* sign, float* out, int64_t out_stride,
                          int16_t* pcm, int64_t pcm_stride, hipStream_t st);

}  // namespace amr
