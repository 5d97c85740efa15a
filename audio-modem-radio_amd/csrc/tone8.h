// tone8.h -- tone8, the 8-FSK modem with Costas sync: what
// tone8_kernels.hip, tone8_acq_kernels.hip and tone8_api.cpp share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amr {

constexpr int kTone8MaxSearch = 16;                 // G, half tone spacings either way
constexpr int kTone8Costas = 7;                     // symbols of the Costas block
constexpr int kTone8Span = 8 * (kTone8Costas - 1);  // 48: slots from the first Costas window to the last
constexpr int kTone8Ahead = kTone8Span + 7;         // 55: slots a start slot needs beyond itself
// the acquisition tile: (C + 55) slots x NB lines of complex slot sums fit kTone8Tile entries
// (51 KB, two workgroups per CU beside the 8 KB line table): C = 64 at the default G = 6
constexpr int kTone8Tile = (64 + kTone8Ahead) * 27;
__host__ __device__ inline int64_t tone8_lines(int64_t G) { return 15 + 2 * G; }
__host__ __device__ inline int64_t tone8_chunk(int64_t G) { return kTone8Tile / tone8_lines(G) - kTone8Ahead; }

// One plan's geometry, by value into the kernels
struct Tone8Params {
  int64_t n;          // samples per stream
  int64_t L;          // int(samp_rate / baud): samples per symbol, a multiple of 8
  int64_t T;          // L / 8: samples per time slot
  int64_t c2;         // half-cycles of carrier per symbol; tone m has c2 + 2 m
  int64_t G;          // the search, half tone spacings either way
  int64_t NB;         // 15 + 2 G searched lines, f = c2 - G .. c2 + 14 + G
  int64_t C;          // start slots per acquisition chunk
  int64_t J;          // n / T slots
  int64_t nj;         // max(0, J - 55) start slots
  int64_t n_sym;      // S = n / L symbols
  int64_t n_bits;     // 3 S
  int64_t n_words;    // 32-bit words per stream in the bit buffer (>= 1)
};

inline void tone8_counts(Tone8Params& p) {
  p.T = p.L / 8;
  p.NB = tone8_lines(p.G);
  p.C = tone8_chunk(p.G);
  p.J = p.T > 0 ? p.n / p.T : 0;
  p.nj = p.J > kTone8Ahead ? p.J - kTone8Ahead : 0;
  p.n_sym = p.L > 0 ? p.n / p.L : 0;
  p.n_bits = 3 * p.n_sym;
  p.n_words = p.n_bits > 0 ? (p.n_bits + 31) / 32 : 1;
}
inline int64_t tone8_acq_chunks(const Tone8Params& p) { return (p.nj + p.C - 1) / p.C; }

// E: device table [2 L][2] (cos th, -sin th).  start / shift: device arrays
// [n_streams] or null for zeros; stream b is read from sample start[b] % L on
// with every tone moved by shift[b] (clamped to [-G, G]) half-cycles per
// symbol; samples at or past n count as 0.0 and are not loaded.
// Y [n_streams][S][8][2].
hipError_t launch_tone8_dft(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const Tone8Params& p,
                            const double* E, const int64_t* start, const int64_t* shift, double* Y, hipStream_t st);
// the decision on e_m = re * re + im * im: the first maximum from m = 0, the inverse Gray map, MSB first
hipError_t launch_tone8_slice(const double* Y, int64_t n_streams, const Tone8Params& p, uint32_t* words,
                              hipStream_t st);
// after launch_sync_pack on the same stream (sync_idx / out_len; both null: every bit from 0)
hipError_t launch_tone8_soft(const double* Y, int64_t n_streams, const Tone8Params& p, const uint32_t* words,
                             const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                             hipStream_t st);

// ---- acquisition (tone8_acq_kernels.hip) ----------------------------------------
// a chunk's first maximum: j < 0 when every score of the chunk is NaN; first = the chunk's first score
struct Tone8Cand {
  double score;
  int64_t j, g;
  double first;
};
// cand [n_streams][chunks]; start, shift [n_streams], score [n_streams] or null
hipError_t launch_tone8_acquire(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const Tone8Params& p,
                                const double* E, Tone8Cand* cand, int64_t* start, int64_t* shift, double* score,
                                hipStream_t st);
// the score and maximum stage on given P [n_streams][n_win][15 + 2 G]; cand [n_streams][ceil((n_win - 48) / C)]
hipError_t launch_tone8_peak(const double* P, int64_t n_streams, int64_t n_win, int64_t T, int64_t G, Tone8Cand* cand,
                             int64_t* start, int64_t* shift, double* score, hipStream_t st);

// ---- transmit ------------------------------------------------------------------
struct Tone8Tx {
  int64_t L, c2;
  int64_t n_out;        // samples written per stream
  int64_t sym_stride;   // symbol phases kept per stream
};
// symbols of an n_bytes payload: the Costas block, then a tribit each
__host__ __device__ inline int64_t tone8_tx_syms(int64_t nb) { return kTone8Costas + (8 * nb + 2) / 3; }
// Sn: device [2 L] doubles; ph: [n_streams][sym_stride] uint32 of work (p_k in the low 28 bits, the tone above)
hipError_t launch_tone8_tx(const Tone8Tx& t, const double* Sn, const uint8_t* data, int64_t stride,
                           const int64_t* n_bytes, int64_t n_streams, uint32_t* ph, float* out, int64_t out_stride,
                           int16_t* pcm, int64_t pcm_stride, hipStream_t st);

}  // namespace amr
