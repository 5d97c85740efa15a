// psk8_kernels.hip -- d8psk: the 8-ary differential PSK demodulator's own two
// stages (no reference counterpart -- the reference's "8PSK" is
// a QPSK alias).  The band-pass, mixer, low-pass and symbol sampler are QPSK's
// kernels unchanged; these are the siblings of K4a (psk_kernels.hip k_slice)
// and K4s (psk_soft_kernels.hip k_psk_soft) behind them.
//
// Decision on the differential product d = s[k+1] * conj(s[k]) (the fma form
// K4a evaluates), T = 0x1.a827999fcef32p-2 (the double nearest tan(pi/8)),
// ar = |dr|, ai = |di|, each T * x one rounded product:
//   ai < T*ar        m = dr > 0 ? 0 : 4          (on the real axis)
//   else ar < T*ai   m = di > 0 ? 2 : 6          (on the imaginary axis)
//   else             m = di > 0 ? (dr > 0 ? 1 : 3) : (dr > 0 ? 7 : 5)
// (zeros, NaN and an exact tie reach the last line: the rule is total), and
// the three bits sent are the Gray code m ^ (m >> 1), MSB first.  The bit
// string is contiguous: a tribit may straddle two 32-bit words (product 10
// covers bits 30-32), so the unit of work is 32 products = 96 bits = 3 words.
#include <hip/hip_runtime.h>

#include "psk_common.h"

namespace amr {
namespace {

constexpr double kTanPi8 = 0x1.a827999fcef32p-2;

__device__ __forceinline__ uint32_t d8psk_tribit(double dr, double di) {
  const double ar = fabs(dr), ai = fabs(di);
  uint32_t m;
  if (ai < kTanPi8 * ar) m = dr > 0 ? 0u : 4u;
  else if (ar < kTanPi8 * ai) m = di > 0 ? 2u : 6u;
  else if (di > 0) m = dr > 0 ? 1u : 3u;
  else m = dr > 0 ? 7u : 5u;
  return m ^ (m >> 1);
}

// ---------------------------------------------------------------------------
// K4a8: differential product + 8-sector slicer + bit packing.
// Workgroup = 64 streams x kSlice8Units units of 32 products (3 words each):
// wave w slices units 2w, 2w + 1 of its 64 streams (lane = stream; symbol
// loads are whole 512-B lines through sym_index, the running symbol carried
// from product to product), the words go through LDS and leave as row
// segments of 24 consecutive words per stream, as k_slice's do.
constexpr int kSlice8Units = 8;                     // per workgroup: 256 products, 24 words
constexpr int kSlice8Words = 3 * kSlice8Units;

__global__ __launch_bounds__(256) void k_slice8(PskBuffers buf, PskParams p, int only_flagged) {
  if (buf.gate && *buf.gate == 0) return;   // a gated launch (PskBuffers::gate): whole grid
  constexpr int UPW = kSlice8Units / 4;             // units per wave
  __shared__ uint32_t wl[kWave][kSlice8Words + 1];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.y * kWave + lane;
  const bool live = s < buf.n_streams && (!only_flagged || buf.flags[s] != 0);
  const int64_t S = p.n_sym;
  const int64_t nd = S - 1;                         // number of diffs
  const int64_t u0 = (int64_t)blockIdx.x * kSlice8Units + wv * UPW;   // this wave's first unit
  const double* __restrict__ sym = buf.s1;
  auto SYM = [&](int64_t k) { return make_double2(sym[sym_index(s, S, k, 0)], sym[sym_index(s, S, k, 1)]); };
  double2 prev = make_double2(0.0, 0.0);
  if (live) {
    const int64_t k0 = u0 * 32;
    prev = SYM(k0 < S ? k0 : S - 1);
  }
  for (int q = 0; q < UPW; ++q) {
    const int64_t k0 = (u0 + q) * 32;
    uint32_t w[3] = {0u, 0u, 0u};
    if (live && k0 < nd) {
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        const int64_t k = k0 + u;
        if (k < nd) {
          const double2 nx = SYM(k + 1);
          // diff_k = s_{k+1} * conj(s_k): numpy fma form (see oracle)
          const double br = prev.x, bi = -prev.y;
          const double dr = __builtin_fma(nx.x, br, -(nx.y * bi));
          const double di = __builtin_fma(nx.x, bi, nx.y * br);
          const uint32_t g = d8psk_tribit(dr, di);
          const int o = 3 * u, wi = o >> 5, sh = 29 - (o & 31);   // compile-time after the unroll
          if (sh >= 0) {
            w[wi] |= g << sh;
          } else {                                  // the tribit straddles words wi, wi + 1
            w[wi] |= g >> (-sh);
            w[wi + 1] |= g << (32 + sh);
          }
          prev = nx;
        }
      }
    }
    const int c = (wv * UPW + q) * 3;
    wl[lane][c] = w[0];
    wl[lane][c + 1] = w[1];
    wl[lane][c + 2] = w[2];
  }
  __syncthreads();
  // rows leave whole: 24 consecutive threads write 24 consecutive words of one stream
  const int64_t j0 = (int64_t)blockIdx.x * kSlice8Words;
  for (int idx = threadIdx.x; idx < kWave * kSlice8Words; idx += 256) {
    const int sl = idx / kSlice8Words, jj = idx - sl * kSlice8Words;
    const int64_t ss = (int64_t)blockIdx.y * kWave + sl;
    const int64_t j = j0 + jj;
    if (ss < buf.n_streams && j < p.n_words && (!only_flagged || buf.flags[ss] != 0))
      buf.words[(size_t)ss * p.n_words + j] = wl[sl][jj];
  }
}

// ---------------------------------------------------------------------------
// K4s8: three int8 per product, in bit order b2, b1, b0.  The sign is the hard
// bit read back from the words (as K4s), the magnitude K4s's rule
//   q = floor(num / den * 127.0 + 0.5);  1 unless q >= 1;  127 if q > 127
// with den = |dr| + |di| and, each T * x rounded, then the sum rounded:
//   b2  num = |di + T*dr|         b1  num = |T*di - dr|
//   b0  a = |di - T*dr|, b = |dr + T*di|, num = a < b ? a : b
// -- up to a common factor the distances from each bit's decision lines (b0
// has two pairs of them, so it tops out near 74, not 127).
// Workgroup = 64 streams x kSoft8Tile products; wave w computes products
// w*16 .. w*16+15 of the tile (their 48 hard bits lie in two words of the
// stream's row), the values go through LDS and leave as row segments of 192
// consecutive bytes per stream, inside the sync / out_len window as K4s.
constexpr int kSoft8Tile = 64;                      // products per stream and workgroup
constexpr int kSoft8Pitch = 3 * kSoft8Tile + 4;     // LDS row pitch, bytes: 49 dwords, lanes on distinct banks

// as psk_soft_kernels.hip soft_mag
__device__ __forceinline__ int soft8_mag(double num, double den) {
  const double r = num / den;
  const double q = floor(r * 127.0 + 0.5);
  if (!(q >= 1.0)) return 1;                        // NaN (0/0, inf/inf, a NaN component) and the decision edge
  return q > 127.0 ? 127 : (int)q;
}

__global__ __launch_bounds__(256) void k_psk_soft8(PskBuffers buf, PskParams p, int8_t* __restrict__ soft,
                                                   int64_t soft_stride) {
  __shared__ int8_t tile[kWave][kSoft8Pitch];
  __shared__ int64_t row_start[kWave], row_vals[kWave];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.y * kWave + lane;
  const bool live = s < buf.n_streams;
  const int64_t S = p.n_sym;
  const int64_t nd = S - 1;                         // differential products per stream
  const int64_t k0 = (int64_t)blockIdx.x * kSoft8Tile;
  if (wv == 0) {
    // the window of the stream's bits its bytes hold (k_sync_pack's outputs); without them every bit from 0
    int64_t st = 0, nv = 0;
    if (live) {
      const int64_t sy = buf.sync_idx ? buf.sync_idx[s] : -1;
      st = sy > 0 ? sy : 0;
      nv = buf.out_len ? 8 * buf.out_len[s] : p.n_bits;
      if (nv > p.n_bits - st) nv = p.n_bits - st;
      if (nv > soft_stride) nv = soft_stride;
      if (nv < 0) nv = 0;
    }
    row_start[lane] = st;
    row_vals[lane] = nv;
  }
  const double* __restrict__ sym = buf.s1;
  const int64_t kw = k0 + wv * 16;                  // this wave's first product: bit 3 kw = 48 (kw / 16)
  if (live && kw < nd) {
    // the 48 hard bits from bit 3 kw on: at offset 0 or 16 of a word, so inside two words
    const int64_t bit0 = 3 * kw, wi = bit0 >> 5;
    const uint32_t w0 = buf.words[(size_t)s * p.n_words + (size_t)wi];
    const uint32_t w1 = wi + 1 < p.n_words ? buf.words[(size_t)s * p.n_words + (size_t)wi + 1] : 0u;
    const uint64_t hard = (((uint64_t)w0 << 32) | w1) << (int)(bit0 & 31);
    double pr = sym[sym_index(s, S, kw, 0)], pi = sym[sym_index(s, S, kw, 1)];
    for (int u = 0; u < 16; ++u) {
      const int64_t k = kw + u;
      if (k >= nd) break;
      const double nr = sym[sym_index(s, S, k + 1, 0)], ni = sym[sym_index(s, S, k + 1, 1)];
      // diff_k = s_{k+1} * conj(s_k): numpy's fma form, as K4a
      const double br = pr, bi = -pi;
      const double dr = __builtin_fma(nr, br, -(ni * bi));
      const double di = __builtin_fma(nr, bi, ni * br);
      const double den = fabs(dr) + fabs(di);
      const double tr = kTanPi8 * dr, ti = kTanPi8 * di;
      const double a = fabs(di - tr), b = fabs(dr + ti);
      const int m2 = soft8_mag(fabs(di + tr), den);
      const int m1 = soft8_mag(fabs(ti - dr), den);
      const int m0 = soft8_mag(a < b ? a : b, den);
      const uint32_t g = (uint32_t)(hard >> (61 - 3 * u)) & 7u;
      const int col = (wv * 16 + u) * 3;
      tile[lane][col] = (int8_t)((g & 4u) ? m2 : -m2);
      tile[lane][col + 1] = (int8_t)((g & 2u) ? m1 : -m1);
      tile[lane][col + 2] = (int8_t)((g & 1u) ? m0 : -m0);
      pr = nr;
      pi = ni;
    }
  }
  __syncthreads();
  // rows leave whole: 192 consecutive threads write 192 consecutive bytes of one stream
  constexpr int nb = 3 * kSoft8Tile;                // the tile's bits per stream
  for (int idx = threadIdx.x; idx < kWave * nb; idx += 256) {
    const int sl = idx / nb, col = idx - sl * nb;
    const int64_t ss = (int64_t)blockIdx.y * kWave + sl;
    const int64_t bit = k0 * 3 + col;
    const int64_t j = bit - row_start[sl];
    if (ss < buf.n_streams && bit < p.n_bits && j >= 0 && j < row_vals[sl])
      soft[(size_t)ss * (size_t)soft_stride + (size_t)j] = tile[sl][col];
  }
}

}  // namespace

hipError_t launch_psk_slice8(const PskBuffers& b, const PskParams& p, hipStream_t st, bool only_flagged) {
  const int64_t groups = (b.n_streams + kWave - 1) / kWave;
  if (p.n_words < 1 || p.n_bits < 1) return hipSuccess;
  const dim3 grid((unsigned)((p.n_words + kSlice8Words - 1) / kSlice8Words), (unsigned)groups);
  hipLaunchKernelGGL(k_slice8, grid, dim3(256), 0, st, b, p, only_flagged ? 1 : 0);
  return hipGetLastError();
}

// after launch_sync_pack on the same stream (b.sync_idx / b.out_len; both null: every bit from 0)
hipError_t launch_psk_soft8(const PskBuffers& b, const PskParams& p, int8_t* soft, int64_t soft_stride,
                            hipStream_t st) {
  if (b.n_streams <= 0 || p.n_sym < 2 || p.n_bits < 1 || soft_stride < 1) return hipSuccess;
  const int64_t groups = (b.n_streams + kWave - 1) / kWave;
  const dim3 grid((unsigned)((p.n_sym - 1 + kSoft8Tile - 1) / kSoft8Tile), (unsigned)groups);
  hipLaunchKernelGGL(k_psk_soft8, grid, dim3(256), 0, st, b, p, soft, soft_stride);
  return hipGetLastError();
}

}  // namespace amr
