// star16_kernels.hip -- star16: the two-ring 16-DAPSK demodulator's own two
// stages (no reference counterpart -- the reference's "APSK16"
// is a QPSK alias).  The band-pass, mixer, low-pass and symbol sampler are
// QPSK's kernels unchanged; these are the siblings of psk8_kernels.hip's
// k_slice8 and k_psk_soft8 behind them.
//
// Per differential product d = s[k+1] * conj(s[k]) (the fma form K4a evaluates)
// four bits (a, b2, b1, b0), MSB first:
//   b2 b1 b0   d8psk's tribit of d, unchanged (psk8_kernels.hip)
//   a          the ring changed: with e = sr*sr + si*si of a symbol (two rounded
//              products, one rounded sum -- numpy's, never an fma)
//                a = (e[k+1] > 2.0 * e[k]) | (e[k] > 2.0 * e[k+1])
//              (2.0 * e is exact; NaN, inf against inf, zeros and exact ties
//              compare false: the rule is total).
// Eight products fill one 32-bit word and no nibble straddles words, so the
// unit of work is 8 products = 1 word.
#include <hip/hip_runtime.h>

#include "psk_common.h"

namespace amr {
namespace {

constexpr double kTanPi8 = 0x1.a827999fcef32p-2;

// as psk8_kernels.hip d8psk_tribit
__device__ __forceinline__ uint32_t star16_tribit(double dr, double di) {
  const double ar = fabs(dr), ai = fabs(di);
  uint32_t m;
  if (ai < kTanPi8 * ar) m = dr > 0 ? 0u : 4u;
  else if (ar < kTanPi8 * ai) m = di > 0 ? 2u : 6u;
  else if (di > 0) m = dr > 0 ? 1u : 3u;
  else m = dr > 0 ? 7u : 5u;
  return m ^ (m >> 1);
}

// a symbol's energy as numpy evaluates sr*sr + si*si on the two arrays: the
// intrinsics keep the three roundings whatever the contraction setting
__device__ __forceinline__ double star16_energy(double sr, double si) {
  return __dadd_rn(__dmul_rn(sr, sr), __dmul_rn(si, si));
}

__device__ __forceinline__ uint32_t star16_ring_bit(double e0, double e1) {
  return (e1 > 2.0 * e0) || (e0 > 2.0 * e1) ? 1u : 0u;
}

// ---------------------------------------------------------------------------
// K4a16: differential product + energy compare + 8-sector slicer + bit packing.
// Workgroup = 64 streams x kSlice16Units units of 8 products (1 word each):
// wave w slices units 8w .. 8w + 7 of its 64 streams (lane = stream; symbol
// loads are whole 512-B lines through sym_index, the running symbol and its
// energy carried from product to product, so each e is computed once), the
// words go through LDS and leave as row segments of 32 consecutive words per
// stream, as k_slice8's do.
constexpr int kSlice16Units = 32;                   // per workgroup: 256 products, 32 words

__global__ __launch_bounds__(256) void k_slice16(PskBuffers buf, PskParams p, int only_flagged) {
  if (buf.gate && *buf.gate == 0) return;   // a gated launch (PskBuffers::gate): whole grid
  constexpr int UPW = kSlice16Units / 4;            // units per wave
  __shared__ uint32_t wl[kWave][kSlice16Units + 1];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.y * kWave + lane;
  const bool live = s < buf.n_streams && (!only_flagged || buf.flags[s] != 0);
  const int64_t S = p.n_sym;
  const int64_t nd = S - 1;                         // number of diffs
  const int64_t u0 = (int64_t)blockIdx.x * kSlice16Units + wv * UPW;   // this wave's first unit
  const double* __restrict__ sym = buf.s1;
  auto SYM = [&](int64_t k) { return make_double2(sym[sym_index(s, S, k, 0)], sym[sym_index(s, S, k, 1)]); };
  double2 prev = make_double2(0.0, 0.0);
  double pe = 0.0;
  if (live) {
    const int64_t k0 = u0 * 8;
    prev = SYM(k0 < S ? k0 : S - 1);
    pe = star16_energy(prev.x, prev.y);
  }
  for (int q = 0; q < UPW; ++q) {
    const int64_t k0 = (u0 + q) * 8;
    uint32_t w = 0u;
    if (live && k0 < nd) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t k = k0 + u;
        if (k < nd) {
          const double2 nx = SYM(k + 1);
          const double ne = star16_energy(nx.x, nx.y);
          // diff_k = s_{k+1} * conj(s_k): numpy fma form (see oracle)
          const double br = prev.x, bi = -prev.y;
          const double dr = __builtin_fma(nx.x, br, -(nx.y * bi));
          const double di = __builtin_fma(nx.x, bi, nx.y * br);
          const uint32_t nib = (star16_ring_bit(pe, ne) << 3) | star16_tribit(dr, di);
          w |= nib << (28 - 4 * u);
          prev = nx;
          pe = ne;
        }
      }
    }
    wl[lane][wv * UPW + q] = w;
  }
  __syncthreads();
  // rows leave whole: 32 consecutive threads write 32 consecutive words of one stream
  const int64_t j0 = (int64_t)blockIdx.x * kSlice16Units;
  for (int idx = threadIdx.x; idx < kWave * kSlice16Units; idx += 256) {
    const int sl = idx / kSlice16Units, jj = idx - sl * kSlice16Units;
    const int64_t ss = (int64_t)blockIdx.y * kWave + sl;
    const int64_t j = j0 + jj;
    if (ss < buf.n_streams && j < p.n_words && (!only_flagged || buf.flags[ss] != 0))
      buf.words[(size_t)ss * p.n_words + j] = wl[sl][jj];
  }
}

// ---------------------------------------------------------------------------
// K4s16: four int8 per product, in bit order a, b2, b1, b0.  The sign is the
// hard bit read back from the words (as K4s), the magnitude K4s's rule
//   q = floor(num / den * 127.0 + 0.5);  1 unless q >= 1;  127 if q > 127
// b2, b1, b0 are k_psk_soft8's three expressions with den = |dr| + |di|; for a,
// with e0 = e[k], e1 = e[k+1]:
//   p = |e1 - 2.0*e0|, r = |e0 - 2.0*e1|, num = p < r ? p : r, den = e0 + e1
// (64 at equal energies, 51 at a clean ring change; inf - inf is NaN and falls
// to magnitude 1).
// Workgroup = 64 streams x kSoft16Tile products; wave w computes products
// w*16 .. w*16+15 of the tile (their 64 hard bits are exactly two words of the
// stream's row), the values go through LDS and leave as row segments of 256
// consecutive bytes per stream, inside the sync / out_len window as K4s.
constexpr int kSoft16Tile = 64;                     // products per stream and workgroup
constexpr int kSoft16Pitch = 4 * kSoft16Tile + 4;   // LDS row pitch, bytes: 65 dwords, lanes on distinct banks

// as psk_soft_kernels.hip soft_mag
__device__ __forceinline__ int soft16_mag(double num, double den) {
  const double r = num / den;
  const double q = floor(r * 127.0 + 0.5);
  if (!(q >= 1.0)) return 1;                        // NaN (0/0, inf/inf, a NaN component) and the decision edge
  return q > 127.0 ? 127 : (int)q;
}

__global__ __launch_bounds__(256) void k_psk_soft16(PskBuffers buf, PskParams p, int8_t* __restrict__ soft,
                                                    int64_t soft_stride) {
  __shared__ int8_t tile[kWave][kSoft16Pitch];
  __shared__ int64_t row_start[kWave], row_vals[kWave];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.y * kWave + lane;
  const bool live = s < buf.n_streams;
  const int64_t S = p.n_sym;
  const int64_t nd = S - 1;                         // differential products per stream
  const int64_t k0 = (int64_t)blockIdx.x * kSoft16Tile;
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
  const int64_t kw = k0 + wv * 16;                  // this wave's first product: bit 4 kw = 64 (kw / 16)
  if (live && kw < nd) {
    // the 64 hard bits from bit 4 kw on: two whole words
    const int64_t wi = kw >> 3;
    const uint32_t w0 = buf.words[(size_t)s * p.n_words + (size_t)wi];
    const uint32_t w1 = wi + 1 < p.n_words ? buf.words[(size_t)s * p.n_words + (size_t)wi + 1] : 0u;
    const uint64_t hard = ((uint64_t)w0 << 32) | w1;
    double pr = sym[sym_index(s, S, kw, 0)], pi = sym[sym_index(s, S, kw, 1)];
    double e0 = star16_energy(pr, pi);
    for (int u = 0; u < 16; ++u) {
      const int64_t k = kw + u;
      if (k >= nd) break;
      const double nr = sym[sym_index(s, S, k + 1, 0)], ni = sym[sym_index(s, S, k + 1, 1)];
      const double e1 = star16_energy(nr, ni);
      // diff_k = s_{k+1} * conj(s_k): numpy's fma form, as K4a
      const double br = pr, bi = -pi;
      const double dr = __builtin_fma(nr, br, -(ni * bi));
      const double di = __builtin_fma(nr, bi, ni * br);
      const double den = fabs(dr) + fabs(di);
      const double tr = kTanPi8 * dr, ti = kTanPi8 * di;
      const double a = fabs(di - tr), b = fabs(dr + ti);
      const int m2 = soft16_mag(fabs(di + tr), den);
      const int m1 = soft16_mag(fabs(ti - dr), den);
      const int m0 = soft16_mag(a < b ? a : b, den);
      const double pp = fabs(e1 - 2.0 * e0), rr = fabs(e0 - 2.0 * e1);
      const int ma = soft16_mag(pp < rr ? pp : rr, e0 + e1);
      const uint32_t nib = (uint32_t)(hard >> (60 - 4 * u)) & 15u;
      const int col = (wv * 16 + u) * 4;
      tile[lane][col] = (int8_t)((nib & 8u) ? ma : -ma);
      tile[lane][col + 1] = (int8_t)((nib & 4u) ? m2 : -m2);
      tile[lane][col + 2] = (int8_t)((nib & 2u) ? m1 : -m1);
      tile[lane][col + 3] = (int8_t)((nib & 1u) ? m0 : -m0);
      pr = nr;
      pi = ni;
      e0 = e1;
    }
  }
  __syncthreads();
  // rows leave whole: 256 consecutive threads write 256 consecutive bytes of one stream
  constexpr int nb = 4 * kSoft16Tile;               // the tile's bits per stream
  for (int idx = threadIdx.x; idx < kWave * nb; idx += 256) {
    const int sl = idx / nb, col = idx - sl * nb;
    const int64_t ss = (int64_t)blockIdx.y * kWave + sl;
    const int64_t bit = k0 * 4 + col;
    const int64_t j = bit - row_start[sl];
    if (ss < buf.n_streams && bit < p.n_bits && j >= 0 && j < row_vals[sl])
      soft[(size_t)ss * (size_t)soft_stride + (size_t)j] = tile[sl][col];
  }
}

}  // namespace

hipError_t launch_psk_slice16(const PskBuffers& b, const PskParams& p, hipStream_t st, bool only_flagged) {
  const int64_t groups = (b.n_streams + kWave - 1) / kWave;
  if (p.n_words < 1 || p.n_bits < 1) return hipSuccess;
  const dim3 grid((unsigned)((p.n_words + kSlice16Units - 1) / kSlice16Units), (unsigned)groups);
  hipLaunchKernelGGL(k_slice16, grid, dim3(256), 0, st, b, p, only_flagged ? 1 : 0);
  return hipGetLastError();
}

// after launch_sync_pack on the same stream (b.sync_idx / b.out_len; both null: every bit from 0)
hipError_t launch_psk_soft16(const PskBuffers& b, const PskParams& p, int8_t* soft, int64_t soft_stride,
                             hipStream_t st) {
  if (b.n_streams <= 0 || p.n_sym < 2 || p.n_bits < 1 || soft_stride < 1) return hipSuccess;
  const int64_t groups = (b.n_streams + kWave - 1) / kWave;
  const dim3 grid((unsigned)((p.n_sym - 1 + kSoft16Tile - 1) / kSoft16Tile), (unsigned)groups);
  hipLaunchKernelGGL(k_psk_soft16, grid, dim3(256), 0, st, b, p, soft, soft_stride);
  return hipGetLastError();
}

}  // namespace amr
