// psk_soft_kernels.hip -- K4s: soft-decision output of the PSK demodulators
// (no reference counterpart).  One int8 per demodulated bit:
// the sign is the bit K4a decided (read back from the words buffer, so the
// two cannot disagree), the magnitude 1..127 how far the differential product
//   d = s[k+1] * conj(s[k])        (the fma form K4a evaluates)
// lies from the bit's decision boundary, in fp64 in this operation order:
//   den = |dr| + |di|
//   QPSK hi bit  r = |dr + di| / den     lo bit  r = |dr - di| / den
//   BPSK bit     r = |dr| / den
//   q = floor(r * 127.0 + 0.5);  m = 1 unless q >= 1;  m = 127 if q > 127
// (IEEE division; the build contracts nothing).  It runs after k_sync_pack:
// soft[s][j], j < 8 * out_len[s], belongs to bit start + j, start = the sync
// index or 0 -- the bits of the stream's packed bytes.
//
// Workgroup = 64 streams x kSoftTile differential products.  Wave w computes
// products w*16 .. w*16+15 of the tile for its 64 streams (lane = stream: the
// symbol loads are whole 512-B lines, the running symbol carried from product
// to product; the 16 products' hard bits are one word of the stream's row),
// the values go through LDS and leave as row segments of 128 (QPSK) / 64
// (BPSK) consecutive bytes per stream.
#include <hip/hip_runtime.h>

#include "psk_common.h"

namespace amr {
namespace {

constexpr int kSoftTile = 64;                   // products per stream and workgroup
constexpr int kSoftPitch = 2 * kSoftTile + 4;   // LDS row pitch, bytes: 33 dwords, lanes on distinct banks

// the magnitude of one soft value from its numerator and den = |dr| + |di|
__device__ __forceinline__ int soft_mag(double num, double den) {
  const double r = num / den;
  const double q = floor(r * 127.0 + 0.5);
  if (!(q >= 1.0)) return 1;                    // NaN (0/0, inf/inf, a NaN component) and the decision edge
  return q > 127.0 ? 127 : (int)q;
}

__global__ __launch_bounds__(256) void k_psk_soft(PskBuffers buf, PskParams p, int8_t* __restrict__ soft,
                                                  int64_t soft_stride) {
  __shared__ int8_t tile[kWave][kSoftPitch];
  __shared__ int64_t row_start[kWave], row_vals[kWave];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.y * kWave + lane;
  const bool live = s < buf.n_streams;
  const int64_t S = p.n_sym;
  const int64_t nd = S - 1;                     // differential products per stream
  const bool qpsk = p.kind == kQpsk;
  const int bps = qpsk ? 2 : 1;
  const int64_t k0 = (int64_t)blockIdx.x * kSoftTile;
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
  const int64_t kw = k0 + wv * 16;              // this wave's first product: 16 | kw, one word's worth (half a BPSK word)
  if (live && kw < nd) {
    const uint32_t word = buf.words[(size_t)s * p.n_words + (size_t)(qpsk ? kw >> 4 : kw >> 5)];
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
      const int col = (wv * 16 + u) * bps;
      if (qpsk) {
        const uint32_t dib = (word >> (30 - 2 * u)) & 3u;
        const int mh = soft_mag(fabs(dr + di), den), ml = soft_mag(fabs(dr - di), den);
        tile[lane][col] = (int8_t)((dib & 2u) ? mh : -mh);
        tile[lane][col + 1] = (int8_t)((dib & 1u) ? ml : -ml);
      } else {
        const uint32_t bit = (word >> (31 - (int)(k & 31))) & 1u;
        const int m = soft_mag(fabs(dr), den);
        tile[lane][col] = (int8_t)(bit ? m : -m);
      }
      pr = nr;
      pi = ni;
    }
  }
  __syncthreads();
  // rows leave whole: nb consecutive threads write nb consecutive bytes of one stream
  const int nb = kSoftTile * bps;               // the tile's bits per stream: 128 / 64
  const int rows = 256 / nb;                    // streams per pass
  const int col = threadIdx.x & (nb - 1);
  const int64_t bit = k0 * bps + col;
  for (int i = 0; i < kWave / rows; ++i) {
    const int sl = i * rows + (int)(threadIdx.x / nb);
    const int64_t ss = (int64_t)blockIdx.y * kWave + sl;
    const int64_t j = bit - row_start[sl];
    if (ss < buf.n_streams && bit < p.n_bits && j >= 0 && j < row_vals[sl])
      soft[(size_t)ss * (size_t)soft_stride + (size_t)j] = tile[sl][col];
  }
}

}  // namespace

// after launch_sync_pack on the same stream (b.sync_idx / b.out_len; both null: every bit from 0)
hipError_t launch_psk_soft(const PskBuffers& b, const PskParams& p, int8_t* soft, int64_t soft_stride,
                           hipStream_t st) {
  if (b.n_streams <= 0 || p.n_sym < 2 || p.n_bits < 1 || soft_stride < 1) return hipSuccess;
  const int64_t groups = (b.n_streams + kWave - 1) / kWave;
  const dim3 grid((unsigned)((p.n_sym - 1 + kSoftTile - 1) / kSoftTile), (unsigned)groups);
  hipLaunchKernelGGL(k_psk_soft, grid, dim3(256), 0, st, b, p, soft, soft_stride);
  return hipGetLastError();
}

}  // namespace amr
