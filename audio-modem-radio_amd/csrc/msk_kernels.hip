// msk_kernels.hip -- minshift: the MSK modem (no reference
// counterpart -- the reference's msk_modulate is an FSK alias and it has no
// msk_demodulate).  tests/minshift_cases.py restates every kernel here in
// numpy; both directions are bit-equal to it.
//
//   k_msk_corr    W[b][k] = sum_i x[b][o_b + (k+1) L - h + i] * U[i], at per-stream offsets
//   k_msk_slice   the differential decision, a ballot into MSB-first words
//   k_msk_soft    one int8 per product (K4s's BPSK magnitude and window rule)
//   k_tx_msk_phase / k_tx_msk   the modulator
#include <hip/hip_runtime.h>

#include "msk.h"
#include "psk_common.h"

namespace amr {
namespace {

// ---------------------------------------------------------------------------
// k_msk_corr.  k_dsss_despread's mapping, a sibling: one lane
// owns one window, flat index b*Sw + k; workgroup = one wave.  The window is
// walked in chunks of kMsChunk samples: the wave stages its 64 windows' chunk
// in LDS as float64 (two rows of 32 consecutive samples per load instruction,
// all 32 loads of a chunk in flight before the first is used), then every lane
// reads its own row back (pitch 33 doubles: a half-wave on distinct bank
// pairs).  U[i] is one wave-uniform (scalar) load of 16 bytes.
// A row starts at (k+1) L - h + o_b with o_b in [0, L - 1]; the last window
// starts at Sw L - h + o_b <= n - L + o_b < n (Sw L <= n + h - L), so every row
// starts below n (the `safe` sample of lane 0 is always a real one) and only a
// stream's last window can pass n: rowlim[r] is the count of the row's samples
// below n, and a sample at or past it is staged as 0.0 without a load.  A wave
// with no such row takes the staging loop without the per-row limit (CUT false).
//
// The order is the specification: p[i & 3] += x * U, product rounded, then the
// sum, sequential in i from 0.0; W = (p0 + p1) + (p2 + p3).
constexpr int kMsChunk = 32;                    // samples of a window in LDS at a time (a multiple of 4)
constexpr int kMsPitch = kMsChunk + 1;          // doubles

template <typename T, bool CUT>
__device__ __forceinline__ void corr_rows(const T* __restrict__ x, int64_t L, CDouble* Ut,
                                          double (&tile)[kWave][kMsPitch], const int64_t (&rowbase)[kWave],
                                          const int64_t (&rowlim)[kWave], double* __restrict__ w_out) {
  const int lane = threadIdx.x;
  const int sj = lane & (kMsChunk - 1), sr = lane >> 5;   // staging: sample of the chunk, row parity
  double pr[4] = {0.0, 0.0, 0.0, 0.0}, pi[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t m0 = 0; m0 < L; m0 += kMsChunk) {
    const int cnt = L - m0 < kMsChunk ? (int)(L - m0) : kMsChunk;
    // a lane with nothing to read (a dead row, past the chunk's or the stream's end) reads the block's first
    // sample instead (lane 0 is always live, its row starts below n) and stores 0.0
    T raw[kWave / 2];
    const int64_t safe = rowbase[0];
#pragma unroll
    for (int i = 0; i < kWave / 2; ++i) {
      const int r = 2 * i + sr;
      const int64_t rb = rowbase[r];
      bool ok = rb >= 0 && sj < cnt;
      if constexpr (CUT) ok = ok && m0 + sj < rowlim[r];
      raw[i] = x[ok ? rb + m0 + sj : safe];
    }
    __syncthreads();                            // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < kWave / 2; ++i) {
      const int r = 2 * i + sr;
      bool ok = rowbase[r] >= 0 && sj < cnt;
      if constexpr (CUT) ok = ok && m0 + sj < rowlim[r];
      tile[r][sj] = ok ? In<T>::cvt(raw[i]) : 0.0;
    }
    __syncthreads();
    CDouble* u = Ut + m0 * 2;
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {              // m0 + j is a multiple of 4: q = i & 3
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double xv = tile[lane][j + q];
        pr[q] = pr[q] + xv * u[2 * (j + q)];
        pi[q] = pi[q] + xv * u[2 * (j + q) + 1];
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {               // L mod 4 != 0: the last chunk's tail
      if (j + q < cnt) {
        const double xv = tile[lane][j + q];
        pr[q] = pr[q] + xv * u[2 * (j + q)];
        pi[q] = pi[q] + xv * u[2 * (j + q) + 1];
      }
    }
  }
  if (w_out)
    *reinterpret_cast<double2*>(w_out) =
        make_double2((pr[0] + pr[1]) + (pr[2] + pr[3]), (pi[0] + pi[1]) + (pi[2] + pi[3]));
}

// rowbase and rowlim are written by one lane each and read by every lane with
// no barrier in between: the workgroup is one wave, and a wave's LDS operations
// complete in the order it issued them (as k_dsss_despread).
template <typename T>
__global__ __launch_bounds__(kWave) void k_msk_corr(const T* __restrict__ x, int64_t x_stride, int64_t n_streams,
                                                    MskParams p, CDouble* Ut, const int64_t* __restrict__ offset,
                                                    double* __restrict__ W) {
  __shared__ double tile[kWave][kMsPitch];
  __shared__ int64_t rowbase[kWave];
  __shared__ int64_t rowlim[kWave];
  const int lane = threadIdx.x;
  const int64_t S = p.n_sym;
  const int64_t flat = (int64_t)blockIdx.x * kWave + lane;
  const bool live = flat < n_streams * S;
  {
    const int64_t b = live ? flat / S : 0;
    const int64_t k = flat - b * S;
    int64_t o = live && offset ? offset[b] : 0;
    o = o < 0 ? 0 : (o > p.L - 1 ? p.L - 1 : o);              // the entries refuse anything else; never out of bounds
    const int64_t i0 = o + (k + 1) * p.L - p.h;               // 0 < i0 < n for a live lane
    rowbase[lane] = live ? b * x_stride + i0 : -1;
    rowlim[lane] = p.n - i0;
  }
  const bool cut = __any(live && rowlim[lane] < p.L) != 0;    // wave-uniform: the workgroup is one wave
  double* const w_out = live ? W + (size_t)flat * 2 : nullptr;
  if (cut) corr_rows<T, true>(x, p.L, Ut, tile, rowbase, rowlim, w_out);
  else corr_rows<T, false>(x, p.L, Ut, tile, rowbase, rowlim, w_out);
}

// ---------------------------------------------------------------------------
// d = W[k+1] * conj(W[k]) (numpy's fma form, as K4a), then D = d * (-i)^rot, a
// swap and negation; the bit is D.imag > 0: NaN and zeros of either sign give 0.
__device__ __forceinline__ void msk_product(double2 nx, double2 prev, int rot, double& Dr, double& Di) {
  const double br = prev.x, bi = -prev.y;
  const double dr = __builtin_fma(nx.x, br, -(nx.y * bi));
  const double di = __builtin_fma(nx.x, bi, nx.y * br);
  Dr = rot == 0 ? dr : rot == 1 ? di : rot == 2 ? -dr : -di;
  Di = rot == 0 ? di : rot == 1 ? -dr : rot == 2 ? -di : dr;
}

// k_msk_slice: one lane per bit slot, 32 consecutive lanes per output word:
// lane u of word w of stream b decides bit j = 32 w + u; the wave's ballot holds
// its two words, bit u of a half at position u, reversed into MSB-first order.
__global__ __launch_bounds__(256) void k_msk_slice(const double* __restrict__ W, int64_t n_streams, MskParams p,
                                                   uint32_t* __restrict__ words) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t wi = t >> 5;                    // flat word index b * n_words + w
  const int u = (int)(t & 31);
  const bool live = wi < n_streams * p.n_words;
  const int rot = (int)(p.cyc4 & 3);
  bool bit = false;
  if (live) {
    const int64_t b = wi / p.n_words, w = wi - b * p.n_words;
    const int64_t j = 32 * w + u;
    if (j < p.n_bits) {
      const double2* __restrict__ y = reinterpret_cast<const double2*>(W) + (size_t)b * (size_t)p.n_sym;
      double Dr, Di;
      msk_product(y[j + 1], y[j], rot, Dr, Di);
      bit = Di > 0;
    }
  }
  // every lane of the wave takes part (no early exit above)
  const unsigned long long m = __ballot(bit);
  const uint32_t half = (uint32_t)(m >> ((threadIdx.x & 32) ? 32 : 0));
  if (live && u == 0) words[wi] = __brev(half);
}

// as psk_soft_kernels.hip soft_mag
__device__ __forceinline__ int msk_soft_mag(double num, double den) {
  const double r = num / den;
  const double q = floor(r * 127.0 + 0.5);
  if (!(q >= 1.0)) return 1;                    // NaN (0/0, inf/inf, a NaN component) and the decision edge
  return q > 127.0 ? 127 : (int)q;
}

// k_msk_soft: one thread per product; the sign is the hard bit read back from
// the words, the window K4s's: soft[b][j], j < 8 * out_len[b], belongs to bit
// start + j, start = the sync index or 0.
__global__ __launch_bounds__(256) void k_msk_soft(const double* __restrict__ W, int64_t n_streams, MskParams p,
                                                  const uint32_t* __restrict__ words,
                                                  const int64_t* __restrict__ sync_idx,
                                                  const int64_t* __restrict__ out_len, int8_t* __restrict__ soft,
                                                  int64_t soft_stride, int64_t blocks_per_stream) {
  const int64_t b = blockIdx.x / blocks_per_stream;
  const int64_t j = (blockIdx.x - b * blocks_per_stream) * 256 + threadIdx.x;
  if (b >= n_streams || j >= p.n_bits) return;
  const int64_t sy = sync_idx ? sync_idx[b] : -1;
  const int64_t st = sy > 0 ? sy : 0;
  int64_t nv = out_len ? 8 * out_len[b] : p.n_bits;
  if (nv > p.n_bits - st) nv = p.n_bits - st;
  if (nv > soft_stride) nv = soft_stride;
  const int64_t o = j - st;
  if (o < 0 || o >= nv) return;
  const double2* __restrict__ y = reinterpret_cast<const double2*>(W) + (size_t)b * (size_t)p.n_sym;
  double Dr, Di;
  msk_product(y[j + 1], y[j], (int)(p.cyc4 & 3), Dr, Di);
  const int m = msk_soft_mag(fabs(Di), fabs(Di) + fabs(Dr));
  const uint32_t bit = (words[(size_t)b * p.n_words + (size_t)(j >> 5)] >> (31 - (int)(j & 31))) & 1u;
  soft[(size_t)b * (size_t)soft_stride + (size_t)o] = (int8_t)(bit ? m : -m);
}

// ---------------------------------------------------------------------------
// Transmit.  The bits [0] + [1,0]*40 + payload (MSB first) + [0]; bit k starts
// at the integer phase p_k = L * ((k cyc4 + sum_{j<k} (2 bit_j - 1)) mod 4) in
// units of 1 / (4 L) cycle.  k_tx_msk_phase: one thread per stream, sequential
// over the bits it keeps; quad[k] = (p_k / L) | (bit_k << 2).
__device__ __forceinline__ uint32_t msk_tx_bit(const uint8_t* __restrict__ d, int64_t k, int64_t total) {
  if (k == 0 || k == total - 1) return 0u;
  if (k <= 80) return (uint32_t)(k & 1);        // preamble bit k - 1 of [1,0]*40
  const int64_t q = k - 81;
  return ((uint32_t)d[q >> 3] >> (7 - (int)(q & 7))) & 1u;
}

__global__ __launch_bounds__(kWave) void k_tx_msk_phase(const uint8_t* __restrict__ data, int64_t stride,
                                                        const int64_t* __restrict__ n_bytes, int64_t n_streams,
                                                        MskTx t, uint8_t* __restrict__ quad) {
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (s >= n_streams) return;
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const uint8_t* __restrict__ d = data + s * stride;
  const int64_t total = msk_tx_bits(nb);
  const int64_t n = total < t.bit_stride ? total : t.bit_stride;   // bits stored
  uint8_t* __restrict__ out = quad + (size_t)s * (size_t)t.bit_stride;
  const uint32_t c = (uint32_t)(t.cyc4 & 3);
  uint32_t ph = 0;                              // p_k / L, mod 4
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t bit = msk_tx_bit(d, k, total);
    out[k] = (uint8_t)(ph | (bit << 2));
    ph = (ph + c + (bit ? 1u : 3u)) & 3u;       // + cyc4 + 1, or + cyc4 - 1, quarter-turns
  }
}

// k_tx_msk: T2's shape, 4 consecutive samples per thread: sample i of bit k is
// float32(Sn[(p_k + i * inc_k) % (4 L)]), the index in 64-bit integers (i * inc
// < 2 L * L <= 2^49); zeros past the frame.
template <bool VEC>
__global__ __launch_bounds__(256) void k_tx_msk(const int64_t* __restrict__ n_bytes, int64_t stride, MskTx t,
                                                const double* __restrict__ Sn, const uint8_t* __restrict__ quad,
                                                float* __restrict__ out, int64_t out_stride,
                                                int16_t* __restrict__ pcm, int64_t pcm_stride) {
  const int64_t s = blockIdx.y;
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const int64_t len = msk_tx_bits(nb) * t.L;
  const uint8_t* __restrict__ qd = quad + (size_t)s * (size_t)t.bit_stride;
  const int64_t k0 = (int64_t)blockIdx.x * 1024 + 4 * threadIdx.x;
  if (k0 >= t.n_out) return;
  const int64_t P4 = 4 * t.L;
  float f[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    f[u] = 0.0f;
    const int64_t idx = k0 + u;
    if (idx < len && idx < t.n_out) {
      const int64_t k = idx / t.L, i = idx - k * t.L;          // k < bit_stride = ceil(n_out / L)
      const uint32_t v = qd[k];
      const int64_t inc = t.cyc4 + ((v & 4u) ? 1 : -1);
      const int64_t ph = ((int64_t)(v & 3u) * t.L + i * inc) % P4;
      f[u] = (float)Sn[ph];
    }
  }
  int16_t q[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) q[u] = (int16_t)(int)(f[u] * 32767.0f);   // (arr * 32767).astype(np.int16)
  float* __restrict__ o = out + s * out_stride + k0;
  int16_t* __restrict__ c = pcm ? pcm + s * pcm_stride + k0 : nullptr;
  if (VEC && k0 + 4 <= t.n_out) {
    *reinterpret_cast<float4*>(o) = make_float4(f[0], f[1], f[2], f[3]);
    if (c) *reinterpret_cast<short4*>(c) = make_short4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (k0 + u < t.n_out) {
        o[u] = f[u];
        if (c) c[u] = q[u];
      }
    }
  }
}

}  // namespace

hipError_t launch_msk_corr(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const MskParams& p,
                           const double* U, const int64_t* offset, double* W, hipStream_t st) {
  const int64_t total = n_streams * p.n_sym;
  if (total < 1) return hipSuccess;
  const int64_t blocks = (total + kWave - 1) / kWave;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  CDouble* u = (CDouble*)U;
  if (dtype == kF32)
    hipLaunchKernelGGL(k_msk_corr<float>, grid, dim3(kWave), 0, st, (const float*)x, x_stride, n_streams, p, u, offset,
                       W);
  else if (dtype == kF64)
    hipLaunchKernelGGL(k_msk_corr<double>, grid, dim3(kWave), 0, st, (const double*)x, x_stride, n_streams, p, u,
                       offset, W);
  else if (dtype == kI16)
    hipLaunchKernelGGL(k_msk_corr<int16_t>, grid, dim3(kWave), 0, st, (const int16_t*)x, x_stride, n_streams, p, u,
                       offset, W);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_msk_slice(const double* W, int64_t n_streams, const MskParams& p, uint32_t* words, hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1) return hipSuccess;
  const int64_t total = n_streams * p.n_words * 32;   // a lane per bit slot
  hipLaunchKernelGGL(k_msk_slice, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, n_streams, p, words);
  return hipGetLastError();
}

hipError_t launch_msk_soft(const double* W, int64_t n_streams, const MskParams& p, const uint32_t* words,
                           const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                           hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1 || soft_stride < 1) return hipSuccess;
  const int64_t bps = (p.n_bits + 255) / 256;
  hipLaunchKernelGGL(k_msk_soft, dim3((unsigned)(n_streams * bps)), dim3(256), 0, st, W, n_streams, p, words,
                     sync_idx, out_len, soft, soft_stride, bps);
  return hipGetLastError();
}

hipError_t launch_msk_tx(const MskTx& t, const double* Sn, const uint8_t* data, int64_t stride,
                         const int64_t* n_bytes, int64_t n_streams, uint8_t* quad, float* out, int64_t out_stride,
                         int16_t* pcm, int64_t pcm_stride, hipStream_t st) {
  if (n_streams < 1 || t.n_out < 1) return hipSuccess;
  const dim3 pg((unsigned)((n_streams + kWave - 1) / kWave));
  hipLaunchKernelGGL(k_tx_msk_phase, pg, dim3(kWave), 0, st, data, stride, n_bytes, n_streams, t, quad);
  const dim3 sg((unsigned)((t.n_out + 1023) / 1024), (unsigned)n_streams);
  const bool vec = (out_stride % 4) == 0 && ((uintptr_t)out % 16) == 0 &&
                   (!pcm || ((pcm_stride % 4) == 0 && ((uintptr_t)pcm % 8) == 0));
  if (vec)
    hipLaunchKernelGGL((k_tx_msk<true>), sg, dim3(256), 0, st, n_bytes, stride, t, Sn, quad, out, out_stride, pcm,
                       pcm_stride);
  else
    hipLaunchKernelGGL((k_tx_msk<false>), sg, dim3(256), 0, st, n_bytes, stride, t, Sn, quad, out, out_stride, pcm,
                       pcm_stride);
  return hipGetLastError();
}

}  // namespace amr
