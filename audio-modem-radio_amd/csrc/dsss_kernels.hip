// dsss_kernels.hip -- spread: the direct-sequence DBPSK modem (DESIGN.md §3l;
// no reference counterpart -- the reference's dsss_modulate is a BPSK alias and
// it has no dsss_demodulate).  tests/spread_cases.py restates every kernel here
// in numpy; both directions are bit-equal to it.
//
//   k_dsss_despread  Y[b][s] = sum_i x[b][o_b + s*L + i] * T[i], at per-stream offsets
//   k_dsss_slice     the differential BPSK decision, a ballot into MSB-first words
//   k_dsss_soft      one int8 per product (K4s's BPSK magnitude and window rule)
//   k_tx_dsss_sign / k_tx_dsss   the modulator
#include <hip/hip_runtime.h>

#include "dsss.h"
#include "psk_common.h"

namespace amr {
namespace {

// ---------------------------------------------------------------------------
// k_dsss_despread.  k_ofdm_dft's mapping with one "subcarrier":
// one lane owns one bit, flat index b*S + s; workgroup = one wave.  The bit is
// walked in chunks of kDsChunk samples: the wave stages its 64 bits' chunk in
// LDS as float64 (two rows of 32 consecutive samples per load instruction, all
// 32 loads of a chunk in flight before the first is used), then every lane
// reads its own row back (pitch 33 doubles: a half-wave on distinct bank
// pairs).  T[i] is one wave-uniform (scalar) load of 16 bytes.
// A row starts at its stream's offset o_b in [0, L - 1], so every row starts
// below S*L <= n (the `safe` sample of lane 0 is always a real one) and only a
// stream's last bit can pass n: rowlim[r] is the count of the row's samples
// below n, and a sample at or past it is staged as 0.0 without a load.  A wave
// with no such row takes the staging loop without the per-row limit (CUT false).
//
// The order is the specification: p[i & 3] += x * T, product rounded, then the
// sum, sequential in i from 0.0; Y = (p0 + p1) + (p2 + p3).
constexpr int kDsChunk = 32;                    // samples of a bit in LDS at a time (a multiple of 4)
constexpr int kDsPitch = kDsChunk + 1;          // doubles

template <typename T, bool CUT>
__device__ __forceinline__ void despread_rows(const T* __restrict__ x, int64_t L, CDouble* Tt,
                                              double (&tile)[kWave][kDsPitch], const int64_t (&rowbase)[kWave],
                                              const int64_t (&rowlim)[kWave], double* __restrict__ y) {
  const int lane = threadIdx.x;
  const int sj = lane & (kDsChunk - 1), sr = lane >> 5;   // staging: sample of the chunk, row parity
  double pr[4] = {0.0, 0.0, 0.0, 0.0}, pi[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t m0 = 0; m0 < L; m0 += kDsChunk) {
    const int cnt = L - m0 < kDsChunk ? (int)(L - m0) : kDsChunk;
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
    CDouble* w = Tt + m0 * 2;
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {              // m0 + j is a multiple of 4: q = i & 3
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double xv = tile[lane][j + q];
        pr[q] = pr[q] + xv * w[2 * (j + q)];
        pi[q] = pi[q] + xv * w[2 * (j + q) + 1];
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {               // L mod 4 != 0: the last chunk's tail
      if (j + q < cnt) {
        const double xv = tile[lane][j + q];
        pr[q] = pr[q] + xv * w[2 * (j + q)];
        pi[q] = pi[q] + xv * w[2 * (j + q) + 1];
      }
    }
  }
  if (y) *reinterpret_cast<double2*>(y) = make_double2((pr[0] + pr[1]) + (pr[2] + pr[3]), (pi[0] + pi[1]) + (pi[2] + pi[3]));
}

// rowbase and rowlim are written by one lane each and read by every lane with
// no barrier in between: the workgroup is one wave, and a wave's LDS operations
// complete in the order it issued them (as k_ofdm_dft_at).
template <typename T>
__global__ __launch_bounds__(kWave) void k_dsss_despread(const T* __restrict__ x, int64_t x_stride, int64_t n_streams,
                                                         DsssParams p, CDouble* Tt,
                                                         const int64_t* __restrict__ offset, double* __restrict__ Y) {
  __shared__ double tile[kWave][kDsPitch];
  __shared__ int64_t rowbase[kWave];
  __shared__ int64_t rowlim[kWave];
  const int lane = threadIdx.x;
  const int64_t S = p.n_sym;
  const int64_t flat = (int64_t)blockIdx.x * kWave + lane;
  const bool live = flat < n_streams * S;
  {
    const int64_t b = live ? flat / S : 0;
    const int64_t s = flat - b * S;
    int64_t o = live && offset ? offset[b] : 0;
    o = o < 0 ? 0 : (o > p.L - 1 ? p.L - 1 : o);              // the entries refuse anything else; never out of bounds
    const int64_t i0 = o + s * p.L;                           // 0 <= i0 < S*L <= n
    rowbase[lane] = live ? b * x_stride + i0 : -1;
    rowlim[lane] = p.n - i0;
  }
  const bool cut = __any(live && rowlim[lane] < p.L) != 0;    // wave-uniform: the workgroup is one wave
  double* const y = live ? Y + (size_t)flat * 2 : nullptr;
  if (cut) despread_rows<T, true>(x, p.L, Tt, tile, rowbase, rowlim, y);
  else despread_rows<T, false>(x, p.L, Tt, tile, rowbase, rowlim, y);
}

// ---------------------------------------------------------------------------
// d = Y[s+1] * conj(Y[s]) (numpy's fma form, as K4a); the bit is dr < 0: NaN
// and zeros of either sign give 0.
__device__ __forceinline__ void dsss_product(double2 nx, double2 prev, double& dr, double& di) {
  const double br = prev.x, bi = -prev.y;
  dr = __builtin_fma(nx.x, br, -(nx.y * bi));
  di = __builtin_fma(nx.x, bi, nx.y * br);
}

// k_dsss_slice: one lane per bit slot, 32 consecutive lanes per output word:
// lane u of word w of stream b decides bit j = 32 w + u; the wave's ballot holds
// its two words, bit u of a half at position u, reversed into MSB-first order.
__global__ __launch_bounds__(256) void k_dsss_slice(const double* __restrict__ Y, int64_t n_streams, DsssParams p,
                                                    uint32_t* __restrict__ words) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t wi = t >> 5;                    // flat word index b * n_words + w
  const int u = (int)(t & 31);
  const bool live = wi < n_streams * p.n_words;
  bool bit = false;
  if (live) {
    const int64_t b = wi / p.n_words, w = wi - b * p.n_words;
    const int64_t j = 32 * w + u;
    if (j < p.n_bits) {
      const double2* __restrict__ y = reinterpret_cast<const double2*>(Y) + (size_t)b * (size_t)p.n_sym;
      double dr, di;
      dsss_product(y[j + 1], y[j], dr, di);
      bit = dr < 0;
    }
  }
  // every lane of the wave takes part (no early exit above)
  const unsigned long long m = __ballot(bit);
  const uint32_t half = (uint32_t)(m >> ((threadIdx.x & 32) ? 32 : 0));
  if (live && u == 0) words[wi] = __brev(half);
}

// as psk_soft_kernels.hip soft_mag
__device__ __forceinline__ int dsss_soft_mag(double num, double den) {
  const double r = num / den;
  const double q = floor(r * 127.0 + 0.5);
  if (!(q >= 1.0)) return 1;                    // NaN (0/0, inf/inf, a NaN component) and the decision edge
  return q > 127.0 ? 127 : (int)q;
}

// k_dsss_soft: one thread per product; the sign is the hard bit read back from
// the words, the window K4s's: soft[b][j], j < 8 * out_len[b], belongs to bit
// start + j, start = the sync index or 0.
__global__ __launch_bounds__(256) void k_dsss_soft(const double* __restrict__ Y, int64_t n_streams, DsssParams p,
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
  const double2* __restrict__ y = reinterpret_cast<const double2*>(Y) + (size_t)b * (size_t)p.n_sym;
  double dr, di;
  dsss_product(y[j + 1], y[j], dr, di);
  const int m = dsss_soft_mag(fabs(dr), fabs(dr) + fabs(di));
  const uint32_t bit = (words[(size_t)b * p.n_words + (size_t)(j >> 5)] >> (31 - (int)(j & 31))) & 1u;
  soft[(size_t)b * (size_t)soft_stride + (size_t)o] = (int8_t)(bit ? m : -m);
}

// ---------------------------------------------------------------------------
// Transmit.  The bits [1,0]*40 + payload (MSB first); s[0] = +1, s[k+1] = -s[k]
// when bit k is 1.  k_tx_dsss_sign: one thread per stream, sequential over the
// symbols it keeps.
__device__ __forceinline__ uint32_t dsss_tx_bit(const uint8_t* __restrict__ d, int64_t k) {
  if (k < 80) return (uint32_t)(~k & 1);
  const int64_t q = k - 80;
  return ((uint32_t)d[q >> 3] >> (7 - (int)(q & 7))) & 1u;
}

__global__ __launch_bounds__(kWave) void k_tx_dsss_sign(const uint8_t* __restrict__ data, int64_t stride,
                                                        const int64_t* __restrict__ n_bytes, int64_t n_streams,
                                                        DsssTx t, int8_t* __restrict__ sign) {
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (s >= n_streams) return;
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const uint8_t* __restrict__ d = data + s * stride;
  const int64_t total = dsss_tx_symbols(nb);
  const int64_t n = total < t.sym_stride ? total : t.sym_stride;   // symbols stored
  int8_t* __restrict__ out = sign + (size_t)s * (size_t)t.sym_stride;
  int8_t v = 1;
  if (n > 0) out[0] = v;
  for (int64_t k = 1; k < n; ++k) {
    if (dsss_tx_bit(d, k - 1)) v = (int8_t)-v;
    out[k] = v;
  }
}

// k_tx_dsss: T2's shape, 4 consecutive samples per thread: sample i of symbol
// k is float32(s[k] * tab[i]), tab = sg * Sn from the host; zeros past the frame.
template <bool VEC>
__global__ __launch_bounds__(256) void k_tx_dsss(const int64_t* __restrict__ n_bytes, int64_t stride, DsssTx t,
                                                 const double* __restrict__ tab, const int8_t* __restrict__ sign,
                                                 float* __restrict__ out, int64_t out_stride,
                                                 int16_t* __restrict__ pcm, int64_t pcm_stride) {
  const int64_t s = blockIdx.y;
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const int64_t len = dsss_tx_symbols(nb) * t.L;
  const int8_t* __restrict__ sg = sign + (size_t)s * (size_t)t.sym_stride;
  const int64_t k0 = (int64_t)blockIdx.x * 1024 + 4 * threadIdx.x;
  if (k0 >= t.n_out) return;
  float f[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    f[u] = 0.0f;
    const int64_t idx = k0 + u;
    if (idx < len && idx < t.n_out) {
      const int64_t sym = idx / t.L, i = idx - sym * t.L;      // sym < sym_stride = ceil(n_out / L)
      f[u] = (float)((double)sg[sym] * tab[i]);
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

hipError_t launch_dsss_despread(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const DsssParams& p,
                                const double* T, const int64_t* offset, double* Y, hipStream_t st) {
  const int64_t total = n_streams * p.n_sym;
  if (total < 1) return hipSuccess;
  const int64_t blocks = (total + kWave - 1) / kWave;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  CDouble* t = (CDouble*)T;
  if (dtype == kF32)
    hipLaunchKernelGGL(k_dsss_despread<float>, grid, dim3(kWave), 0, st, (const float*)x, x_stride, n_streams, p, t,
                       offset, Y);
  else if (dtype == kF64)
    hipLaunchKernelGGL(k_dsss_despread<double>, grid, dim3(kWave), 0, st, (const double*)x, x_stride, n_streams, p,
                       t, offset, Y);
  else if (dtype == kI16)
    hipLaunchKernelGGL(k_dsss_despread<int16_t>, grid, dim3(kWave), 0, st, (const int16_t*)x, x_stride, n_streams,
                       p, t, offset, Y);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_dsss_slice(const double* Y, int64_t n_streams, const DsssParams& p, uint32_t* words,
                             hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1) return hipSuccess;
  const int64_t total = n_streams * p.n_words * 32;   // a lane per bit slot
  hipLaunchKernelGGL(k_dsss_slice, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Y, n_streams, p, words);
  return hipGetLastError();
}

hipError_t launch_dsss_soft(const double* Y, int64_t n_streams, const DsssParams& p, const uint32_t* words,
                            const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                            hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1 || soft_stride < 1) return hipSuccess;
  const int64_t bps = (p.n_bits + 255) / 256;
  hipLaunchKernelGGL(k_dsss_soft, dim3((unsigned)(n_streams * bps)), dim3(256), 0, st, Y, n_streams, p, words,
                     sync_idx, out_len, soft, soft_stride, bps);
  return hipGetLastError();
}

hipError_t launch_dsss_tx(const DsssTx& t, const double* tab, const uint8_t* data, int64_t stride,
                          const int64_t* n_bytes, int64_t n_streams, int8_t* sign, float* out, int64_t out_stride,
                          int16_t* pcm, int64_t pcm_stride, hipStream_t st) {
  if (n_streams < 1 || t.n_out < 1) return hipSuccess;
  const dim3 pg((unsigned)((n_streams + kWave - 1) / kWave));
  hipLaunchKernelGGL(k_tx_dsss_sign, pg, dim3(kWave), 0, st, data, stride, n_bytes, n_streams, t, sign);
  const dim3 sg((unsigned)((t.n_out + 1023) / 1024), (unsigned)n_streams);
  const bool vec = (out_stride % 4) == 0 && ((uintptr_t)out % 16) == 0 &&
                   (!pcm || ((pcm_stride % 4) == 0 && ((uintptr_t)pcm % 8) == 0));
  if (vec)
    hipLaunchKernelGGL((k_tx_dsss<true>), sg, dim3(256), 0, st, n_bytes, stride, t, tab, sign, out, out_stride, pcm,
                       pcm_stride);
  else
    hipLaunchKernelGGL((k_tx_dsss<false>), sg, dim3(256), 0, st, n_bytes, stride, t, tab, sign, out, out_stride, pcm,
                       pcm_stride);
  return hipGetLastError();
}

}  // namespace amr
