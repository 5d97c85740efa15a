// tone8_kernels.hip -- tone8: the 8-FSK modem with Costas sync (DESIGN.md §3n;
// no reference counterpart -- the reference's ft8_modulate is a two-tone FSK
// alias).  tests/tone8_cases.py restates every kernel here in numpy; both
// directions are bit-equal to it.
//
//   k_tone8_dft    Y[b][k][m] = sum_i x[b][o_b + k L + i] * E[((c2 + g_b + 2 m) i) % (2 L)], per-stream (o, g)
//   k_tone8_slice  the tone of the greatest energy, inverse Gray, a ballot into MSB-first words
//   k_tone8_soft   one int8 per bit from the best tone with the bit set and the best with it clear
//   k_tx_tone8_phase / k_tx_tone8   the modulator
#include <hip/hip_runtime.h>

#include "psk_common.h"
#include "tone8.h"

namespace amr {
namespace {

constexpr int kT8LdsEntries = 512;              // E in LDS when 2 L entries fit (8 KB)

// ---------------------------------------------------------------------------
// k_tone8_dft.  k_ofdm_dft at per-stream offsets is the nearest
// relative; a sibling, so that its resource lines stay where they are.  One
// lane owns one (symbol, tone): flat index (b S + k) 8 + m, so the eight lanes
// of a symbol load the same sample in one instruction (one fetch) and a wave
// covers eight symbols.  The table index is window-local, i * inc mod 2 L,
// advanced by inc = c2 + g + 2 m < L with one conditional subtraction.
//
// The order is the specification: p[i & 3] += x * E, product rounded, then the
// sum, sequential in i from 0.0; Y = (p0 + p1) + (p2 + p3).  L is a multiple of
// 8.  A symbol that passes n takes 0.0 for the samples it does not have and
// still adds their products.
template <typename T, bool LDS>
__global__ __launch_bounds__(256) void k_tone8_dft(const T* __restrict__ x, int64_t x_stride, int64_t n_streams,
                                                   Tone8Params p, const double2* __restrict__ E,
                                                   const int64_t* __restrict__ start,
                                                   const int64_t* __restrict__ shift, double* __restrict__ Y) {
  __shared__ double2 es[LDS ? kT8LdsEntries : 1];
  const uint32_t P2 = (uint32_t)(2 * p.L);      // <= 2^25
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < P2; i += 256) es[i] = E[i];
    __syncthreads();
  }
  const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t S = p.n_sym;
  if (flat >= n_streams * S * 8) return;
  const int64_t sym = flat >> 3;
  const int m = (int)(flat & 7);
  const int64_t b = sym / S, k = sym - b * S;
  int64_t o = start ? start[b] : 0;
  o = o < 0 ? 0 : o % p.L;                      // the entries refuse a negative one; never out of bounds
  int64_t g = shift ? shift[b] : 0;
  g = g < -p.G ? -p.G : (g > p.G ? p.G : g);
  const uint32_t inc = (uint32_t)(p.c2 + g + 2 * m);          // 2 <= inc < L
  const int64_t base = o + k * p.L;             // < n: k L + L <= n and o < L
  const int64_t left = p.n - base;
  const int cnt = left < p.L ? (int)left : (int)p.L;          // samples of the symbol below n, >= 1
  const T* __restrict__ xs = x + b * x_stride + base;
  double pr[4] = {0.0, 0.0, 0.0, 0.0}, pi[4] = {0.0, 0.0, 0.0, 0.0};
  uint32_t idx = 0;
  const int full = cnt & ~3;
  int i = 0;
  for (; i < full; i += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double xv = In<T>::cvt(xs[i + q]);
      const double2 e = LDS ? es[idx] : E[idx];
      pr[q] = pr[q] + xv * e.x;
      pi[q] = pi[q] + xv * e.y;
      idx += inc;
      if (idx >= P2) idx -= P2;
    }
  }
  for (; i < (int)p.L; i += 4) {                // a stream's last symbols, cut by n
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double xv = i + q < cnt ? In<T>::cvt(xs[i + q]) : 0.0;
      const double2 e = LDS ? es[idx] : E[idx];
      pr[q] = pr[q] + xv * e.x;
      pi[q] = pi[q] + xv * e.y;
      idx += inc;
      if (idx >= P2) idx -= P2;
    }
  }
  *reinterpret_cast<double2*>(Y + (size_t)flat * 2) =
      make_double2((pr[0] + pr[1]) + (pr[2] + pr[3]), (pi[0] + pi[1]) + (pi[2] + pi[3]));
}

// ---------------------------------------------------------------------------
// the eight energies of a symbol, each product rounded before the sum
__device__ __forceinline__ void tone8_energies(const double2* __restrict__ y, double (&e)[8]) {
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const double2 v = y[m];
    e[m] = v.x * v.x + v.y * v.y;
  }
}

// the first maximum from m = 0: greater must be strict, so a NaN never wins and a NaN e[0] keeps 0
__device__ __forceinline__ int tone8_decide(const double (&e)[8]) {
  int best = 0;
  double bv = e[0];
#pragma unroll
  for (int m = 1; m < 8; ++m) {
    if (e[m] > bv) {
      bv = e[m];
      best = m;
    }
  }
  return best;
}

// the tribit of a tone: the inverse of v ^ (v >> 1)
__device__ __forceinline__ int tone8_ungray(int t) { return t ^ (t >> 1) ^ (t >> 2); }

// k_tone8_slice: k_msk_slice's shape, one lane per bit slot, 32 consecutive
// lanes per output word: lane u of word w of stream b decides bit j = 32 w + u
// of symbol j / 3.
__global__ __launch_bounds__(256) void k_tone8_slice(const double* __restrict__ Y, int64_t n_streams, Tone8Params p,
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
      const int64_t k = j / 3;
      const int r = (int)(j - 3 * k);
      double e[8];
      tone8_energies(reinterpret_cast<const double2*>(Y) + ((size_t)b * (size_t)p.n_sym + (size_t)k) * 8, e);
      bit = (tone8_ungray(tone8_decide(e)) >> (2 - r)) & 1;
    }
  }
  // every lane of the wave takes part (no early exit above)
  const unsigned long long m = __ballot(bit);
  const uint32_t half = (uint32_t)(m >> ((threadIdx.x & 32) ? 32 : 0));
  if (live && u == 0) words[wi] = __brev(half);
}

// as psk_soft_kernels.hip soft_mag
__device__ __forceinline__ int tone8_soft_mag(double num, double den) {
  const double r = num / den;
  const double q = floor(r * 127.0 + 0.5);
  if (!(q >= 1.0)) return 1;                    // NaN (0/0, inf/inf, a NaN component) and the decision edge
  return q > 127.0 ? 127 : (int)q;
}

// the larger of two energies, a NaN losing: b when it is greater or a is a NaN
__device__ __forceinline__ double tone8_larger(double a, double b) { return (b > a || a != a) ? b : a; }

// k_tone8_soft: one thread per bit; a1 / a0 the largest energy among the four
// tones whose tribit has the bit set / clear, folded in tone order; the sign is
// the hard bit read back from the words, the window K4s's.
__global__ __launch_bounds__(256) void k_tone8_soft(const double* __restrict__ Y, int64_t n_streams, Tone8Params p,
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
  const int64_t k = j / 3;
  const int r = (int)(j - 3 * k);
  double e[8];
  tone8_energies(reinterpret_cast<const double2*>(Y) + ((size_t)b * (size_t)p.n_sym + (size_t)k) * 8, e);
  double a1 = 0.0, a0 = 0.0;
  bool h1 = false, h0 = false;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if ((tone8_ungray(m) >> (2 - r)) & 1) {
      a1 = h1 ? tone8_larger(a1, e[m]) : e[m];
      h1 = true;
    } else {
      a0 = h0 ? tone8_larger(a0, e[m]) : e[m];
      h0 = true;
    }
  }
  const int mag = tone8_soft_mag(fabs(a1 - a0), a1 + a0);
  const uint32_t bit = (words[(size_t)b * p.n_words + (size_t)(j >> 5)] >> (31 - (int)(j & 31))) & 1u;
  soft[(size_t)b * (size_t)soft_stride + (size_t)o] = (int8_t)(bit ? mag : -mag);
}

// ---------------------------------------------------------------------------
// Transmit.  The symbols: the Costas block 3, 1, 4, 0, 6, 5, 2, then the
// payload's tribits (MSB first, zero-padded), tribit v as tone v ^ (v >> 1).
// Symbol k starts at the integer phase p_k in units of 1 / (2 L) cycle, p_0 = 0,
// p_{k+1} = (p_k + L * inc_k) % (2 L).  k_tx_tone8_phase: one thread per stream,
// sequential over the symbols it keeps; ph[k] = p_k | (tone_k << 28).
__device__ __forceinline__ uint32_t tone8_tx_tone(const uint8_t* __restrict__ d, int64_t nb, int64_t k) {
  constexpr uint32_t costas = 0x2560413u;       // 3, 1, 4, 0, 6, 5, 2 in nibbles, the first lowest
  if (k < kTone8Costas) return (costas >> (4 * (int)k)) & 7u;
  const int64_t q = 3 * (k - kTone8Costas);
  uint32_t v = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int64_t bi = q + r;
    const uint32_t bit = bi < 8 * nb ? ((uint32_t)d[bi >> 3] >> (7 - (int)(bi & 7))) & 1u : 0u;
    v = (v << 1) | bit;
  }
  return v ^ (v >> 1);
}

__global__ __launch_bounds__(kWave) void k_tx_tone8_phase(const uint8_t* __restrict__ data, int64_t stride,
                                                          const int64_t* __restrict__ n_bytes, int64_t n_streams,
                                                          Tone8Tx t, uint32_t* __restrict__ ph) {
  const int64_t s = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (s >= n_streams) return;
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const uint8_t* __restrict__ d = data + s * stride;
  const int64_t total = tone8_tx_syms(nb);
  const int64_t n = total < t.sym_stride ? total : t.sym_stride;   // symbols stored
  uint32_t* __restrict__ out = ph + (size_t)s * (size_t)t.sym_stride;
  const int64_t P2 = 2 * t.L;
  int64_t pk = 0;
  for (int64_t k = 0; k < n; ++k) {
    const uint32_t tone = tone8_tx_tone(d, nb, k);
    out[k] = (uint32_t)pk | (tone << 28);
    pk = (pk + t.L * (t.c2 + 2 * (int64_t)tone)) % P2;          // L * inc < 2^48
  }
}

// k_tx_tone8: k_tx_msk's shape, 4 consecutive samples per thread: sample i of
// symbol k is float32(Sn[(p_k + i * inc_k) % (2 L)]), the index in 64-bit
// integers (i * inc < L * L <= 2^48); zeros past the frame.
template <bool VEC>
__global__ __launch_bounds__(256) void k_tx_tone8(const int64_t* __restrict__ n_bytes, int64_t stride, Tone8Tx t,
                                                  const double* __restrict__ Sn, const uint32_t* __restrict__ ph,
                                                  float* __restrict__ out, int64_t out_stride,
                                                  int16_t* __restrict__ pcm, int64_t pcm_stride) {
  const int64_t s = blockIdx.y;
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const int64_t len = tone8_tx_syms(nb) * t.L;
  const uint32_t* __restrict__ pd = ph + (size_t)s * (size_t)t.sym_stride;
  const int64_t k0 = (int64_t)blockIdx.x * 1024 + 4 * threadIdx.x;
  if (k0 >= t.n_out) return;
  const int64_t P2 = 2 * t.L;
  float f[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    f[u] = 0.0f;
    const int64_t idx = k0 + u;
    if (idx < len && idx < t.n_out) {
      const int64_t k = idx / t.L, i = idx - k * t.L;          // k < sym_stride = ceil(n_out / L)
      const uint32_t v = pd[k];
      const int64_t inc = t.c2 + 2 * (int64_t)(v >> 28);
      f[u] = (float)Sn[((int64_t)(v & 0xfffffffu) + i * inc) % P2];
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

template <typename T>
hipError_t dft_launch(const void* x, int64_t x_stride, int64_t n_streams, const Tone8Params& p, dim3 grid,
                      const double* E, const int64_t* start, const int64_t* shift, double* Y, hipStream_t st) {
  const double2* e = reinterpret_cast<const double2*>(E);
  if (2 * p.L <= kT8LdsEntries)
    hipLaunchKernelGGL((k_tone8_dft<T, true>), grid, dim3(256), 0, st, (const T*)x, x_stride, n_streams, p, e, start,
                       shift, Y);
  else
    hipLaunchKernelGGL((k_tone8_dft<T, false>), grid, dim3(256), 0, st, (const T*)x, x_stride, n_streams, p, e, start,
                       shift, Y);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_tone8_dft(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const Tone8Params& p,
                            const double* E, const int64_t* start, const int64_t* shift, double* Y, hipStream_t st) {
  const int64_t total = n_streams * p.n_sym * 8;
  if (total < 1) return hipSuccess;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  if (dtype == kF32) return dft_launch<float>(x, x_stride, n_streams, p, grid, E, start, shift, Y, st);
  if (dtype == kF64) return dft_launch<double>(x, x_stride, n_streams, p, grid, E, start, shift, Y, st);
  if (dtype == kI16) return dft_launch<int16_t>(x, x_stride, n_streams, p, grid, E, start, shift, Y, st);
  return hipErrorInvalidValue;
}

hipError_t launch_tone8_slice(const double* Y, int64_t n_streams, const Tone8Params& p, uint32_t* words,
                              hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1) return hipSuccess;
  const int64_t total = n_streams * p.n_words * 32;   // a lane per bit slot
  hipLaunchKernelGGL(k_tone8_slice, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Y, n_streams, p, words);
  return hipGetLastError();
}

hipError_t launch_tone8_soft(const double* Y, int64_t n_streams, const Tone8Params& p, const uint32_t* words,
                             const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                             hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1 || soft_stride < 1) return hipSuccess;
  const int64_t bps = (p.n_bits + 255) / 256;
  hipLaunchKernelGGL(k_tone8_soft, dim3((unsigned)(n_streams * bps)), dim3(256), 0, st, Y, n_streams, p, words,
                     sync_idx, out_len, soft, soft_stride, bps);
  return hipGetLastError();
}

hipError_t launch_tone8_tx(const Tone8Tx& t, const double* Sn, const uint8_t* data, int64_t stride,
                           const int64_t* n_bytes, int64_t n_streams, uint32_t* ph, float* out, int64_t out_stride,
                           int16_t* pcm, int64_t pcm_stride, hipStream_t st) {
  if (n_streams < 1 || t.n_out < 1) return hipSuccess;
  const dim3 pg((unsigned)((n_streams + kWave - 1) / kWave));
  hipLaunchKernelGGL(k_tx_tone8_phase, pg, dim3(kWave), 0, st, data, stride, n_bytes, n_streams, t, ph);
  const dim3 sg((unsigned)((t.n_out + 1023) / 1024), (unsigned)n_streams);
  const bool vec = (out_stride % 4) == 0 && ((uintptr_t)out % 16) == 0 &&
                   (!pcm || ((pcm_stride % 4) == 0 && ((uintptr_t)pcm % 8) == 0));
  if (vec)
    hipLaunchKernelGGL((k_tx_tone8<true>), sg, dim3(256), 0, st, n_bytes, stride, t, Sn, ph, out, out_stride, pcm,
                       pcm_stride);
  else
    hipLaunchKernelGGL((k_tx_tone8<false>), sg, dim3(256), 0, st, n_bytes, stride, t, Sn, ph, out, out_stride, pcm,
                       pcm_stride);
  return hipGetLastError();
}

}  // namespace amr
