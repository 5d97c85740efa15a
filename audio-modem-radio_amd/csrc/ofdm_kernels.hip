// ofdm_kernels.hip -- ofdm: the multi-carrier DQPSK modem (no
// reference counterpart -- the reference's ofdm_*_simple are QPSK aliases).
// tests/ofdm_cases.py restates every kernel here in numpy; the receive side is
// bit-equal to it, the transmit samples up to sin's last ulp.
//
//   k_ofdm_dft    Y[b][s][k] = sum_m x[b][s*L + Ncp + m] * W[k][m], the hot path
//   k_ofdm_dft_at the same with each stream read from its own offset (§3k)
//   k_ofdm_slice  the differential decision across time per subcarrier, packed
//   k_ofdm_soft   two int8 per product (K4s's magnitudes and window rule)
//   k_tx_ofdm_phase / k_tx_ofdm_synth   the modulator
#include <hip/hip_runtime.h>

#include "ofdm.h"
#include "psk_common.h"

namespace amr {
namespace {

// ---------------------------------------------------------------------------
// k_ofdm_dft.  One lane owns one OFDM symbol, flat index b*S + s (a wave spans
// stream boundaries when S < 64); workgroup = one wave.  The useful part of
// the symbol is walked in chunks of kDftChunk samples: the wave stages its 64
// symbols' chunk in LDS as float64 (two rows of 32 consecutive samples per
// load instruction, 128-B runs of float32; all 32 loads of a chunk in flight
// before the first is used), then every lane reads its own row back (pitch 33
// doubles: the 32 lanes of a half-wave on distinct bank pairs).
// The subcarriers go in groups of at most kDftGroup: a lane keeps the group's
// 4 partial sums x 2 components in registers, one LDS read serves the group,
// and W[m][k0 .. k0+G) is one wave-uniform (scalar) load of 16 G bytes.  A
// further group re-stages x (from L2: the wave read the same lines just before).
//
// The order is the specification: p[m & 3] += x * W, product
// rounded, then the sum, sequential in m from 0.0; Y = (p0 + p1) + (p2 + p3).
constexpr int kDftChunk = 32;                   // samples of a symbol in LDS at a time (a multiple of 4)
constexpr int kDftPitch = kDftChunk + 1;        // doubles
constexpr int kDftGroup = 4;                    // subcarriers per pass over x

template <int G, int Q>
__device__ __forceinline__ void dft_term(double (&pr)[G][4], double (&pi)[G][4], double xv, CDouble* w) {
#pragma unroll
  for (int i = 0; i < G; ++i) {
    pr[i][Q] = pr[i][Q] + xv * w[2 * i];
    pi[i][Q] = pi[i][Q] + xv * w[2 * i + 1];
  }
}

// One group of subcarriers over the whole symbol, k_ofdm_dft's body.
// AT (k_ofdm_dft_at): a row starts at its stream's offset, so
// its tail may pass the stream's end: rowlim[r] is the count of the row's
// samples below n, and a sample at or past it is staged as 0.0 without a load.
template <typename T, int G, bool AT = false>
__device__ __forceinline__ void dft_group(const T* __restrict__ x, const OfdmParams& p, CDouble* W, int k0,
                                          double (&tile)[kWave][kDftPitch], const int64_t (&rowbase)[kWave],
                                          double* __restrict__ y, const int64_t (&rowlim)[kWave]) {
  const int lane = threadIdx.x;
  const int sj = lane & (kDftChunk - 1), sr = lane >> 5;   // staging: sample of the chunk, row parity
  double pr[G][4], pi[G][4];
#pragma unroll
  for (int i = 0; i < G; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) pr[i][q] = pi[i][q] = 0.0;
  for (int64_t m0 = 0; m0 < p.nu; m0 += kDftChunk) {
    const int cnt = p.nu - m0 < kDftChunk ? (int)(p.nu - m0) : kDftChunk;
    // every load is issued before the first is waited for: a lane with nothing to read (a dead row, past
    // the chunk's end) reads the block's first sample instead (lane 0 is always live) and stores 0.0
    T raw[kWave / 2];
    const int64_t safe = rowbase[0];
#pragma unroll
    for (int i = 0; i < kWave / 2; ++i) {
      const int64_t rb = rowbase[2 * i + sr];
      if constexpr (AT) raw[i] = x[rb >= 0 && sj < cnt && m0 + sj < rowlim[2 * i + sr] ? rb + m0 + sj : safe];
      else raw[i] = x[rb >= 0 && sj < cnt ? rb + m0 + sj : safe];
    }
    __syncthreads();                            // the previous chunk's reads are done
#pragma unroll
    for (int i = 0; i < kWave / 2; ++i) {
      const int r = 2 * i + sr;
      if constexpr (AT) tile[r][sj] = rowbase[r] >= 0 && sj < cnt && m0 + sj < rowlim[r] ? In<T>::cvt(raw[i]) : 0.0;
      else tile[r][sj] = rowbase[r] >= 0 && sj < cnt ? In<T>::cvt(raw[i]) : 0.0;
    }
    __syncthreads();
    CDouble* w = W + (m0 * p.K + k0) * 2;
    const int64_t wstep = 2 * (int64_t)p.K;
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {              // m0 + j is a multiple of 4: q = m & 3
      dft_term<G, 0>(pr, pi, tile[lane][j], w);
      dft_term<G, 1>(pr, pi, tile[lane][j + 1], w + wstep);
      dft_term<G, 2>(pr, pi, tile[lane][j + 2], w + 2 * wstep);
      dft_term<G, 3>(pr, pi, tile[lane][j + 3], w + 3 * wstep);
      w += 4 * wstep;
    }
    if (j < cnt) dft_term<G, 0>(pr, pi, tile[lane][j], w);                  // Nu mod 4 != 0: the last chunk's tail
    if (j + 1 < cnt) dft_term<G, 1>(pr, pi, tile[lane][j + 1], w + wstep);
    if (j + 2 < cnt) dft_term<G, 2>(pr, pi, tile[lane][j + 2], w + 2 * wstep);
  }
  if (y) {
#pragma unroll
    for (int i = 0; i < G; ++i)
      *reinterpret_cast<double2*>(y + 2 * (k0 + i)) =
          make_double2((pr[i][0] + pr[i][1]) + (pr[i][2] + pr[i][3]), (pi[i][0] + pi[i][1]) + (pi[i][2] + pi[i][3]));
  }
}

template <typename T>
__global__ __launch_bounds__(kWave) void k_ofdm_dft(const T* __restrict__ x, int64_t x_stride, int64_t n_streams,
                                                    OfdmParams p, CDouble* W, double* __restrict__ Y) {
  __shared__ double tile[kWave][kDftPitch];
  __shared__ int64_t rowbase[kWave];
  const int lane = threadIdx.x;
  const int64_t S = p.n_sym;
  const int64_t flat = (int64_t)blockIdx.x * kWave + lane;
  const bool live = flat < n_streams * S;
  {
    const int64_t b = live ? flat / S : 0;
    const int64_t s = flat - b * S;
    // the symbol's useful part: its last sample is b*x_stride + s*L + L - 1 <= b*x_stride + n - 1
    rowbase[lane] = live ? b * x_stride + s * p.L + p.ncp : -1;
  }
  double* const y = live ? Y + (size_t)flat * (size_t)p.K * 2 : nullptr;
  for (int k0 = 0; k0 < p.K; k0 += kDftGroup) {
    const int g = p.K - k0;                     // wave-uniform
    if (g >= 4) dft_group<T, 4>(x, p, W, k0, tile, rowbase, y, rowbase);
    else if (g == 3) dft_group<T, 3>(x, p, W, k0, tile, rowbase, y, rowbase);
    else if (g == 2) dft_group<T, 2>(x, p, W, k0, tile, rowbase, y, rowbase);
    else dft_group<T, 1>(x, p, W, k0, tile, rowbase, y, rowbase);
  }
}

// k_ofdm_dft at per-stream offsets: symbol s of stream b starts at sample
// offset[b] + s*L + Ncp of its row.  offset[b] >= -Ncp, so no row starts before
// sample 0; offset[b] <= L - 1 - Ncp, so every row starts below S*L <= n (the
// `safe` sample of lane 0 is always a real one) and only a stream's last
// symbol can pass n: its samples from n on are zeros, never loads.  A wave
// with no such row (all but about one in S / 64 of them, and none when the
// offsets leave the tails whole) takes k_ofdm_dft's own staging loop: the
// per-row limit costs a second LDS read and compare per load, and the staging
// loop is what the kernel's time is.
// rowbase and rowlim are written by one lane each and read by every lane with
// no barrier in between, as k_ofdm_dft reads its rowbase: the workgroup is one
// wave, and a wave's LDS operations complete in the order it issued them.
template <typename T>
__global__ __launch_bounds__(kWave) void k_ofdm_dft_at(const T* __restrict__ x, int64_t x_stride, int64_t n_streams,
                                                       OfdmParams p, CDouble* W,
                                                       const int64_t* __restrict__ offset, double* __restrict__ Y) {
  __shared__ double tile[kWave][kDftPitch];
  __shared__ int64_t rowbase[kWave];
  __shared__ int64_t rowlim[kWave];
  const int lane = threadIdx.x;
  const int64_t S = p.n_sym;
  const int64_t flat = (int64_t)blockIdx.x * kWave + lane;
  const bool live = flat < n_streams * S;
  {
    const int64_t b = live ? flat / S : 0;
    const int64_t s = flat - b * S;
    const int64_t i0 = live ? offset[b] + s * p.L + p.ncp : 0;   // 0 <= i0 < S*L
    rowbase[lane] = live ? b * x_stride + i0 : -1;
    rowlim[lane] = p.n - i0;
  }
  const bool cut = __any(live && rowlim[lane] < p.nu) != 0;   // wave-uniform: the workgroup is one wave
  double* const y = live ? Y + (size_t)flat * (size_t)p.K * 2 : nullptr;
  for (int k0 = 0; k0 < p.K; k0 += kDftGroup) {
    const int g = p.K - k0;                     // wave-uniform
    if (cut) {
      if (g >= 4) dft_group<T, 4, true>(x, p, W, k0, tile, rowbase, y, rowlim);
      else if (g == 3) dft_group<T, 3, true>(x, p, W, k0, tile, rowbase, y, rowlim);
      else if (g == 2) dft_group<T, 2, true>(x, p, W, k0, tile, rowbase, y, rowlim);
      else dft_group<T, 1, true>(x, p, W, k0, tile, rowbase, y, rowlim);
    } else {
      if (g >= 4) dft_group<T, 4>(x, p, W, k0, tile, rowbase, y, rowbase);
      else if (g == 3) dft_group<T, 3>(x, p, W, k0, tile, rowbase, y, rowbase);
      else if (g == 2) dft_group<T, 2>(x, p, W, k0, tile, rowbase, y, rowbase);
      else dft_group<T, 1>(x, p, W, k0, tile, rowbase, y, rowbase);
    }
  }
}

// ---------------------------------------------------------------------------
// The decision on d = Y[s+1][k] * conj(Y[s][k]) (numpy's fma form, as K4a):
//   ai < ar: m = dr > 0 ? 0 : 2;  else m = di > 0 ? 1 : 3;  dibit {0, 1, 3, 2}[m]
// Zeros, NaN and exact ties fall to the second line: the rule is total.
__device__ __forceinline__ void ofdm_product(double2 nx, double2 prev, double& dr, double& di) {
  const double br = prev.x, bi = -prev.y;
  dr = __builtin_fma(nx.x, br, -(nx.y * bi));
  di = __builtin_fma(nx.x, bi, nx.y * br);
}
__device__ __forceinline__ uint32_t ofdm_dibit(double dr, double di) {
  const double ar = fabs(dr), ai = fabs(di);
  if (ai < ar) return dr > 0 ? 0u : 3u;
  return di > 0 ? 1u : 2u;
}

// k_ofdm_slice: 16 consecutive lanes per output word, one dibit each: lane u of
// word w of stream b decides j = 16 w + u from Y[j] and Y[j + K] of the stream's
// [S][K] block (a wave reads 1 KiB of each, contiguous), the 16 dibits meet by
// an OR over the 16 lanes, and lane 0 of them stores the word.  (One lane per
// word -- 16 products each -- puts a wave's lanes 256 B apart in every load:
// that form took 2.7 ms for 78.6 M products; this one's time is in DESIGN.md §3j.)
__global__ __launch_bounds__(256) void k_ofdm_slice(const double* __restrict__ Y, int64_t n_streams, OfdmParams p,
                                                    uint32_t* __restrict__ words) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t wi = t >> 4;                    // flat word index b * n_words + w
  const int u = (int)(t & 15);
  const bool live = wi < n_streams * p.n_words;
  uint32_t g = 0u;
  if (live) {
    const int64_t b = wi / p.n_words, w = wi - b * p.n_words;
    const int64_t nd = p.n_bits >> 1;           // products per stream: K (S - 1)
    const int64_t j = 16 * w + u;
    if (j < nd) {
      const double2* __restrict__ y = reinterpret_cast<const double2*>(Y) + (size_t)b * (size_t)(p.n_sym * p.K);
      double dr, di;
      ofdm_product(y[j + p.K], y[j], dr, di);
      g = ofdm_dibit(dr, di) << (30 - 2 * u);
    }
  }
  // every lane of the wave takes part (no early exit above); the partners stay inside the 16 lanes
  g |= __shfl_xor(g, 1);
  g |= __shfl_xor(g, 2);
  g |= __shfl_xor(g, 4);
  g |= __shfl_xor(g, 8);
  if (live && u == 0) words[wi] = g;
}

// as psk_soft_kernels.hip soft_mag
__device__ __forceinline__ int ofdm_soft_mag(double num, double den) {
  const double r = num / den;
  const double q = floor(r * 127.0 + 0.5);
  if (!(q >= 1.0)) return 1;                    // NaN (0/0, inf/inf, a NaN component) and the decision edge
  return q > 127.0 ? 127 : (int)q;
}

// k_ofdm_soft: one thread per product, its two values side by side, so a
// block's 512 bytes are consecutive in the stream's row (Y is stream-major
// here; K4s's 64-stream tiles serve the PSK symbol layout).  The sign is the
// hard bit read back from the words, the window K4s's: soft[b][j], j < 8 *
// out_len[b], belongs to bit start + j, start = the sync index or 0.
__global__ __launch_bounds__(256) void k_ofdm_soft(const double* __restrict__ Y, int64_t n_streams, OfdmParams p,
                                                   const uint32_t* __restrict__ words,
                                                   const int64_t* __restrict__ sync_idx,
                                                   const int64_t* __restrict__ out_len, int8_t* __restrict__ soft,
                                                   int64_t soft_stride, int64_t blocks_per_stream) {
  const int64_t b = blockIdx.x / blocks_per_stream;
  const int64_t j = (blockIdx.x - b * blocks_per_stream) * 256 + threadIdx.x;
  const int64_t nd = p.n_bits >> 1;
  if (b >= n_streams || j >= nd) return;
  const int64_t sy = sync_idx ? sync_idx[b] : -1;
  const int64_t st = sy > 0 ? sy : 0;
  int64_t nv = out_len ? 8 * out_len[b] : p.n_bits;
  if (nv > p.n_bits - st) nv = p.n_bits - st;
  if (nv > soft_stride) nv = soft_stride;
  const double2* __restrict__ y = reinterpret_cast<const double2*>(Y) + (size_t)b * (size_t)(p.n_sym * p.K);
  double dr, di;
  ofdm_product(y[j + p.K], y[j], dr, di);
  const double den = fabs(dr) + fabs(di);
  const int mh = ofdm_soft_mag(fabs(dr + di), den), ml = ofdm_soft_mag(fabs(dr - di), den);
  const uint32_t dib = (words[(size_t)b * p.n_words + (size_t)(j >> 4)] >> (30 - 2 * (int)(j & 15))) & 3u;
  int8_t* __restrict__ row = soft + (size_t)b * (size_t)soft_stride;
  const int64_t o = 2 * j - st;
  if (o >= 0 && o < nv) row[o] = (int8_t)((dib & 2u) ? mh : -mh);
  if (o + 1 >= 0 && o + 1 < nv) row[o + 1] = (int8_t)((dib & 1u) ? ml : -ml);
}

// ---------------------------------------------------------------------------
// Transmit.  The bits [0,0]*30 + [1,1]*10 + payload, zero-padded to a multiple
// of 2 K; dibit j on symbol 1 + j / K, subcarrier j % K.
__device__ __forceinline__ uint32_t ofdm_tx_dibit(const uint8_t* __restrict__ d, int64_t nb, int64_t j) {
  if (j < 30) return 0u;
  if (j < 40) return 3u;
  const int64_t q = j - 40, byte = q >> 2;
  return byte < nb ? ((uint32_t)d[byte] >> (6 - 2 * (int)(q & 3))) & 3u : 0u;
}

// ---- begin ofdm_sin_cr ------------------------------------------------------
// The sine of a double, correctly rounded (up to arguments within 2^-100 of a
// rounding tie): a sample is a sum of K sines that may cancel to nothing, and
// then a last-ulp difference in one sine is the whole sample.  numpy's sin
// (libm's) returns the correctly rounded value for all but about one argument
// in a thousand; ocml's sin is within an ulp, which is not enough here.
// Double-double arithmetic (explicit fma for the exact products): the argument
// minus k * pi/2 with pi/2 in three doubles, then the Taylor series of sin or
// cos on [-pi/4, pi/4] to y^27 / y^28 (the next term is below 2^-113).
#ifndef AMR_HD
#define AMR_HD __host__ __device__
#endif
struct Dd { double hi, lo; };
AMR_HD inline Dd dd_quick(double a, double b) { const double s = a + b; return {s, b - (s - a)}; }
AMR_HD inline Dd dd_two_sum(double a, double b) {
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
AMR_HD inline Dd dd_two_prod(double a, double b) { const double p = a * b; return {p, __builtin_fma(a, b, -p)}; }
AMR_HD inline Dd dd_add(Dd a, Dd b) {
  const Dd s = dd_two_sum(a.hi, b.hi), t = dd_two_sum(a.lo, b.lo);
  const Dd u = dd_quick(s.hi, s.lo + t.hi);
  return dd_quick(u.hi, u.lo + t.lo);
}
AMR_HD inline Dd dd_mul(Dd a, Dd b) {
  const Dd p = dd_two_prod(a.hi, b.hi);
  return dd_quick(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}
AMR_HD inline double ofdm_sin_cr(double a) {
  // (-1)^j / (2j+1)! and (-1)^j / (2j)! as double-doubles
  const Dd ks[14] = {
      {0x1.0000000000000p+0, 0x0.0p+0},
      {-0x1.5555555555555p-3, -0x1.5555555555555p-57},
      {0x1.1111111111111p-7, 0x1.1111111111111p-63},
      {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73},
      {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73},
      {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80},
      {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87},
      {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97},
      {0x1.952c77030ad4ap-49, 0x1.ac981465ddc6cp-103},
      {-0x1.2f49b46814157p-57, -0x1.2650f61dbdcb4p-112},
      {0x1.71b8ef6dcf572p-66, -0x1.d043ae40c4647p-120},
      {-0x1.761b41316381ap-75, 0x1.3423c7d91404fp-130},
      {0x1.3f3ccdd165fa9p-84, -0x1.58ddadf344487p-139},
      {-0x1.d1ab1c2dccea3p-94, -0x1.054d0c78aea14p-149}};
  const Dd kc[15] = {
      {0x1.0000000000000p+0, 0x0.0p+0},
      {-0x1.0000000000000p-1, 0x0.0p+0},
      {0x1.5555555555555p-5, 0x1.5555555555555p-59},
      {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65},
      {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76},
      {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76},
      {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83},
      {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92},
      {0x1.ae7f3e733b81fp-45, 0x1.1d8656b0ee8cbp-101},
      {-0x1.6827863b97d97p-53, -0x1.eec01221a8b0bp-107},
      {0x1.e542ba4020225p-62, 0x1.ea72b4afe3c2fp-120},
      {-0x1.0ce396db7f853p-70, 0x1.aebcdbd20331cp-124},
      {0x1.f2cf01972f578p-80, -0x1.9ada5fcc1ab14p-135},
      {-0x1.88e85fc6a4e5ap-89, 0x1.71c37ebd16540p-143},
      {0x1.0a18a2635085dp-98, 0x1.b9e2e28e1aa54p-153}};
  if (a == 0.0 || !(fabs(a) < 0x1p20)) return sin(a);        // +-0 keeps its sign; huge, inf, NaN: not a sample's argument
  const double k = nearbyint(a * 0x1.45f306dc9c883p-1);      // a * (2 / pi), |k| < 2^20: k * a part of pi/2 is a two-prod
  const Dd p1 = dd_two_prod(k, 0x1.921fb54442d18p+0), p2 = dd_two_prod(k, 0x1.1a62633145c07p-54);
  Dd y = dd_two_sum(a, -p1.hi);                               // exact
  y = dd_add(y, {-p1.lo, 0.0});
  y = dd_add(y, {-p2.hi, -p2.lo});
  y = dd_add(y, {-(k * -0x1.f1976b7ed8fbcp-110), 0.0});
  const Dd z = dd_mul(y, y);
  const int q = (int)((long long)k & 3);
  Dd r;
  if (q & 1) {                                               // cos(y)
    r = kc[14];
    for (int j = 13; j >= 0; --j) r = dd_add(dd_mul(r, z), kc[j]);
  } else {                                                   // sin(y) = y * (1 - z/3! + ...)
    r = ks[13];
    for (int j = 12; j >= 0; --j) r = dd_add(dd_mul(r, z), ks[j]);
    r = dd_mul(r, y);
  }
  return q & 2 ? -r.hi : r.hi;
}
// ---- end ofdm_sin_cr --------------------------------------------------------

// k_tx_ofdm_phase: lane per (stream, subcarrier), sequential over symbols.
// ph[0][k] = (pi * (k*k)) / K (Newman phases), ph[s][k] = ph[s-1][k] + step,
// step 00 -> 0, 01 -> pi/2, 11 -> pi, 10 -> -pi/2: one rounding per symbol.
__global__ __launch_bounds__(kWave) void k_tx_ofdm_phase(const uint8_t* __restrict__ data, int64_t stride,
                                                         const int64_t* __restrict__ n_bytes, int64_t n_streams,
                                                         OfdmTx t, double* __restrict__ phase) {
  constexpr double kPi = 3.141592653589793;
  const int64_t flat = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (flat >= n_streams * t.K) return;
  const int64_t s = flat / t.K;
  const int k = (int)(flat - s * t.K);
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const uint8_t* __restrict__ d = data + s * stride;
  const int64_t total = ofdm_tx_symbols(nb, t.K);
  const int64_t n = total < t.sym_stride ? total : t.sym_stride;   // symbols stored
  double* __restrict__ out = phase + (size_t)s * (size_t)(t.sym_stride * t.K) + k;
  double ph = (kPi * (double)(k * k)) / (double)t.K;
  if (n > 0) out[0] = ph;
  for (int64_t q = 1; q < n; ++q) {
    const uint32_t dib = ofdm_tx_dibit(d, nb, (q - 1) * t.K + k);
    const double step = dib == 0u ? 0.0 : dib == 1u ? kPi / 2 : dib == 3u ? kPi : -kPi / 2;
    ph = ph + step;
    out[q * t.K] = ph;
  }
}

// k_tx_ofdm_synth: T2's shape, 4 consecutive samples per thread; K sin per
// sample, summed sequentially in k from 0.0, then * (1.0 / K) and the float32 cast.
template <bool VEC>
__global__ __launch_bounds__(256) void k_tx_ofdm_synth(const int64_t* __restrict__ n_bytes, int64_t stride, OfdmTx t,
                                                       const double* __restrict__ phase, float* __restrict__ out,
                                                       int64_t out_stride, int16_t* __restrict__ pcm,
                                                       int64_t pcm_stride) {
  constexpr double kTwoPi = 2 * 3.141592653589793;
  const int64_t s = blockIdx.y;
  int64_t nb = n_bytes[s];
  nb = nb < 0 ? 0 : (nb > stride ? stride : nb);
  const int64_t len = ofdm_tx_symbols(nb, t.K) * t.L;
  const double* __restrict__ ph = phase + (size_t)s * (size_t)(t.sym_stride * t.K);
  const double inv_k = 1.0 / (double)t.K, nu = (double)t.nu;
  const int64_t k0 = (int64_t)blockIdx.x * 1024 + 4 * threadIdx.x;
  if (k0 >= t.n_out) return;
  float f[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    f[u] = 0.0f;
    const int64_t idx = k0 + u;
    if (idx < len && idx < t.n_out) {
      const int64_t sym = idx / t.L, i = idx - sym * t.L;
      const int64_t m = i < t.ncp ? i - t.ncp + t.nu : i - t.ncp;      // (i - Ncp) mod Nu
      int64_t r = ((int64_t)t.bin0 * m) % t.nu;                         // (bins[k] * m) % Nu, k = 0
      const double* __restrict__ pk = ph + sym * t.K;
      double acc = 0.0;
      for (int k = 0; k < t.K; ++k) {
        acc = acc + ofdm_sin_cr(kTwoPi * ((double)r / nu) + pk[k]);
        r += m;
        if (r >= t.nu) r -= t.nu;
      }
      f[u] = (float)(acc * inv_k);
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

hipError_t launch_ofdm_dft(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const OfdmParams& p,
                           const double* W, double* Y, hipStream_t st) {
  const int64_t total = n_streams * p.n_sym;
  if (total < 1) return hipSuccess;
  const dim3 grid((unsigned)((total + kWave - 1) / kWave));
  CDouble* w = (CDouble*)W;
  if (dtype == kF32)
    hipLaunchKernelGGL(k_ofdm_dft<float>, grid, dim3(kWave), 0, st, (const float*)x, x_stride, n_streams, p, w, Y);
  else if (dtype == kF64)
    hipLaunchKernelGGL(k_ofdm_dft<double>, grid, dim3(kWave), 0, st, (const double*)x, x_stride, n_streams, p, w, Y);
  else if (dtype == kI16)
    hipLaunchKernelGGL(k_ofdm_dft<int16_t>, grid, dim3(kWave), 0, st, (const int16_t*)x, x_stride, n_streams, p, w,
                       Y);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_ofdm_dft_at(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const OfdmParams& p,
                              const double* W, const int64_t* offset, double* Y, hipStream_t st) {
  const int64_t total = n_streams * p.n_sym;
  if (total < 1) return hipSuccess;
  const dim3 grid((unsigned)((total + kWave - 1) / kWave));
  CDouble* w = (CDouble*)W;
  if (dtype == kF32)
    hipLaunchKernelGGL(k_ofdm_dft_at<float>, grid, dim3(kWave), 0, st, (const float*)x, x_stride, n_streams, p, w,
                       offset, Y);
  else if (dtype == kF64)
    hipLaunchKernelGGL(k_ofdm_dft_at<double>, grid, dim3(kWave), 0, st, (const double*)x, x_stride, n_streams, p, w,
                       offset, Y);
  else if (dtype == kI16)
    hipLaunchKernelGGL(k_ofdm_dft_at<int16_t>, grid, dim3(kWave), 0, st, (const int16_t*)x, x_stride, n_streams, p,
                       w, offset, Y);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_ofdm_slice(const double* Y, int64_t n_streams, const OfdmParams& p, uint32_t* words,
                             hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1) return hipSuccess;
  const int64_t total = n_streams * p.n_words * 16;   // a lane per dibit slot
  hipLaunchKernelGGL(k_ofdm_slice, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Y, n_streams, p, words);
  return hipGetLastError();
}

hipError_t launch_ofdm_soft(const double* Y, int64_t n_streams, const OfdmParams& p, const uint32_t* words,
                            const int64_t* sync_idx, const int64_t* out_len, int8_t* soft, int64_t soft_stride,
                            hipStream_t st) {
  if (n_streams < 1 || p.n_bits < 1 || soft_stride < 1) return hipSuccess;
  const int64_t bps = ((p.n_bits >> 1) + 255) / 256;
  hipLaunchKernelGGL(k_ofdm_soft, dim3((unsigned)(n_streams * bps)), dim3(256), 0, st, Y, n_streams, p, words,
                     sync_idx, out_len, soft, soft_stride, bps);
  return hipGetLastError();
}

hipError_t launch_ofdm_tx(const OfdmTx& t, const uint8_t* data, int64_t stride, const int64_t* n_bytes,
                          int64_t n_streams, double* phase, float* out, int64_t out_stride, int16_t* pcm,
                          int64_t pcm_stride, hipStream_t st) {
  if (n_streams < 1 || t.n_out < 1) return hipSuccess;
  const dim3 pg((unsigned)((n_streams * t.K + kWave - 1) / kWave));
  hipLaunchKernelGGL(k_tx_ofdm_phase, pg, dim3(kWave), 0, st, data, stride, n_bytes, n_streams, t, phase);
  const dim3 sg((unsigned)((t.n_out + 1023) / 1024), (unsigned)n_streams);
  const bool vec = (out_stride % 4) == 0 && ((uintptr_t)out % 16) == 0 &&
                   (!pcm || ((pcm_stride % 4) == 0 && ((uintptr_t)pcm % 8) == 0));
  if (vec)
    hipLaunchKernelGGL((k_tx_ofdm_synth<true>), sg, dim3(256), 0, st, n_bytes, stride, t, phase, out, out_stride, pcm,
                       pcm_stride);
  else
    hipLaunchKernelGGL((k_tx_ofdm_synth<false>), sg, dim3(256), 0, st, n_bytes, stride, t, phase, out, out_stride,
                       pcm, pcm_stride);
  return hipGetLastError();
}

}  // namespace amr
