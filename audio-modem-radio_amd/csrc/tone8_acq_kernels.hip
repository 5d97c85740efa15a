// tone8_acq_kernels.hip -- tone8 acquisition: where a frame
// starts and how far its tones are shifted, from one 2-D correlation of the
// Costas block over the capture's spectrogram.  tests/tone8_cases.py restates
// the kernels in numpy; float64, no fma, and the summation orders below are the
// specification: bit-equal.
//
//   k_tone8_acq      a chunk of start slots of one stream: slot sums, window energies, scores, the first maximum
//   k_tone8_peak     the scores and the first maximum of a chunk on given P (amr_tone8_peak_host)
//   k_tone8_acq_max  the chunks' maxima in order: start, shift, score
#include <hip/hip_runtime.h>

#include "psk_common.h"
#include "tone8.h"

namespace amr {
namespace {

constexpr int kT8AcqLdsEntries = 512;           // E in LDS when 2 L entries fit (8 KB)
constexpr int kT8Threads = 256;
constexpr int kT8PerThread = (kTone8Tile + kT8Threads - 1) / kT8Threads;   // window energies a thread holds
constexpr int kT8None = 0x7fffffff;

// the Costas tones 3, 1, 4, 0, 6, 5, 2 in nibbles, the first lowest
__device__ __forceinline__ int costas_tone(int s) { return (int)((0x2560413u >> (4 * s)) & 7u); }

// ---------------------------------------------------------------------------
// The scores of a chunk and its first maximum, from the chunk's window
// energies pt [(C + 48)][NB] in LDS (row jj = window j0 + jj, column li = line
// c2 - G + li).  Candidate t = jj (2 G + 1) + gi is start slot j0 + jj at shift
// g = gi - G, so ascending t is the rule's scan order: j ascending, g ascending
// within a j.
//   S = 0.0; for s = 0 .. 6: S = S + pt[jj + 8 s][gi + 2 costas[s]]
// The sequential rule's result, for a parallel search (as k_msk_acq_max): a
// thread scans its own candidates ascending with the strict comparison, a NaN
// never taken; across threads the larger value wins and, on equal values, the
// smaller t.  A chunk whose every score is NaN reports j = -1; `first` is the
// chunk's first score, which the per-stream kernel needs of chunk 0.
__device__ __forceinline__ void score_chunk(const double* __restrict__ pt, int NB, int G, int C, int64_t j0,
                                            int64_t nj, Tone8Cand* __restrict__ out) {
  __shared__ double rv[kT8Threads / kWave];
  __shared__ int rk[kT8Threads / kWave];
  __shared__ double first;
  const int tid = threadIdx.x;
  const int W = 2 * G + 1;
  const int64_t rows = nj - j0 < C ? nj - j0 : C;             // start slots of this chunk, >= 1
  const int total = (int)rows * W;
  double bv = 0.0;
  int bk = kT8None;
  for (int t = tid; t < total; t += kT8Threads) {
    const int jj = t / W, gi = t - jj * W;
    double S = 0.0;
#pragma unroll
    for (int s = 0; s < kTone8Costas; ++s) S = S + pt[(jj + 8 * s) * NB + gi + 2 * costas_tone(s)];
    if (t == 0) first = S;
    if (S == S && (bk == kT8None || S > bv)) {
      bv = S;
      bk = t;
    }
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const double ov = __shfl_xor(bv, m);
    const int ok = __shfl_xor(bk, m);
    if (ok != kT8None && (bk == kT8None || ov > bv || (ov == bv && ok < bk))) {
      bv = ov;
      bk = ok;
    }
  }
  if ((tid & (kWave - 1)) == 0) {
    rv[tid / kWave] = bv;
    rk[tid / kWave] = bk;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kT8Threads / kWave; ++w) {
      const double ov = rv[w];
      const int ok = rk[w];
      if (ok != kT8None && (bk == kT8None || ov > bv || (ov == bv && ok < bk))) {
        bv = ov;
        bk = ok;
      }
    }
    Tone8Cand c;
    c.score = bv;
    c.j = bk == kT8None ? -1 : j0 + bk / W;
    c.g = bk == kT8None ? 0 : bk % W - G;
    c.first = first;
    *out = c;
  }
}

// ---------------------------------------------------------------------------
// k_tone8_acq.  One workgroup per (stream, chunk of C start slots j0 .. j0 + C
// - 1).  The chunk needs the slots j0 .. j0 + C + 54 (a start slot's last
// Costas window begins 48 slots on and spans 8), so chunks overlap by 55 slots:
// x is re-read (from L2) and the slot sums redone by the factor 1 + 55 / C.
//
// 1. Slot sums.  One thread per (slot, line), flat t = slot * NB + line:
//      Z[j][f] = sum_{i<T} x[j T + i] * E[(f (j T + i)) % (2 L)]
//    sequential in i from 0.0, each product rounded before it is added.  The
//    table index is divided once, for i = 0, and then advanced by f < L with
//    one conditional subtraction.  The lanes of a slot load the same sample in
//    one instruction.  A slot at or past J = n / T is not read: 0.0.
// 2. Window energies.  One thread per (window, line), kept in registers while
//    the tile still holds Z:
//      Wd = ((Z0 + Z1) + (Z2 + Z3)) + ((Z4 + Z5) + (Z6 + Z7)), P = re * re + im * im
//    then written over the tile as pt [(C + 48)][NB].
// 3. score_chunk.
// E is read from LDS when its 2 L entries fit kT8AcqLdsEntries, from global
// memory otherwise.  LDS: the 51 KB tile + 8 KB: two workgroups per CU.
template <typename T, bool LDS>
__global__ __launch_bounds__(kT8Threads) void k_tone8_acq(const T* __restrict__ x, int64_t x_stride, Tone8Params p,
                                                          int64_t chunks, const double2* __restrict__ E,
                                                          Tone8Cand* __restrict__ cand) {
  __shared__ double2 zt[kTone8Tile];
  __shared__ double2 es[LDS ? kT8AcqLdsEntries : 1];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / chunks, q = blockIdx.x - b * chunks;
  const int64_t j0 = q * p.C;
  const int NB = (int)p.NB, C = (int)p.C;
  const uint32_t P2 = (uint32_t)(2 * p.L);      // <= 2^25
  if constexpr (LDS) {
    for (uint32_t i = tid; i < P2; i += kT8Threads) es[i] = E[i];
    __syncthreads();
  }
  const T* __restrict__ xb = x + b * x_stride;
  const int nz = (C + kTone8Ahead) * NB;        // <= kTone8Tile
  for (int t = tid; t < nz; t += kT8Threads) {
    const int sl = t / NB, li = t - sl * NB;
    const int64_t j = j0 + sl;
    double zr = 0.0, zi = 0.0;
    if (j < p.J) {
      const uint32_t f = (uint32_t)(p.c2 - p.G + li);         // 2 <= f < L
      const int64_t m0 = j * p.T;
      uint32_t idx = (uint32_t)(((uint64_t)(m0 % (int64_t)P2) * f) % P2);
      const T* __restrict__ xs = xb + m0;                     // m0 + T <= J T <= n
      for (int64_t i = 0; i < p.T; ++i) {
        const double xv = In<T>::cvt(xs[i]);
        const double2 e = LDS ? es[idx] : E[idx];
        zr = zr + xv * e.x;
        zi = zi + xv * e.y;
        idx += f;
        if (idx >= P2) idx -= P2;
      }
    }
    zt[t] = make_double2(zr, zi);
  }
  __syncthreads();
  const int np = (C + kTone8Span) * NB;         // < nz
  double pw[kT8PerThread];
#pragma unroll
  for (int k = 0; k < kT8PerThread; ++k) {
    const int t = tid + k * kT8Threads;
    pw[k] = 0.0;
    if (t < np) {
      double2 z[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) z[s] = zt[t + s * NB];      // the same line of the next slot is NB on
      const double re = ((z[0].x + z[1].x) + (z[2].x + z[3].x)) + ((z[4].x + z[5].x) + (z[6].x + z[7].x));
      const double im = ((z[0].y + z[1].y) + (z[2].y + z[3].y)) + ((z[4].y + z[5].y) + (z[6].y + z[7].y));
      pw[k] = re * re + im * im;
    }
  }
  __syncthreads();                              // every read of Z is done
  double* const pt = reinterpret_cast<double*>(zt);
#pragma unroll
  for (int k = 0; k < kT8PerThread; ++k) {
    const int t = tid + k * kT8Threads;
    if (t < np) pt[t] = pw[k];
  }
  __syncthreads();
  score_chunk(pt, NB, (int)p.G, C, j0, p.nj, cand + blockIdx.x);
}

// k_tone8_peak: the same chunks on a given P [n_win][NB] of each stream; a window at or past n_win counts as 0.0
__global__ __launch_bounds__(kT8Threads) void k_tone8_peak(const double* __restrict__ P, int64_t n_win, int NB, int G,
                                                           int C, int64_t chunks, Tone8Cand* __restrict__ cand) {
  __shared__ double pt[kTone8Tile];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x / chunks, q = blockIdx.x - b * chunks;
  const int64_t j0 = q * C;
  const double* __restrict__ pb = P + ((size_t)b * (size_t)n_win + (size_t)j0) * (size_t)NB;
  const int np = (C + kTone8Span) * NB;
  const int64_t have = (n_win - j0) * NB;       // entries of the stream's P from window j0 on, > 0
  for (int t = tid; t < np; t += kT8Threads) pt[t] = t < have ? pb[t] : 0.0;
  __syncthreads();
  score_chunk(pt, NB, G, C, j0, n_win - kTone8Span, cand + blockIdx.x);
}

// ---------------------------------------------------------------------------
// k_tone8_acq_max.  k_msk_acq_max's shape: one wave per stream over the chunks'
// maxima in chunk order.  The rule: best = (0, -G); every later candidate in
// scan order wins only if strictly greater.  So a NaN first score keeps (0, -G)
// and is the score; otherwise the result is the first of the greatest non-NaN
// scores: chunks hold disjoint ascending ranges of j, a lane takes its chunks
// ascending with the strict comparison, across lanes the larger value wins and,
// on equal values, the smaller j.  No chunk (nj <= 0): start 0, shift 0, score 0.0.
__global__ __launch_bounds__(kWave) void k_tone8_acq_max(const Tone8Cand* __restrict__ cand, int64_t chunks, int64_t T,
                                                         int64_t G, int64_t* __restrict__ start,
                                                         int64_t* __restrict__ shift, double* __restrict__ score) {
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const Tone8Cand* __restrict__ cb = cand + (size_t)b * (size_t)chunks;
  double bv = 0.0;
  int64_t bj = -1, bg = 0;
  for (int64_t q = lane; q < chunks; q += kWave) {
    const Tone8Cand c = cb[q];
    if (c.j >= 0 && (bj < 0 || c.score > bv)) {
      bv = c.score;
      bj = c.j;
      bg = c.g;
    }
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) {
    const double ov = __shfl_xor(bv, m);
    const int64_t oj = __shfl_xor(bj, m);
    const int64_t og = __shfl_xor(bg, m);
    if (oj >= 0 && (bj < 0 || ov > bv || (ov == bv && oj < bj))) {
      bv = ov;
      bj = oj;
      bg = og;
    }
  }
  if (lane == 0) {
    int64_t s = 0, g = 0;
    double v = 0.0;
    if (chunks > 0) {
      const double first = cb[0].first;
      if (first != first || bj < 0) {           // bj < 0 only with a NaN first score
        g = -G;
        v = first;
      } else {
        s = bj * T;
        g = bg;
        v = bv;
      }
    }
    start[b] = s;
    shift[b] = g;
    if (score) score[b] = v;
  }
}

template <typename T>
hipError_t acq_launch(const void* x, int64_t x_stride, const Tone8Params& p, int64_t chunks, dim3 grid,
                      const double* E, Tone8Cand* cand, hipStream_t st) {
  const double2* e = reinterpret_cast<const double2*>(E);
  if (2 * p.L <= kT8AcqLdsEntries)
    hipLaunchKernelGGL((k_tone8_acq<T, true>), grid, dim3(kT8Threads), 0, st, (const T*)x, x_stride, p, chunks, e,
                       cand);
  else
    hipLaunchKernelGGL((k_tone8_acq<T, false>), grid, dim3(kT8Threads), 0, st, (const T*)x, x_stride, p, chunks, e,
                       cand);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_tone8_acquire(const void* x, int dtype, int64_t x_stride, int64_t n_streams, const Tone8Params& p,
                                const double* E, Tone8Cand* cand, int64_t* start, int64_t* shift, double* score,
                                hipStream_t st) {
  if (n_streams < 1) return hipSuccess;
  const int64_t chunks = tone8_acq_chunks(p);
  if (chunks > 0) {
    const int64_t blocks = n_streams * chunks;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    hipError_t e = hipErrorInvalidValue;
    if (dtype == kF32) e = acq_launch<float>(x, x_stride, p, chunks, grid, E, cand, st);
    else if (dtype == kF64) e = acq_launch<double>(x, x_stride, p, chunks, grid, E, cand, st);
    else if (dtype == kI16) e = acq_launch<int16_t>(x, x_stride, p, chunks, grid, E, cand, st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_tone8_acq_max, dim3((unsigned)n_streams), dim3(kWave), 0, st, cand, chunks, p.T, p.G, start,
                     shift, score);
  return hipGetLastError();
}

hipError_t launch_tone8_peak(const double* P, int64_t n_streams, int64_t n_win, int64_t T, int64_t G, Tone8Cand* cand,
                             int64_t* start, int64_t* shift, double* score, hipStream_t st) {
  if (n_streams < 1) return hipSuccess;
  const int64_t C = tone8_chunk(G);
  const int64_t nj = n_win > kTone8Span ? n_win - kTone8Span : 0;
  const int64_t chunks = (nj + C - 1) / C;
  if (chunks > 0) {
    const int64_t blocks = n_streams * chunks;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tone8_peak, dim3((unsigned)blocks), dim3(kT8Threads), 0, st, P, n_win, (int)tone8_lines(G),
                       (int)G, (int)C, chunks, cand);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_tone8_acq_max, dim3((unsigned)n_streams), dim3(kWave), 0, st, cand, chunks, T, G, start, shift,
                     score);
  return hipGetLastError();
}

}  // namespace amr
