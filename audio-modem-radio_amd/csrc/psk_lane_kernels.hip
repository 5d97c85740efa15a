// psk_lane_kernels.hip -- the PSK filtfilt passes with ONE STREAM PER LANE
// (the throughput layout), for gfx950.
//
// Same reference arithmetic as psk_kernels.hip (K1r/K1g band-pass, K2q/K3q
// low-pass; modem.py:194-204 -> scipy filtfilt/lfilter in DF-II-T order, no
// contraction), the same buffers downstream (f in s2 for the low-pass and
// K3x, symbols in s1 for K4a) and the same low-pass zero/denormal detector,
// so every stream's bytes are identical whichever layout ran.
//
// Why a second layout.  The state-per-lane kernels spread one stream over
// 4-16 lanes to keep ~1000 waves busy at B = 4096, but half of their
// instructions move states between lanes (DPP, selects), and their lanes do
// 8-16x the arithmetic one lane needs: measured register-only
// (tools/step_probe3.hip, one wave per SIMD) a lane-per-stream band-pass
// step issues 34 FP64 instructions for 64 streams and sustains 921
// stream-samples/ns against 303 for the 8-lane groups of K1g; the low-pass
// per component 1452 against 592 (quads).  The FP64 pipe is saturated at one
// wave per SIMD.  The price is parallelism: B = 4096 is only 64 band-pass
// waves, so this layout is picked when enough streams are in flight on the
// device (api.cpp) -- several batches at once, or big batches.
//
// Intermediates not written to HBM (checkpoint + recompute):
//   * band-pass (k_bp_lane2, two waves per group of 64 streams): the forward
//     pass keeps the filter state at the start of every kBpT-sample tile (8
//     doubles); then one wave re-runs each tile forward from its checkpoint
//     into LDS while the other filters the tile before it backward out of LDS
//     -- the forward output s1 (2 x 8 B/sample of HBM traffic in the round-1
//     kernels) becomes 4 B/sample of re-read input plus 4 B/sample of
//     checkpoints.
//   * low-pass (k_lp_lane): the same in one wave over f with kLpT-sample
//     tiles, each re-run into registers and filtered backward from there (4
//     doubles per component) -- the complex forward output s3 (2 x 16
//     B/sample) becomes a second read of f (8 B/sample, mostly L2: the re and
//     im waves of the same streams run on one XCD) plus 2 B/sample of
//     checkpoints.  Symbols are written straight from the backward pass.
//   * low-pass with the slicer fused (from 32768 live streams, static symbol
//     slots): k_lp_lane_h, both components of 32 streams in one wave -- f is
//     fetched once per group and pass, the symbol samples go from the
//     backward pass through a half-wave swap into the slicer, and only the
//     decided words leave the chip; no LDS symbol ring and no workgroup
//     barrier.  AMR_LP_HALF=0 keeps the earlier two-wave form (k_lp_lane
//     FUSE: a component per wave, ring + one barrier per slicing region).
// A re-run tile executes exactly the operations the forward pass executed,
// from exactly the same state, so it reproduces its outputs bit for bit.
#include <math.h>

#include <type_traits>
#include <utility>

#include "amr.h"
#include "amr_internal.h"
#include "env_switch.h"
#include "psk_common.h"

namespace amr {

constexpr int kBpT = 32;    // band-pass checkpoint tile (samples)
constexpr int kLpT = 40;     // low-pass checkpoint tile: a multiple of sps 5 / 10 / 20 (static symbol slots)
// The static symbol slots number tile t's symbols from t * (kLpT / SPS) -
// first / SPS, which is valid (>= 0 from the first recomputed tile on) while
// first is at most the tile length; a plan with a later first sample takes the
// generic kernel.  20 is conservative for the 40-sample tile; it decides which
// low-pass a plan gets (amr_psk_plan_last_lowpass), so it keeps its value.
constexpr int kLpStaticFirstMax = 20;
// s3 reserves a checkpoint row per 20 samples: twice what kLpT needs.  The
// plans' scratch totals are pinned to the byte (amr_psk_plan_scratch_bytes);
// shrinking the reservation is a footprint change for a change of its own.
constexpr int kLpCkReserveT = 20;

// (the DF-II-T step functions df2t_step / df2t_step_zo / lp_step: psk_common.h)

// ZO: 0 every tap; kZoY the zero odd taps skipped, the detector on y
// (bp_watch, one v_min3_f32 per pair of steps); kZoZ the same steps under the
// earlier four-state detector inside the step (AMR_BP_ZDET=0)
constexpr int kZoY = 1, kZoZ = 2;
template <int ZO>
__device__ __forceinline__ double bp_step(double (&z)[8], const Iir& f, double x, float& acc) {
  if constexpr (ZO == kZoZ) return df2t_step_zo(z, f, x, acc);
  else if constexpr (ZO == kZoY) return bp_step_zo(z, f, x);
  else return df2t_step<8>(z, f, x);
}
// the outputs of the two steps just taken (of a single step: y twice)
template <int ZO>
__device__ __forceinline__ void bp_watch(float& acc, double y0, double y1) {
  if constexpr (ZO == kZoY) zo_watch_y(acc, y0, y1);
}

template <int ZO>
__device__ __forceinline__ bool bp_bad(float acc, const double (&z)[8]) {
  if constexpr (!ZO) return false;
  bool bad = !(acc >= kTinyHi);
#pragma unroll
  for (int j = 0; j < 8; ++j) bad |= !__builtin_isfinite(z[j]);
  return bad;
}

// checkpoint + edge scratch inside the plan's s1 (band-pass) / s3 (low-pass)
__host__ __device__ inline int64_t bp_lane_edge_cap(int pad) { return kBpT + pad; }
__host__ __device__ inline int64_t lp_lane_edge_cap(int pad) { return 2 * (kLpT + pad); }
int64_t psk_lane_bp_scratch_doubles(int64_t n_streams, int64_t n, int pad) {
  const int64_t g = (n_streams + 63) / 64;
  return g * ((n / kBpT) * 8 + bp_lane_edge_cap(pad)) * 64;
}
int64_t psk_lane_lp_scratch_doubles(int64_t n_streams, int64_t n, int pad) {
  const int64_t g = (n_streams + 63) / 64;
  return 2 * g * ((n / kLpCkReserveT) * 4 + lp_lane_edge_cap(pad)) * 64;
}

// ---------------------------------------------------------------------------
// band-pass: lane = stream, two waves per group of 64 streams (GPB groups per
// workgroup).  Coefficients are wave-uniform (kernel arguments in SGPRs).
// s1 = [G][nt][8][64] checkpoints, then [G][edge][64] tail outputs.
// Wave 0 runs the forward pass (a checkpoint at the start of every tile, no
// output; the tail's edge outputs) while wave 1 waits; then, tile by tile from
// the end, wave 0 re-runs tile t-1 forward from its checkpoint into one LDS
// buffer while wave 1 filters tile t backward out of the other buffer and
// stores f -- the backward pass and the re-run overlap, so the kernel takes
// two passes of latency instead of three.  One workgroup barrier per tile.
// Two forms are instantiated:
//   * GPB = 2, any ZO: the band-pass launch, two groups per 256-thread
//     workgroup.
//   * GPB = 1, FIXUP (every tap, float64 f): the re-run of the groups the
//     zero-tap launch (or the float32 hand-off's margin check) flagged; a
//     workgroup whose group has no flagged stream returns before its first
//     barrier (2-wave, 108-VGPR workgroups find room beside the resident
//     band-pass / low-pass waves).
// F32F (PskBuffers::f32f): f is stored rounded to float32 into the first half
// of the group's s2 slot (the f64 layout's element order, float elements),
// and each stream's max |f| (bits: NaN / inf dominate) into buf.fpeak.
// NT: which access classes go non-temporal (psk_common.h: kNtFStore the f
// stores, kNtCk the checkpoints and edge rows, kNtX the x tiles); 0 with F32F.
template <typename T, int GPB, int ZO, bool FIXUP = false, bool F32F = false, int NT = 0>
__global__ __launch_bounds__(128 * GPB) void k_bp_lane2(PskBuffers buf, PskParams p, Iir f, int dev_fence) {
  static_assert(FIXUP ? GPB == 1 && !ZO && !F32F : GPB == 2,
                "two groups per workgroup, or the fix-up pass: one group, every tap, float64 f");
  static_assert(NT == 0 || !F32F, "cache policies: the float64 paths only");
  constexpr bool NTF = (NT & kNtFStore) != 0, NTC = (NT & kNtCk) != 0, NTX = (NT & kNtX) != 0;
  constexpr int TB = kBpT;
  constexpr int PER = 16 / (int)sizeof(T);
  constexpr int NL = TB / PER;
  static_assert(TB % PER == 0 && TB % 2 == 0, "tile = whole loads and whole pairs");
  __shared__ __attribute__((aligned(16))) double2 yb[GPB][2][TB / 2][64];   // forward outputs of a tile, by pairs
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gi = wv >> 1, role = wv & 1;
  const int64_t w = (int64_t)blockIdx.x * GPB + gi;
  const bool active = w * 64 < buf.n_streams;   // inactive groups still meet every barrier
  const int64_t last = buf.n_streams - 1;
  const int64_t s = w * 64 + lane;
  if constexpr (FIXUP) {
    if (!active) return;                        // workgroup-uniform (one group)
    if (!__syncthreads_or(s <= last && buf.bp_flags[s] != 0)) return;   // nothing flagged in this group
  }
  const T* __restrict__ x = reinterpret_cast<const T*>(buf.x) + (s < last ? s : last) * buf.x_stride;
  const uint8_t* __restrict__ xb = reinterpret_cast<const uint8_t*>(x);
  const int64_t n = p.n, n2 = (n + 1) >> 1;
  const int pad = p.pad1;
  const int64_t nt = n / TB;
  const int64_t G = (buf.n_streams + 63) / 64;
  const int64_t ecap = bp_lane_edge_cap(pad);
  const int64_t i_tail = nt * TB;
  const int ne = (int)(n - i_tail) + pad;
  double* __restrict__ ck = buf.s1 + (size_t)w * nt * 8 * 64 + lane;
  double* __restrict__ eb = buf.s1 + (size_t)G * nt * 8 * 64 + (size_t)w * ecap * 64 + lane;
  double* __restrict__ fo = buf.s2 + (size_t)(w * 2 + (lane >> 5)) * n2 * 64 + (lane & 31) * 2;
  [[maybe_unused]] float* __restrict__ fo32 =
      reinterpret_cast<float*>(buf.s2 + (size_t)w * 2 * n2 * 64) + (size_t)(lane >> 5) * n2 * 64 + (lane & 31) * 2;

  auto load_tile = [&](int64_t t, v4u (&r)[NL]) {
#pragma unroll
    for (int k = 0; k < NL; ++k)
      r[k] = ld_pol<NTX>(reinterpret_cast<const v4u*>(xb + (size_t)t * TB * sizeof(T) + k * 16));
  };
  auto tile_x = [&](const v4u (&r)[NL], int k) -> double {
    T v[PER];
    __builtin_memcpy(v, &r[k / PER], 16);
    return In<T>::cvt(v[k % PER]);
  };

  if (role == 0 && active) {
    // ---- forward pass: pads + tiles (checkpoints only) + tail (edge) ------
    // (written out here, not a device function: through one the compiler
    // kept 238 VGPRs live against 113); the zero-tap detector flags a stream
    // it cannot vouch for
    double z[8];
    float acc = __builtin_inff();
    const OddExt<T> ox(x, buf.edge, s < last ? s : last, n, pad);
    {
      const double e0 = ox.left(0);
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = f.zi[j] * e0;
    }
    for (int jj = 0; jj < pad; ++jj) {
      const double y = bp_step<ZO>(z, f, ox.left(jj), acc);
      bp_watch<ZO>(acc, y, y);
    }
    v4u xr[NL];
    if (nt > 0) load_tile(0, xr);
    for (int64_t t = 0; t < nt; ++t) {
#pragma unroll
      for (int j = 0; j < 8; ++j) st_pol<NTC>(&ck[(t * 8 + j) * 64], z[j]);
      v4u cur[NL];
#pragma unroll
      for (int k = 0; k < NL; ++k) cur[k] = xr[k];
      load_tile(t + 1 < nt ? t + 1 : t, xr);
#pragma unroll
      for (int k = 0; k < TB; k += 2) {
        const double y0 = bp_step<ZO>(z, f, tile_x(cur, k), acc);
        const double y1 = bp_step<ZO>(z, f, tile_x(cur, k + 1), acc);
        bp_watch<ZO>(acc, y0, y1);
      }
    }
    int e = 0;
    for (int64_t i = i_tail; i < n; ++i) {
      const double y = bp_step<ZO>(z, f, In<T>::cvt(x[i]), acc);
      bp_watch<ZO>(acc, y, y);
      st_pol<NTC>(&eb[(e++) * 64], y);
    }
    for (int jj = 0; jj < pad; ++jj) {
      const double y = bp_step<ZO>(z, f, ox.right(jj), acc);
      bp_watch<ZO>(acc, y, y);
      st_pol<NTC>(&eb[(e++) * 64], y);
    }
    if (bp_bad<ZO>(acc, z) && s <= last) atomicOr(&buf.bp_flags[s], 1);
    // the checkpoints are re-read by this wave (its re-run role below), the
    // edge rows by the backward wave of the same workgroup behind the barrier
    // that follows: nothing stored here is read by another workgroup
    lane_pass_fence(dev_fence);
  }
  __syncthreads();

  if (role == 0) {
    // ---- re-run tiles nt-1, nt-2, ... 0 forward into LDS --------------------
    v4u xr[NL];
    double cn[8];
    if (active && nt > 0) {
      load_tile(nt - 1, xr);
#pragma unroll
      for (int j = 0; j < 8; ++j) cn[j] = ld_pol<NTC>(&ck[((nt - 1) * 8 + j) * 64]);
    }
    for (int64_t it = 0; it <= nt; ++it) {
      const int64_t t = nt - 1 - it;
      if (active && t >= 0) {
        double zf[8];
        v4u cur[NL];
#pragma unroll
        for (int j = 0; j < 8; ++j) zf[j] = cn[j];
#pragma unroll
        for (int k = 0; k < NL; ++k) cur[k] = xr[k];
        const int64_t tp = t > 0 ? t - 1 : 0;
        load_tile(tp, xr);
#pragma unroll
        for (int j = 0; j < 8; ++j) cn[j] = ld_pol<NTC>(&ck[(tp * 8 + j) * 64]);
        double2 (*ybuf)[64] = yb[gi][it & 1];
        float dummy = 0.0f;                     // the re-run repeats checked steps: no detector
#pragma unroll
        for (int k = 0; k < TB; k += 2) {
          const double y0 = bp_step<ZO>(zf, f, tile_x(cur, k), dummy);
          const double y1 = bp_step<ZO>(zf, f, tile_x(cur, k + 1), dummy);
          ybuf[k >> 1][lane] = make_double2(y0, y1);
        }
      }
      __syncthreads();
    }
  } else {
    // ---- backward pass: the tail edge, then the tiles out of LDS -------------
    double zb[8];
    float acc = __builtin_inff();
    unsigned long long pk = 0;                  // F32F: max |f| as bits
    auto pk_acc = [&](double y) {
      if constexpr (F32F) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(y) & 0x7fffffffffffffffULL;
        pk = b > pk ? b : pk;
      }
    };
    if (active) {
      const double ylast = ld_pol<NTC>(&eb[(ne - 1) * 64]);
#pragma unroll
      for (int j = 0; j < 8; ++j) zb[j] = f.zi[j] * ylast;
      for (int e = ne - 1; e >= 0; --e) {
        const double y = bp_step<ZO>(zb, f, ld_pol<NTC>(&eb[e * 64]), acc);
        bp_watch<ZO>(acc, y, y);
        const int64_t i = i_tail + e;
        if (i < n) {
          if constexpr (F32F) {
            fo32[(i >> 1) * 64 + (i & 1)] = (float)y;
            pk_acc(y);
          } else {
            st_pol<NTF>(&fo[(i >> 1) * 64 + (i & 1)], y);
          }
        }
      }
    }
    __syncthreads();                            // tile nt-1 is in buffer 0
    for (int64_t it = 1; it <= nt; ++it) {
      const int64_t t = nt - it;
      if (active) {
        const double2 (*ybuf)[64] = yb[gi][(it - 1) & 1];
        double* const fp = fo + (size_t)(t * (TB / 2)) * 64;
        float* const fp32 = fo32 + (size_t)(t * (TB / 2)) * 64;
#pragma unroll
        for (int k = TB / 2 - 1; k >= 0; --k) {
          const double2 yy = ybuf[k][lane];
          const double y1 = bp_step<ZO>(zb, f, yy.y, acc);
          const double y0 = bp_step<ZO>(zb, f, yy.x, acc);
          bp_watch<ZO>(acc, y1, y0);
          if constexpr (F32F) {
            *reinterpret_cast<float2*>(fp32 + k * 64) = make_float2((float)y0, (float)y1);
            pk_acc(y0);
            pk_acc(y1);
          } else {
            st_pair<NTF>(fp + k * 64, y0, y1);
          }
        }
      }
      __syncthreads();
    }
    if (active && bp_bad<ZO>(acc, zb) && s <= last) atomicOr(&buf.bp_flags[s], 1);
    if constexpr (F32F) {
      if (active && s <= last) buf.fpeak[s] = __longlong_as_double((long long)pk);
    }
  }
}

// ---------------------------------------------------------------------------
// low-pass: lane = stream, wave = 64 streams x ONE component (so the LO
// multiplier is wave-uniform), four waves per workgroup: waves (2i, 2i+1) of
// a block are the re and im waves of one stream group, on one CU, so the
// second read of f is a cache hit (PMC: f is read from HBM once per pass).
// Mixer and detector exactly as K2q/K3q (psk_kernels.hip): bb[0] in numpy's
// full complex-multiply form, every other sample f*lo_c (equal whenever it
// is not a zero, and a zero is flagged); min over |hi words| of every input
// and output (forward) and every output (backward), final states finite.
// s3 = [2G][nt][4][64] checkpoints, then [2G][edge][64]: the head (pre-pad
// + tile 0) and tail (last partial tile + post-pad) forward outputs.
// SPS > 0: symbols at tile offsets FM + k*SPS (kLpT % SPS == 0, first % SPS
// == FM); SPS == 0: any sps (run-time symbol test per sample).
// Memory: f streams through a ring of NCH chunk slots (the next tile's chunk
// c is loaded as soon as this tile's chunk c is consumed: a tile of compute
// to arrive); the tile's LO multipliers arrive by one 8-B load per lane a tile
// ahead and are parked in a per-wave LDS double buffer, read back by
// broadcast ds_read_b128.
// (Tried: 3 waves per SIMD through a half-tile ring (CH 4), and a 20-sample
// tile at 4 waves per SIMD: both slower in flight and alone -- the loads
// need the whole tile of lead.)
#ifndef AMR_LP_WAVES
#define AMR_LP_WAVES 1
#endif
#ifndef AMR_LP_CH
#define AMR_LP_CH 8
#endif
#ifndef AMR_LP_REGION_SYMS
#define AMR_LP_REGION_SYMS 8     // fused slicer: symbols per slicing region at most (a power of two >= TL / sps)
#endif
// FUSE (static symbol slots): the slicer runs inside the backward
// pass.  Both component waves of a group park their symbol samples in an LDS
// ring (16 slots: a region -- the tail, RT tiles, the head -- holds at most 8
// symbols, and two consecutive regions never share a slot), meet at one
// workgroup barrier per region (RT = 2 tiles at sps 10: half the barriers of
// one per tile, a lone batch's low-pass 14.5 -> 13.7 ms; 16-symbol regions
// in a 32-slot ring measured slower), and the re wave forms s[k+1] * conj(s[k]),
// the sector decision (qpsk_dibit, as K4a) and the MSB-first words, storing
// each word as it completes.  No symbol leaves the chip (0.63 GB written and
// read back per 4096-stream batch before); streams the detector flags get
// their symbols from K3x and their words from K4a afterwards.
// F32F (with FUSE; PskBuffers::f32f): f arrives rounded to float32 (k_bp_lane2
// F32F), so the symbols differ from the reference's by at most
// E = p.f32_margin * fpeak[s] + 2^-120 (the rounding through the low-pass's L1
// gain, api.cpp f32_design); the re wave flags every decision within E of its
// boundary -- QPSK ||di| - |dr||, BPSK |dr| against sqrt2 E (|s0|_1 + |s1|_1 +
// E) -- into flags and bp_flags, and the fix-up band-pass, K3x and K4a redo
// those streams exactly.
// NT (float64 f): which access classes go non-temporal
// (psk_common.h: kNtFLoad the f loads, kNtCk the checkpoints and edges,
// kNtWords the fused slicer's word stores).
template <int SPS, int FM, bool FUSE = false, bool F32F = false, int NT = 0>
__global__ __launch_bounds__(256, SPS > 0 ? AMR_LP_WAVES : 1) void k_lp_lane(PskBuffers buf, PskParams p, Iir f,
                                                                            int dev_fence) {
  constexpr int WPB = 4;                        // waves per workgroup: two groups x (re, im)
  static_assert(NT == 0 || !F32F, "cache policies: the float64 paths only");
  constexpr bool NTF = (NT & kNtFLoad) != 0, NTC = (NT & kNtCk) != 0, NTW = (NT & kNtWords) != 0;
  static_assert(!FUSE || SPS > 0, "fused slicing: static slots");
  static_assert(!F32F || FUSE, "the float32 hand-off's margin check runs in the fused slicer");
  using FV = typename std::conditional<F32F, float2, double2>::type;
  constexpr int TL = kLpT;
  constexpr int CH = AMR_LP_CH;                 // samples per f chunk (CH / 2 x 16 B per lane)
  constexpr int NCH = TL / CH, HC = CH / 2;
  constexpr int R = NCH % 2 == 0 ? NCH / 2 : NCH;   // ring slots: chunk q lands R chunks ahead of its use
  static_assert(TL % CH == 0 && TL <= 64, "tile = whole chunks; one LO value per lane");
  static_assert(SPS == 0 || (TL % SPS == 0 && FM < SPS), "static symbol slots");
  __shared__ __attribute__((aligned(16))) double lo_lds[WPB][2][TL];
  // FUSE: tiles per slicing region (one barrier each) -- as many as keep a
  // region within MS symbols -- and a ring of 2 MS symbol slots per wave (two
  // consecutive regions never share a slot)
  constexpr int SPR = TL / (SPS > 0 ? SPS : TL);                 // symbols per tile (static slots)
  constexpr int MS = AMR_LP_REGION_SYMS;
  constexpr int RT = MS / SPR > 1 ? MS / SPR : 1;
  constexpr int NSL = FUSE ? 2 * MS : 1;
  static_assert(!FUSE || (RT * SPR <= MS && (MS & (MS - 1)) == 0), "a region holds at most MS symbols");
  __shared__ double sring[FUSE ? WPB : 1][NSL][64];   // FUSE: symbol samples k at slot k & (NSL - 1)
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w = (int64_t)blockIdx.x * (WPB / 2) + (wv >> 1);
  const int comp = wv & 1;
  const int64_t n = p.n, n2 = (n + 1) >> 1;
  const int pad = p.pad2;
  const int64_t nt = n / TL;
  if (w * 64 >= buf.n_streams) {                // wave-uniform
    if constexpr (FUSE) {                       // an idle group still meets the backward pass's barriers
      for (int64_t b = 0; b < (nt > 1 ? (nt - 1 + RT - 1) / RT : 0) + 2; ++b) __syncthreads();
    }
    return;
  }
  const int64_t s = w * 64 + lane;
  const int64_t G = (buf.n_streams + 63) / 64;
  const int64_t wc = w * 2 + comp;
  const int64_t ecap = lp_lane_edge_cap(pad);
  double* __restrict__ ck = buf.s3 + (size_t)wc * nt * 4 * 64 + lane;
  double* __restrict__ eh = buf.s3 + (size_t)2 * G * nt * 4 * 64 + (size_t)wc * ecap * 64 + lane;
  double* __restrict__ et = eh + (size_t)(pad + TL) * 64;
  const double* __restrict__ fl = buf.s2 + (size_t)(w * 2 + (lane >> 5)) * n2 * 64 + (lane & 31) * 2;
  const float* __restrict__ fl32 =
      reinterpret_cast<const float*>(buf.s2 + (size_t)w * 2 * n2 * 64) + (size_t)(lane >> 5) * n2 * 64 + (lane & 31) * 2;
  const double* __restrict__ lov = buf.lo2 + (size_t)comp * n;                   // lo_c[i], vector loads
  CDouble* const loc = (CDouble*)(buf.lo2 + (size_t)comp * n);                   // the same, scalar loads
  CDouble* const lo4 = (CDouble*)(buf.lo) + 2 * comp;                            // (mult, addend) at [4i]
  auto F = [&](int64_t i) -> double {
    if constexpr (F32F) return (double)fl32[(i >> 1) * 64 + (i & 1)];
    else return ld_pol<NTF>(&fl[(i >> 1) * 64 + (i & 1)]);
  };
  auto Xm = [&](int64_t i) { return F(i) * loc[i]; };
  // f pairs of tile t, chunk c: this lane's 16 B (F32F: 8 B) at pair t*TL/2 + c*HC + k
  auto load_chunk = [&](int64_t t, int c, FV (&r)[HC]) {
    if constexpr (F32F) {
      const float2* fp = reinterpret_cast<const float2*>(fl32 + (size_t)(t * (TL / 2) + c * HC) * 64);
#pragma unroll
      for (int k = 0; k < HC; ++k) r[k] = fp[k * 32];
    } else {
      const double* fp = fl + (size_t)(t * (TL / 2) + c * HC) * 64;
#pragma unroll
      for (int k = 0; k < HC; ++k) r[k] = ld_pair<NTF>(fp + k * 64);
    }
  };
  auto load_lo = [&](int64_t t) -> double { return lov[t * TL + (lane < TL ? lane : 0)]; };
  auto put_lo = [&](int64_t t, double v) {
    if (lane < TL) lo_lds[wv][t & 1][lane] = v;
  };
  // mixer inputs of chunk c from the chunk's f pairs and the tile's LDS multipliers
  auto chunk_e = [&](int64_t t, int c, const FV (&fv)[HC], double (&e)[CH]) {
    const double2* lp = reinterpret_cast<const double2*>(&lo_lds[wv][t & 1][c * CH]);
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const double2 l = lp[k];
      e[2 * k] = (double)fv[k].x * l.x;
      e[2 * k + 1] = (double)fv[k].y * l.y;
    }
  };

  // ---- forward pass ---------------------------------------------------------
  double z[4];
  float acc = __builtin_inff();
  bool bad = false;
  const double x0 = F(0) * lo4[0] + lo4[1];      // bb[0]: numpy's (f + 0j) * lo, +0 allowed (class-checked)
  const double xl = Xm(n - 1);
  bad |= __builtin_amdgcn_class(x0, kClsX);
  const double e0 = 2.0 * x0 - Xm(pad);
  bad |= __builtin_amdgcn_class(e0, kClsY);
#pragma unroll
  for (int j = 0; j < 4; ++j) z[j] = f.zi[j] * e0;
  for (int jj = 0; jj < pad; ++jj) {
    const double e = 2.0 * x0 - Xm(pad - jj);
    const double y = lp_step(z, f, e);
    acc = tiny_min3(acc, e, y);
    st_pol<NTC>(&eh[jj * 64], y);
  }
  const int64_t nh = n < TL ? n : TL;           // tile 0 (holds bb[0]): edge buffer, not recomputed
  for (int64_t i = 0; i < nh; ++i) {
    const double e = i == 0 ? x0 : Xm(i);
    const double y = lp_step(z, f, e);
    acc = tiny_min3(acc, i == 0 ? y : e, y);
    st_pol<NTC>(&eh[(pad + i) * 64], y);
  }
  FV ring[R][HC];
  if (nt > 1) {
#pragma unroll
    for (int c = 0; c < R; ++c) load_chunk(1, c, ring[c]);
    put_lo(1, load_lo(1));
  }
  for (int64_t t = 1; t < nt; ++t) {
    const int64_t tn = t + 1 < nt ? t + 1 : t;
    const double lon = load_lo(tn);
#pragma unroll
    for (int j = 0; j < 4; ++j) st_pol<NTC>(&ck[(t * 4 + j) * 64], z[j]);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      FV fv[HC];
#pragma unroll
      for (int k = 0; k < HC; ++k) fv[k] = ring[c % R][k];
      if (c + R < NCH) load_chunk(t, c + R, ring[c % R]);
      else load_chunk(tn, c + R - NCH, ring[c % R]);
      double e[CH];
      chunk_e(t, c, fv, e);
#pragma unroll
      for (int k = 0; k < CH; k += 2) {
        const double y0 = lp_step(z, f, e[k]);
        const double y1 = lp_step(z, f, e[k + 1]);
        acc = tiny_min3(acc, e[k], e[k + 1]);
        acc = tiny_min3(acc, y0, y1);
      }
    }
    put_lo(tn, lon);
  }
  const int64_t i_tail = nt >= 1 ? nt * TL : nh;
  int ne = 0;
  for (int64_t i = i_tail; i < n; ++i) {
    const double e = Xm(i);
    const double y = lp_step(z, f, e);
    acc = tiny_min3(acc, e, y);
    st_pol<NTC>(&et[(ne++) * 64], y);
  }
  double ylast = 0.0;
  for (int jj = 0; jj < pad; ++jj) {
    const double e = 2.0 * xl - Xm(n - 2 - jj);
    ylast = lp_step(z, f, e);
    acc = tiny_min3(acc, e, ylast);
    st_pol<NTC>(&et[(ne++) * 64], ylast);
  }
  bad |= !(acc >= kTinyHi);
#pragma unroll
  for (int j = 0; j < 4; ++j) bad |= !__builtin_isfinite(z[j]);
  lane_pass_fence(dev_fence);                   // checkpoints and edges: re-read below by this wave alone

  // ---- backward pass ----------------------------------------------------------
  const int64_t S = p.n_sym, first = p.first, sps = p.sps;
  double* __restrict__ symp = buf.s1 + sym_index(s, S, 0, comp);   // symbol k at symp[k*64]
  auto put_sym = [&](int64_t k, double y) {
    if constexpr (FUSE) sring[wv][k & (NSL - 1)][lane] = y;
    else symp[k * 64] = y;
  };
  auto sym_out = [&](int64_t i, double y) {     // generic: a symbol sample at i?
    if (i >= first && (i - first) % sps == 0) put_sym((i - first) / sps, y);
  };
  // FUSE: the re wave slices the symbols of samples [i_lo, i_hi) once both
  // components are in the ring (diff_k = s[k+1] * conj(s[k]) in numpy's fma
  // form, exactly as K4a); words complete as k descends through 16j (32j)
  double pr = 0.0, pim = 0.0;                   // s[k+1]
  uint32_t wacc = 0;
  const bool qpsk = p.kind == kQpsk;
  // F32F: this stream's symbol error bound, and whether a decision fell inside it
  const double Em = F32F && s < buf.n_streams ? p.f32_margin * buf.fpeak[s] + 0x1p-120 : 0.0;
  bool mflag = false;
  auto region_done = [&](int64_t i_lo, int64_t i_hi) {
    if constexpr (FUSE) {
      __syncthreads();
      if (comp == 0) {
        const int64_t k_lo = i_lo <= first ? 0 : (i_lo - first + sps - 1) / sps;
        int64_t k_hi = i_hi - 1 < first ? -1 : (i_hi - 1 - first) / sps;
        if (k_hi > S - 1) k_hi = S - 1;
        for (int64_t k = k_hi; k >= k_lo; --k) {
          const double sr = sring[wv][k & (NSL - 1)][lane], si = sring[wv + 1][k & (NSL - 1)][lane];
          if (k <= S - 2) {
            const double br = sr, bi = -si;
            const double dr = __builtin_fma(pr, br, -(pim * bi));
            double md = 0.0;                    // F32F: the decision's margin (d's error bound)
            if constexpr (F32F) {
              const double a0 = fabs(br) + fabs(bi), a1 = fabs(pr) + fabs(pim);
              md = 0x1.6a09e667f3bcdp+0 * Em * (a0 + a1 + Em) * (1.0 + 0x1p-40) + 0x1p-48 * (a0 * a1);
              if (!qpsk && !(fabs(dr) > md)) mflag = true;
            }
            if (qpsk) {
              const double di = __builtin_fma(pr, bi, pim * br);
              if constexpr (F32F) {
                const double adr = fabs(dr), adi = fabs(di);
                if (!(fabs(adi - adr) > md + 0x1p-29 * (adr + adi))) mflag = true;
              }
              wacc |= qpsk_dibit(dr, di) << (30 - 2 * (int)(k & 15));
              if ((k & 15) == 0) {
                if (s < buf.n_streams) st_pol<NTW>(&buf.words[(size_t)s * p.n_words + (k >> 4)], wacc);
                wacc = 0;
              }
            } else {
              wacc |= (dr < 0 ? 1u : 0u) << (31 - (int)(k & 31));
              if ((k & 31) == 0) {
                if (s < buf.n_streams) st_pol<NTW>(&buf.words[(size_t)s * p.n_words + (k >> 5)], wacc);
                wacc = 0;
              }
            }
          }
          pr = sr;
          pim = si;
        }
      }
    }
  };
  float accb = __builtin_inff();
  double zb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) zb[j] = f.zi[j] * ylast;
  for (int e = ne - 1; e >= 0; --e) {
    const double y = lp_step(zb, f, ld_pol<NTC>(&et[e * 64]));
    accb = tiny_min3(accb, y, y);
    const int64_t i = i_tail + e;
    if (i < n) sym_out(i, y);
  }
  region_done(i_tail, n);
  if (nt > 1) {
    const int64_t q0 = SPS > 0 ? first / SPS : 0;
    double cn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cn[j] = ld_pol<NTC>(&ck[((nt - 1) * 4 + j) * 64]);
#pragma unroll
    for (int c = 0; c < R; ++c) load_chunk(nt - 1, c, ring[c]);
    put_lo(nt - 1, load_lo(nt - 1));
    int64_t r_hi = nt * TL;                     // FUSE: upper bound of the region not yet sliced
    for (int64_t t = nt - 1; t >= 1; --t) {
      double zf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) zf[j] = cn[j];
      const int64_t tp = t > 1 ? t - 1 : 1;     // the next (lower) tile's input and checkpoint in flight
#pragma unroll
      for (int j = 0; j < 4; ++j) cn[j] = ld_pol<NTC>(&ck[(tp * 4 + j) * 64]);
      const double lop = load_lo(tp);
      double yt[TL];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        FV fv[HC];
#pragma unroll
        for (int k = 0; k < HC; ++k) fv[k] = ring[c % R][k];
        if (c + R < NCH) load_chunk(t, c + R, ring[c % R]);
        else load_chunk(tp, c + R - NCH, ring[c % R]);
        double e[CH];
        chunk_e(t, c, fv, e);
#pragma unroll
        for (int k = 0; k < CH; ++k) yt[c * CH + k] = lp_step(zf, f, e[k]);
      }
#pragma unroll
      for (int k = TL - 1; k >= 1; k -= 2) {
        const double y1 = lp_step(zb, f, yt[k]);
        const double y0 = lp_step(zb, f, yt[k - 1]);
        accb = tiny_min3(accb, y1, y0);
        if constexpr (SPS > 0) {
          if (k % SPS == FM) put_sym(t * (TL / SPS) + (k - FM) / SPS - q0, y1);
          if ((k - 1) % SPS == FM) put_sym(t * (TL / SPS) + (k - 1 - FM) / SPS - q0, y0);
        } else {
          sym_out(t * TL + k, y1);
          sym_out(t * TL + k - 1, y0);
        }
      }
      put_lo(tp, lop);
      if ((nt - 1 - t) % RT == RT - 1 || t == 1) {
        region_done(t * TL, r_hi);
        r_hi = t * TL;
      }
    }
  }
  for (int e = pad + (int)nh - 1; e >= 0; --e) {
    const double y = lp_step(zb, f, ld_pol<NTC>(&eh[e * 64]));
    accb = tiny_min3(accb, y, y);
    const int64_t i = e - pad;
    if (i >= 0) sym_out(i, y);
  }
  region_done(0, nh);
  bad |= !(accb >= kTinyHi);
#pragma unroll
  for (int j = 0; j < 4; ++j) bad |= !__builtin_isfinite(zb[j]);
  if constexpr (F32F) bad |= mflag;
  if (bad && s < buf.n_streams) {
    atomicOr(&buf.flags[s], 1);
    if constexpr (F32F) atomicOr(&buf.bp_flags[s], 1);   // float64 f for K3x: the fix-up re-runs the group
  }
}

// ---------------------------------------------------------------------------
// low-pass with the fused slicer, both components in ONE wave (AMR_LP_HALF,
// the default wherever the fused slicer runs): a wave holds 32 streams, lanes
// 0-31 their re and lanes 32-63 their im component (lane l and l + 32 are one
// stream).  A group of 64 streams is still two waves -- split by stream half
// (the two 512-B runs of f_index) instead of by component -- and a workgroup
// four waves = two groups, the grid and placement of k_lp_lane.
// Per lane the arithmetic is k_lp_lane's, in its order: the mixer, lp_step,
// the tiny_min3 detector, the class checks, forward pass / re-run / backward
// pass.  What changes is what the waves share:
//   * f: a wave reads only its half's 512-B runs, lanes l and l + 32 the same
//     16 B -- each f pair is fetched once per group and pass, not twice.
//   * the LO multipliers and lo4 are per component, so per lane half: the
//     per-wave LDS double buffer holds both components' tile (lanes < TL load
//     one value of each), read back by ds_read_b128 at a half-dependent
//     address (a broadcast inside each half).
//   * the slicer runs where a symbol sample is produced: one half-wave swap
//     (v_permlane32_swap) hands every lane both components, every lane forms
//     s[k+1] * conj(s[k]), the decision and the MSB-first word exactly as
//     k_lp_lane's region_done, and lanes 0-31 store the words.  No symbol
//     ring, no workgroup barrier, no barrier loop for idle groups: the waves
//     of a workgroup never wait for one another.
//   * s3 holds the same [2G][nt][4][64] checkpoints and [2G][edge][64] edges,
//     indexed by (group, half) instead of (group, component): every store is
//     a whole 512-B row.
// flags are raised per stream (by either component's lane), so K3x and K4a
// redo flagged streams as after k_lp_lane.
// NT: which access classes go non-temporal (psk_common.h: kNtFLoad the f
// loads, kNtCk the checkpoints and edges, kNtWords the word stores).
template <int SPS, int FM, int NT = 0>
__global__ __launch_bounds__(256, AMR_LP_WAVES) void k_lp_lane_h(PskBuffers buf, PskParams p, Iir f, int dev_fence) {
  constexpr bool NTF = (NT & kNtFLoad) != 0, NTC = (NT & kNtCk) != 0, NTW = (NT & kNtWords) != 0;
  constexpr int TL = kLpT;
  constexpr int CH = AMR_LP_CH;
  constexpr int NCH = TL / CH, HC = CH / 2;
  constexpr int R = NCH % 2 == 0 ? NCH / 2 : NCH;
  static_assert(TL % CH == 0 && TL <= 64, "tile = whole chunks; one LO value of each component per lane");
  static_assert(SPS > 0 && TL % SPS == 0 && FM < SPS, "static symbol slots");
  __shared__ __attribute__((aligned(16))) double lo_lds[4][2][2][TL];   // [wave][tile parity][component][sample]
  const int lane = threadIdx.x & 63;
  const int hl = lane & 31, comp = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t w = (int64_t)blockIdx.x * 2 + (wv >> 1);
  const int64_t wc = w * 2 + (wv & 1);          // (group, stream half)
  if (wc * 32 >= buf.n_streams) return;         // wave-uniform: no live stream in this half
  const int64_t n = p.n, n2 = (n + 1) >> 1;
  const int pad = p.pad2;
  const int64_t nt = n / TL;
  const int64_t s = wc * 32 + hl;
  const bool live = s < buf.n_streams;
  const int64_t G = (buf.n_streams + 63) / 64;
  const int64_t ecap = lp_lane_edge_cap(pad);
  // wave-uniform bases (SGPRs) + a small per-lane offset: one VGPR serves every row of a buffer
  double* __restrict__ const ck = buf.s3 + (size_t)wc * nt * 4 * 64;                               // [..][lane]
  double* __restrict__ const eh = buf.s3 + (size_t)2 * G * nt * 4 * 64 + (size_t)wc * ecap * 64;   // [..][lane]
  double* __restrict__ const et = eh + (size_t)(pad + TL) * 64;
  const double* __restrict__ const fl = buf.s2 + (size_t)wc * n2 * 64;                             // [..][hl * 2]
  const unsigned fo = hl * 2;
  const double* __restrict__ lov = buf.lo2 + (size_t)comp * n;                   // lo_c[i] of this lane's component
  const double* __restrict__ lo4 = buf.lo + 2 * comp;                            // (mult, addend) at [4i]
  auto F = [&](int64_t i) -> double { return ld_pol<NTF>(&(fl + ((i >> 1) * 64 + (i & 1)))[fo]); };
  auto Xm = [&](int64_t i) { return F(i) * lov[i]; };
  auto load_chunk = [&](int64_t t, int c, double2 (&r)[HC]) {
    const double* fp = fl + (size_t)(t * (TL / 2) + c * HC) * 64;
#pragma unroll
    for (int k = 0; k < HC; ++k) r[k] = ld_pair<NTF>(&(fp + k * 64)[fo]);
  };
  // the tile's LO multipliers of both components: lanes < TL load one of each a tile ahead
  auto load_lo = [&](int64_t t) -> double2 {
    const double* lb = buf.lo2 + t * TL;
    const unsigned i = lane < TL ? lane : 0;
    return make_double2(lb[i], (lb + n)[i]);
  };
  auto put_lo = [&](int64_t t, double2 v) {
    if (lane < TL) {
      lo_lds[wv][t & 1][0][lane] = v.x;
      lo_lds[wv][t & 1][1][lane] = v.y;
    }
  };
  auto chunk_e = [&](int64_t t, int c, const double2 (&fv)[HC], double (&e)[CH]) {
    const double2* lp = reinterpret_cast<const double2*>(&lo_lds[wv][t & 1][comp][c * CH]);
#pragma unroll
    for (int k = 0; k < HC; ++k) {
      const double2 l = lp[k];
      e[2 * k] = fv[k].x * l.x;
      e[2 * k + 1] = fv[k].y * l.y;
    }
  };

  // ---- forward pass (k_lp_lane's) ---------------------------------------------
  double z[4];
  float acc = __builtin_inff();
  bool bad = false;
  const double x0 = F(0) * lo4[0] + lo4[1];      // bb[0]: numpy's (f + 0j) * lo, +0 allowed (class-checked)
  const double xl = Xm(n - 1);
  bad |= __builtin_amdgcn_class(x0, kClsX);
  const double e0 = 2.0 * x0 - Xm(pad);
  bad |= __builtin_amdgcn_class(e0, kClsY);
#pragma unroll
  for (int j = 0; j < 4; ++j) z[j] = f.zi[j] * e0;
  for (int jj = 0; jj < pad; ++jj) {
    const double e = 2.0 * x0 - Xm(pad - jj);
    const double y = lp_step(z, f, e);
    acc = tiny_min3(acc, e, y);
    st_pol<NTC>(&(eh + jj * 64)[lane], y);
  }
  const int64_t nh = n < TL ? n : TL;           // tile 0 (holds bb[0]): edge buffer, not recomputed
  for (int64_t i = 0; i < nh; ++i) {
    const double e = i == 0 ? x0 : Xm(i);
    const double y = lp_step(z, f, e);
    acc = tiny_min3(acc, i == 0 ? y : e, y);
    st_pol<NTC>(&(eh + (pad + i) * 64)[lane], y);
  }
  double2 ring[R][HC];
  if (nt > 1) {
#pragma unroll
    for (int c = 0; c < R; ++c) load_chunk(1, c, ring[c]);
    put_lo(1, load_lo(1));
  }
  for (int64_t t = 1; t < nt; ++t) {
    const int64_t tn = t + 1 < nt ? t + 1 : t;
    const double2 lon = load_lo(tn);
#pragma unroll
    for (int j = 0; j < 4; ++j) st_pol<NTC>(&(ck + (t * 4 + j) * 64)[lane], z[j]);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      double2 fv[HC];
#pragma unroll
      for (int k = 0; k < HC; ++k) fv[k] = ring[c % R][k];
      if (c + R < NCH) load_chunk(t, c + R, ring[c % R]);
      else load_chunk(tn, c + R - NCH, ring[c % R]);
      double e[CH];
      chunk_e(t, c, fv, e);
#pragma unroll
      for (int k = 0; k < CH; k += 2) {
        const double y0 = lp_step(z, f, e[k]);
        const double y1 = lp_step(z, f, e[k + 1]);
        acc = tiny_min3(acc, e[k], e[k + 1]);
        acc = tiny_min3(acc, y0, y1);
      }
    }
    put_lo(tn, lon);
  }
  const int64_t i_tail = nt >= 1 ? nt * TL : nh;
  int ne = 0;
  for (int64_t i = i_tail; i < n; ++i) {
    const double e = Xm(i);
    const double y = lp_step(z, f, e);
    acc = tiny_min3(acc, e, y);
    st_pol<NTC>(&(et + (ne++) * 64)[lane], y);
  }
  double ylast = 0.0;
  for (int jj = 0; jj < pad; ++jj) {
    const double e = 2.0 * xl - Xm(n - 2 - jj);
    ylast = lp_step(z, f, e);
    acc = tiny_min3(acc, e, ylast);
    st_pol<NTC>(&(et + (ne++) * 64)[lane], ylast);
  }
  bad |= !(acc >= kTinyHi);
#pragma unroll
  for (int j = 0; j < 4; ++j) bad |= !__builtin_isfinite(z[j]);
  lane_pass_fence(dev_fence);                   // checkpoints and edges: re-read below by this wave alone

  // ---- backward pass, slicing as it goes ----------------------------------------
  const int64_t S = p.n_sym, first = p.first, sps = p.sps;
  double pr = 0.0, pim = 0.0;                   // s[k+1]
  uint32_t wacc = 0;
  const bool qpsk = p.kind == kQpsk;
  uint32_t* __restrict__ const wp = buf.words + (size_t)wc * 32 * p.n_words;   // [..][wo]: word j of this lane's stream
  const unsigned wo = (unsigned)hl * (unsigned)p.n_words;
  const bool wr = live && comp == 0;
  // symbol sample k of this lane's component (k wave-uniform, descending from
  // S - 1): both components to every lane, then diff_k = s[k+1] * conj(s[k])
  // in numpy's fma form, exactly as K4a; words complete as k passes 16j (32j)
  auto slice = [&](int64_t k, double y) {
    if (k > S - 1) return;
    const unsigned long long yb = __builtin_bit_cast(unsigned long long, y);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)yb, (unsigned)yb, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)(yb >> 32), (unsigned)(yb >> 32), false, false);
    // [0]: lanes 0-31's value in both halves (re); [1]: lanes 32-63's (im)
    const double sr = __builtin_bit_cast(double, ((unsigned long long)hi[0] << 32) | lo[0]);
    const double si = __builtin_bit_cast(double, ((unsigned long long)hi[1] << 32) | lo[1]);
    if (k <= S - 2) {
      const double br = sr, bi = -si;
      const double dr = __builtin_fma(pr, br, -(pim * bi));
      if (qpsk) {
        const double di = __builtin_fma(pr, bi, pim * br);
        wacc |= qpsk_dibit(dr, di) << (30 - 2 * (int)(k & 15));
        if ((k & 15) == 0) {
          if (wr) st_pol<NTW>(&(wp + (k >> 4))[wo], wacc);
          wacc = 0;
        }
      } else {
        wacc |= (dr < 0 ? 1u : 0u) << (31 - (int)(k & 31));
        if ((k & 31) == 0) {
          if (wr) st_pol<NTW>(&(wp + (k >> 5))[wo], wacc);
          wacc = 0;
        }
      }
    }
    pr = sr;
    pim = si;
  };
  auto sym_out = [&](int64_t i, double y) {     // head / tail edges: a symbol sample at i?
    if (i >= first && (i - first) % sps == 0) slice((i - first) / sps, y);
  };
  float accb = __builtin_inff();
  double zb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) zb[j] = f.zi[j] * ylast;
  for (int e = ne - 1; e >= 0; --e) {
    const double y = lp_step(zb, f, ld_pol<NTC>(&(et + e * 64)[lane]));
    accb = tiny_min3(accb, y, y);
    const int64_t i = i_tail + e;
    if (i < n) sym_out(i, y);
  }
  if (nt > 1) {
    const int64_t q0 = first / SPS;
    double cn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cn[j] = ld_pol<NTC>(&(ck + ((nt - 1) * 4 + j) * 64)[lane]);
#pragma unroll
    for (int c = 0; c < R; ++c) load_chunk(nt - 1, c, ring[c]);
    put_lo(nt - 1, load_lo(nt - 1));
    for (int64_t t = nt - 1; t >= 1; --t) {
      double zf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) zf[j] = cn[j];
      const int64_t tp = t > 1 ? t - 1 : 1;     // the next (lower) tile's input and checkpoint in flight
      double2 lop;
      double yt[TL];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        double2 fv[HC];
#pragma unroll
        for (int k = 0; k < HC; ++k) fv[k] = ring[c % R][k];
        if (c + R < NCH) load_chunk(t, c + R, ring[c % R]);
        else load_chunk(tp, c + R - NCH, ring[c % R]);
        double e[CH];
        chunk_e(t, c, fv, e);
#pragma unroll
        for (int k = 0; k < CH; ++k) yt[c * CH + k] = lp_step(zf, f, e[k]);
      }
      const int64_t kt = t * (TL / SPS) - q0;   // the tile's first symbol
#pragma unroll
      for (int k = TL - 1; k >= 1; k -= 2) {
        const double y1 = lp_step(zb, f, yt[k]);
        const double y0 = lp_step(zb, f, yt[k - 1]);
        accb = tiny_min3(accb, y1, y0);
        // the next tile's LO values and checkpoint: requested once the first outputs are
        // consumed (their registers are free again: 230 VGPRs instead of 238 at sps 5), most
        // of a backward tile before put_lo / the next re-run need them
        if (k == TL - 7) lop = load_lo(tp);
        if (k == TL - 11) {
#pragma unroll
          for (int j = 0; j < 4; ++j) cn[j] = ld_pol<NTC>(&(ck + (tp * 4 + j) * 64)[lane]);
        }
        if (k % SPS == FM) slice(kt + (k - FM) / SPS, y1);
        if ((k - 1) % SPS == FM) slice(kt + (k - 1 - FM) / SPS, y0);
      }
      put_lo(tp, lop);
    }
  }
  for (int e = pad + (int)nh - 1; e >= 0; --e) {
    const double y = lp_step(zb, f, ld_pol<NTC>(&(eh + e * 64)[lane]));
    accb = tiny_min3(accb, y, y);
    const int64_t i = e - pad;
    if (i >= 0) sym_out(i, y);
  }
  bad |= !(accb >= kTinyHi);
#pragma unroll
  for (int j = 0; j < 4; ++j) bad |= !__builtin_isfinite(zb[j]);
  if (bad && live) atomicOr(&buf.flags[s], 1);
}

// ---------------------------------------------------------------------------
// host-side launchers (api.cpp)

// Cache policy of the streamed intermediates (psk_common.h): AMR_LANE_NT=<mask
// of the kNt* classes>, 0 = the default policy everywhere; unset = the
// measured choice (profiles/lane_nt_ab.txt): f stores, f
// loads, checkpoints and edge rows.  Non-temporal x loads cost 36 % of the
// step (a lane's 128-B line is consumed by 8 loads) and non-temporal word
// stores write 11 % more bytes for no time, so both keep the default policy.
// Only the masks compiled in can be asked for (each one is another
// instantiation of every default-path kernel): the default, 0, and every class
// at once for the parity tests; any other value fails the launch.
#ifndef AMR_LANE_NT_DEFAULT
#define AMR_LANE_NT_DEFAULT (kNtFStore | kNtFLoad | kNtCk)
#endif
#ifndef AMR_LANE_NT_MASKS
#define AMR_LANE_NT_MASKS 0, AMR_LANE_NT_DEFAULT, kNtAll
#endif
static int lane_nt() {
  static const int v = (int)env_int("AMR_LANE_NT", INT32_MIN, INT32_MAX, AMR_LANE_NT_DEFAULT);
  return v;
}
template <typename Fn, int... M>
static bool lane_nt_switch(int m, Fn&& fn, std::integer_sequence<int, M...>) {
  return ((m == M ? (fn(std::integral_constant<int, M>{}), true) : false) || ...);
}
// fn(std::integral_constant<int, mask>) for the mask in force; false: that mask is not compiled in
template <typename Fn>
static bool with_lane_nt(Fn&& fn) {
  return lane_nt_switch(lane_nt(), fn, std::integer_sequence<int, AMR_LANE_NT_MASKS>{});
}

static int lane_dev_fence() {
  // AMR_LANE_FENCE=1: the device-scope fence after a forward pass (lane_pass_fence, psk_common.h)
  static const int v = env_on("AMR_LANE_FENCE");
  return v;
}

static int bp_zero_taps(const PskParams& p) {
  // skip the band-pass's +0.0 odd taps (detector + exact re-run of flagged
  // groups): AMR_BP_ZO=0 computes every tap instead.  Which detector vouches
  // for the shortened steps (psk_common.h): the one on y (kZoY), or with
  // AMR_BP_ZDET=0 the earlier watch of four states (kZoZ)
  static const bool on = env_not_off("AMR_BP_ZO");
  static const int det = env_not_off("AMR_BP_ZDET") ? kZoY : kZoZ;
  return on && p.bp_zero_odd && p.bp_sym ? det : 0;
}
// fn(std::integral_constant<int, ZO>) for the band-pass step in force
template <typename Fn>
static void with_bp_zo(int zo, Fn&& fn) {
  if (zo == kZoY) fn(std::integral_constant<int, kZoY>{});
  else if (zo == kZoZ) fn(std::integral_constant<int, kZoZ>{});
  else fn(std::integral_constant<int, 0>{});
}

template <typename T>
static hipError_t launch_bp(const PskBuffers& b, const PskParams& p, const Iir& f, hipStream_t st) {
  const int64_t g = (b.n_streams + 63) / 64;
  const dim3 grid((unsigned)((g + 1) / 2)), block(256);   // two groups per workgroup
  if (b.f32f) {
    // the float32 hand-off; its fix-up launch comes after the low-pass, which
    // flags streams too (launch_psk_bandpass_fixup)
    hipError_t e = hipMemsetAsync(b.bp_flags, 0, (size_t)b.n_streams * 4, st);
    if (e != hipSuccess) return e;
    with_bp_zo(bp_zero_taps(p), [&](auto z) {
      hipLaunchKernelGGL((k_bp_lane2<T, 2, decltype(z)::value, false, true>), grid, block, 0, st, b, p, f,
                         lane_dev_fence());
    });
    return hipGetLastError();
  }
  const int zo = bp_zero_taps(p);
  if (zo) {
    hipError_t e = hipMemsetAsync(b.bp_flags, 0, (size_t)b.n_streams * 4, st);
    if (e != hipSuccess) return e;
  }
  // the cache policies of AMR_LANE_NT; the fix-up launch inherits them
  const bool ok = with_lane_nt([&](auto m) {
    constexpr int NT = decltype(m)::value;
    with_bp_zo(zo, [&](auto z) {
      hipLaunchKernelGGL((k_bp_lane2<T, 2, decltype(z)::value, false, false, NT>), grid, block, 0, st, b, p, f,
                         lane_dev_fence());
    });
    if (zo)   // every tap for the groups holding a flagged stream (the others exit at once)
      hipLaunchKernelGGL((k_bp_lane2<T, 1, 0, true, false, NT>), dim3((unsigned)g), dim3(128), 0, st, b, p, f,
                         lane_dev_fence());
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_psk_bandpass_lane(const PskBuffers& b, const PskParams& p, const Iir& f, hipStream_t st) {
  if (f.nt != 9) return hipErrorInvalidValue;
  switch (b.dtype) {
    case kF32: return launch_bp<float>(b, p, f, st);
    case kF64: return launch_bp<double>(b, p, f, st);
    case kI16: return launch_bp<int16_t>(b, p, f, st);
    default: return hipErrorInvalidValue;
  }
}

// the float32 hand-off's fix-up: every tap, float64 f, for the groups holding
// a stream the band-pass detector or the low-pass margin flagged (bp_flags)
hipError_t launch_psk_bandpass_fixup(const PskBuffers& b, const PskParams& p, const Iir& f, hipStream_t st) {
  if (f.nt != 9) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((b.n_streams + 63) / 64)), block(128);
  switch (b.dtype) {
    case kF32: hipLaunchKernelGGL((k_bp_lane2<float, 1, 0, true>), grid, block, 0, st, b, p, f, lane_dev_fence()); break;
    case kF64: hipLaunchKernelGGL((k_bp_lane2<double, 1, 0, true>), grid, block, 0, st, b, p, f, lane_dev_fence()); break;
    case kI16: hipLaunchKernelGGL((k_bp_lane2<int16_t, 1, 0, true>), grid, block, 0, st, b, p, f, lane_dev_fence()); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

static int lp_half() {
  // the fused low-pass with both components in one wave (k_lp_lane_h) in
  // place of the two-wave fused k_lp_lane: AMR_LP_HALF=1 / 0 forces it on /
  // off; on by default (static symbol slots, float64 f)
  static const int v = env_tri("AMR_LP_HALF") != 0;
  return v;
}

// Whether a batch's low-pass should slice inside its backward pass, given
// static symbol slots: once at least 32768 streams are live.  The fused slicer
// saves the symbols' HBM round trip (+4-5 % per step at 16 x 4096 in flight)
// but lengthens a lone batch's low-pass (11.0 -> 13.7 ms in the two-wave form,
// where the re wave slices between barriers; 12.7 ms in k_lp_lane_h: still
// above 11.0, so the threshold stays), which is what a small live set (a
// 1024-stream shard) waits on.  AMR_FUSED_SLICE=1 / 0 forces it on / off;
// PskBuffers::no_fuse (the soft-output calls) always turns it off.
static bool lp_fuse_wanted(const PskBuffers& b) {
  static const int fuse_env = env_tri("AMR_FUSED_SLICE");
  const int64_t live = b.n_streams * (b.inflight > 1 ? b.inflight : 1);
  return !b.no_fuse && (fuse_env >= 0 ? fuse_env == 1 : live >= 32768);
}

// fn(std::integral_constant<int, SPS>, std::integral_constant<int, FM>) for the
// plan's static symbol slots -- the (sps, first % sps) pairs compiled in, while
// first <= kLpStaticFirstMax (the C ABI allows any first) -- or fn(0, 0): the
// generic kernel.  Returns what fn returns.
template <int V>
using Int = std::integral_constant<int, V>;
template <typename Fn>
static int with_lp_slots(const PskParams& p, Fn&& fn) {
  const int fm = (int)(p.first % (p.sps > 0 ? p.sps : 1));
  if (p.first <= kLpStaticFirstMax) {
    if (p.sps == 10 && fm == 5) return fn(Int<10>{}, Int<5>{});
    if (p.sps == 5 && fm == 2) return fn(Int<5>{}, Int<2>{});
    if (p.sps == 20 && fm == 10) return fn(Int<20>{}, Int<10>{});
    if (p.sps == 10 && fm == 0) return fn(Int<10>{}, Int<0>{});
    if (p.sps == 5 && fm == 0) return fn(Int<5>{}, Int<0>{});
    if (p.sps == 20 && fm == 0) return fn(Int<20>{}, Int<0>{});
  }
  return fn(Int<0>{}, Int<0>{});
}

// which low-pass ran (AMR_LP_* of amr.h), returned by launch_lp; -1: an
// AMR_LANE_NT mask that is not compiled in
template <int S_, int F_>
static int launch_lp(const PskBuffers& b, const PskParams& p, const Iir& f, hipStream_t st) {
  const int64_t g = (b.n_streams + 63) / 64;
  const dim3 grid((unsigned)((g + 1) / 2)), block(256);   // two groups per workgroup
  const bool fuse = S_ > 0 && lp_fuse_wanted(b);
  if (b.f32f) {
    // the float32 hand-off needs the fused slicer (api.cpp asks psk_lane_fused first)
    if (!fuse) return AMR_LP_LANE;
    hipLaunchKernelGGL((k_lp_lane<S_, F_, S_ != 0, S_ != 0>), grid, block, 0, st, b, p, f, lane_dev_fence());
    return AMR_LP_LANE_FUSED;
  }
  if constexpr (S_ != 0) {
    // (k_lp_lane_h offsets a half's words by a 32-bit lane term: 32 * n_words must fit)
    if (fuse && lp_half() && p.n_words < (1 << 26)) {
      const bool ok = with_lane_nt([&](auto m) {
        hipLaunchKernelGGL((k_lp_lane_h<S_, F_, decltype(m)::value>), grid, block, 0, st, b, p, f, lane_dev_fence());
      });
      return ok ? AMR_LP_LANE_HALF : -1;
    }
  }
  // (under 32768 live streams, the soft-output calls, AMR_LP_HALF=0: the same cache policies)
  const bool ok = with_lane_nt([&](auto m) {
    constexpr int NT = decltype(m)::value;
    if (fuse) hipLaunchKernelGGL((k_lp_lane<S_, F_, S_ != 0, false, NT>), grid, block, 0, st, b, p, f, lane_dev_fence());
    else hipLaunchKernelGGL((k_lp_lane<S_, F_, false, false, NT>), grid, block, 0, st, b, p, f, lane_dev_fence());
  });
  if (!ok) return -1;
  return fuse ? AMR_LP_LANE_FUSED : AMR_LP_LANE;
}

// whether launch_psk_lowpass_lane will run the fused slicer for this batch
// (the float32 hand-off's precondition, api.cpp)
bool psk_lane_fused(const PskBuffers& b, const PskParams& p) {
  return with_lp_slots(p, [](auto s, auto) { return (int)decltype(s)::value; }) > 0 && lp_fuse_wanted(b);
}

hipError_t launch_psk_lowpass_lane(const PskBuffers& b, const PskParams& p, const Iir& f, hipStream_t st,
                                   bool* sliced, int* kernel) {
  if (f.nt != 5) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(b.flags, 0, (size_t)b.n_streams * 4, st);
  if (e != hipSuccess) return e;
  const int fused = with_lp_slots(p, [&](auto s, auto m) {
    return launch_lp<decltype(s)::value, decltype(m)::value>(b, p, f, st);
  });
  if (fused < 0) return hipErrorInvalidValue;   // an AMR_LANE_NT mask that is not compiled in
  if (sliced) *sliced = fused != AMR_LP_LANE;
  if (kernel) *kernel = fused;
  return hipGetLastError();
}

}  // namespace amr
