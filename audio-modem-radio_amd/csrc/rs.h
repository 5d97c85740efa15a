// rs.h -- shared between rs_kernels.hip and rs_api.cpp: the Reed-Solomon code of
// fec.ReedSolomonCodec over GF(2^8) (polynomial 0x11D, alpha = 2, generator roots
// alpha^0 .. alpha^(nsym-1)), its block geometry and its interleave, DESIGN §3h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amr {

constexpr int kRsThreads = 256;                          // 4 wavefronts, one block (codeword) each
constexpr int kRsN = 255;                                // the full codeword, bytes
constexpr int kRsMinSym = 2, kRsMaxSym = 64;             // parity bytes per block: one per lane at most
constexpr int kRsMaxInterleave = 64;
constexpr int kRsPoly = 0x11D;

// ---- lengths -----------------------------------------------------------------
// a message of n bytes is ceil(n / k) blocks of k = 255 - nsym bytes (the last 1 .. k), each followed by nsym parity bytes
__host__ __device__ inline int64_t rs_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ inline int64_t rs_encoded_len(int64_t n, int nsym) { return n + rs_ceil_div(n, kRsN - nsym) * nsym; }
// a received length is valid when it is 0 or its last block holds at least one message byte
__host__ __device__ inline bool rs_valid_len(int64_t L, int nsym) {
  if (L <= 0) return L == 0;
  return L - kRsN * (rs_ceil_div(L, kRsN) - 1) >= nsym + 1;
}
__host__ __device__ inline int64_t rs_decoded_len(int64_t L, int nsym) { return L - rs_ceil_div(L, kRsN) * nsym; }
// the longest valid received length a row of in_stride bytes can hold (0: none but the empty one)
inline int64_t rs_max_len(int64_t in_stride, int nsym) {
  if (in_stride <= 0) return 0;
  const int64_t nb = rs_ceil_div(in_stride, kRsN);
  return in_stride - kRsN * (nb - 1) >= nsym + 1 ? in_stride : kRsN * (nb - 1);
}

// ---- interleave ----------------------------------------------------------------
// Stream position of byte c of block B.  Consecutive blocks form groups of I (the last group has Ig <= I);
// a group is emitted column by column, skipping the columns a short block lacks.  Only the stream's very
// last block can be short (last_len bytes; every other block has 255), so with gl the length of the
// group's last block the columns below gl hold Ig bytes each and the columns from gl on hold Ig - 1.
__host__ __device__ inline int64_t rs_stream_pos(int64_t B, int c, int I, int64_t nblk, int last_len) {
  const int64_t g0 = B / I * I;                          // the group's first block
  const int b = (int)(B - g0);
  const int Ig = nblk - g0 < I ? (int)(nblk - g0) : I;
  const int gl = g0 + Ig == nblk ? last_len : kRsN;
  return g0 * kRsN + (c < gl ? c * Ig + b : gl * Ig + (c - gl) * (Ig - 1) + b);
}

// ---- the field, on the host: what the generator needs ----------------------------
inline int rs_host_mul(int a, int b) {
  int r = 0;
  for (int i = 0; i < 8; ++i) {
    if ((b >> i) & 1) r ^= a;
    a = (a << 1) ^ ((a & 0x80) ? kRsPoly : 0);
  }
  return r;
}

// g(x) = prod_{i < nsym} (x - alpha^i) = x^nsym + sum_j g[j] x^(nsym - 1 - j); g[j] = 0 for j >= nsym
struct RsGen {
  uint8_t g[kRsMaxSym];
};
inline RsGen rs_generator(int nsym) {
  int p[kRsMaxSym + 1] = {1};                            // highest power first
  int root = 1;
  for (int d = 0; d < nsym; ++d) {                       // p *= (x + root)
    p[d + 1] = 0;
    for (int j = d + 1; j >= 1; --j) p[j] ^= rs_host_mul(p[j - 1], root);
    root = rs_host_mul(root, 2);
  }
  RsGen gen{};
  for (int j = 0; j < nsym; ++j) gen.g[j] = (uint8_t)p[j + 1];
  return gen;
}

// ---- launches (rs_kernels.hip) ----------------------------------------------------
// One wavefront per block; the grid covers n rows of ceil(in_stride / k) (encode) or ceil(in_stride / 255)
// (decode) blocks.  Lengths are read on the device and checked against the strides there.
// encode: out_len[i] = the encoded length, or -1 for a length outside [0, in_stride] or an output row too short
hipError_t launch_rs_encode(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, int nsym,
                            int interleave, uint8_t* out, int64_t out_stride, int64_t* out_len, hipStream_t st);
// decode: erase is null or [n][in_stride], nonzero = erased; corrected / failed are zeroed on the stream first
hipError_t launch_rs_decode(const uint8_t* in, int64_t in_stride, const int64_t* in_len, const uint8_t* erase,
                            int64_t n, int nsym, int interleave, uint8_t* out, int64_t out_stride, int64_t* out_len,
                            int32_t* corrected, int32_t* failed, hipStream_t st);

}  // namespace amr
