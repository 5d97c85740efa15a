// hell.h -- shared between hell_kernels.hip and hell_api.cpp (Hellschreiber receiver).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amr {

constexpr int64_t kHellBlock = 8192;   // numpy's reduction buffer: the pairwise sum restarts every 8192 elements
constexpr int kHellThreads = 256;      // 4 wavefronts, one 7-pixel group each
constexpr int kHellStack = 16;         // merge stack: a block's tree is at most 8 deep (8192 / 64 leaves)

// one leaf (<= 128 elements) of a pixel's summation tree, in post-order
struct HellLeaf {
  int32_t off;         // first element, from the pixel's start (a multiple of 8 from its block's start)
  int32_t len;         // 1..128; only a block's last leaf has len % 8 != 0
  int32_t merges;      // left + right combines to do once this leaf's sum is on the stack
  int32_t block_end;   // 1: the stack now holds the block's sum -> acc = acc + it
};

// every leaf a split makes has >= 64 elements, so a block of L has at most max(1, L / 64) leaves
inline int64_t hell_leaf_cap(int64_t sps) { return sps / 64 + (sps + kHellBlock - 1) / kHellBlock + 1; }
inline int64_t hell_work_bytes(int64_t sps) { return hell_leaf_cap(sps) * (int64_t)sizeof(HellLeaf) + 16 + 128; }

hipError_t launch_hell(int elem, const void* x, int64_t x_stride, int64_t n_streams, int64_t n_samples, int64_t sps,
                       uint8_t* out, int64_t out_stride, int64_t* out_len, double* energy, void* work,
                       hipStream_t st);

}  // namespace amr
