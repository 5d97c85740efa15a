// viterbi.h -- shared between viterbi_kernels.hip and viterbi_api.cpp: the rate-1/2, K=7
// convolutional code of fec.py:72-111 (polynomials 171/133 octal), DESIGN §3f.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace amr {

constexpr int kVitThreads = 256;                         // 4 wavefronts, one codeword each
constexpr int kVitG1 = 0x79, kVitG2 = 0x5B;              // 171, 133 octal
constexpr int64_t kVitMaxLen = (int64_t)1 << 24;         // longest codeword, bytes: int32 path metrics stay < 2^28
constexpr int32_t kVitInf = 1 << 29;                     // start metric of states != 0: cannot win, cannot overflow
constexpr int64_t kVitWorkBudget = (int64_t)4 << 30;     // the host entry's survivor workspace per chunk, bytes

// a message of n bytes is 8n + 6 steps, 16n + 12 coded bits, L = 2n + 2 bytes
inline bool vit_is_codeword_len(int64_t L) { return L >= 2 && L <= kVitMaxLen && (L & 1) == 0; }
inline int64_t vit_msg_len(int64_t L) { return (L - 2) / 2; }
inline int64_t vit_steps(int64_t L) { return 4 * L - 2; }
inline int64_t vit_blocks(int64_t L) { return (vit_steps(L) + 63) / 64; }   // 64-step survivor blocks of 512 bytes
// the longest codeword a row of in_stride bytes can hold (0: none)
inline int64_t vit_max_len(int64_t in_stride) {
  const int64_t L = (in_stride < kVitMaxLen ? in_stride : kVitMaxLen) & ~(int64_t)1;
  return L >= 2 ? L : 0;
}
// survivor words (uint64) one codeword's slice of the workspace holds
inline int64_t vit_work_words(int64_t in_stride) {
  const int64_t L = vit_max_len(in_stride);
  return L ? vit_blocks(L) * 64 : 0;
}

// ---- soft input (k_viterbi_soft): int8 values, > 0 bit 1, < 0 bit 0, |v| the reliability,
// 0 an erasure, -128 read as -127.  A row of n_vals values is the bit stream (n_vals % 16 == 12: two
// values per step) or the byte-aligned image of a codeword of n_vals / 8 bytes (n_vals % 16 == 0: the
// last byte's high nibble, four values, skipped as V1 ignores it)
constexpr int64_t kVitSoftMaxVals = ((int64_t)1 << 21) - 4;   // longest soft row, values
static_assert(254 * (kVitSoftMaxVals / 2) < ((int64_t)1 << 28) && kVitSoftMaxVals % 16 == 12,
              "a step adds at most 127 + 127: int32 path metrics stay < 2^28, under kVitInf with room to add");
static_assert((int64_t)kVitInf + ((int64_t)1 << 28) + 254 < INT32_MAX, "kVitInf plus a full path metric cannot overflow");
// trellis steps of a soft row, 0 when n_vals is not a soft row length
__host__ __device__ inline int64_t vit_soft_steps(int64_t n_vals) {
  if (n_vals < 12 || n_vals > kVitSoftMaxVals) return 0;
  if ((n_vals & 15) == 12) return n_vals / 2;
  return (n_vals & 15) == 0 ? n_vals / 2 - 2 : 0;
}
// the most steps a row of in_stride values can hold (0: none), and its survivor words
inline int64_t vit_soft_max_steps(int64_t in_stride) {
  const int64_t s = in_stride < kVitSoftMaxVals ? in_stride : kVitSoftMaxVals;
  return s >= 12 ? (((s - 12) & ~(int64_t)15) + 12) / 2 : 0;   // the byte image of 4 more values has the same steps
}
inline int64_t vit_soft_work_words(int64_t in_stride) { return (vit_soft_max_steps(in_stride) + 63) / 64 * 64; }

hipError_t launch_viterbi_soft(const int8_t* in, int64_t in_stride, int64_t in_offset, const int64_t* in_len, int64_t n,
                               uint8_t* out, int64_t out_stride, int64_t* out_len, int32_t* metric, void* work,
                               hipStream_t st);
hipError_t launch_viterbi(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                          int64_t out_stride, int64_t* out_len, int32_t* metric, void* work, hipStream_t st);
// out[i][0 .. 2 in_len[i] + 2) = the codeword of in[i][0 .. in_len[i]); n * l_max threads
hipError_t launch_conv_encode(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                              int64_t out_stride, int64_t l_max, hipStream_t st);

}  // namespace amr
