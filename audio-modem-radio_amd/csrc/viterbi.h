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

hipError_t launch_viterbi(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                          int64_t out_stride, int64_t* out_len, int32_t* metric, void* work, hipStream_t st);
// out[i][0 .. 2 in_len[i] + 2) = the codeword of in[i][0 .. in_len[i]); n * l_max threads
hipError_t launch_conv_encode(const uint8_t* in, int64_t in_stride, const int64_t* in_len, int64_t n, uint8_t* out,
                              int64_t out_stride, int64_t l_max, hipStream_t st);

}  // namespace amr
