// gol_flip_seam.h — the row seam of the fused turn + list kernel (K5, K5r) on
// boards whose width is no multiple of 32.  A row of W
// columns is Ww = ceil(W / 32) words; the last word holds r = W % 32 real
// columns and 32 - r padding bits, zero on input.  One turn needs the torus
// closed across that word only:
//   * the row's last word x becomes x | (word 0 << r): bit r is a ghost of
//     column 0, so column W - 1 sees its east neighbour;
//   * the word left of the row's first word becomes (last word) << (32 - r):
//     its bit 31 is column W - 1, the west neighbour of column 0;
//   * after the rule, bits >= r of the last word's result are cleared, so
//     padding stays zero and no cell with x >= W is counted or listed.
// Ww == 1: both apply to the same word.  Plain word operations, no HIP call:
// the kernel and the CPU test (tests/test_flip_seam_cpu.py, compiled alone
// under the sanitizers) share them.  r is in 1..31 everywhere.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define GOL_SEAM_FN __host__ __device__ __forceinline__
#else
#define GOL_SEAM_FN inline
#endif

namespace golk {

// The row's last word with column 0 (bit 0 of `first`, the row's word 0) as a ghost at bit r.
GOL_SEAM_FN uint32_t seam_last_word(uint32_t x, uint32_t first, unsigned r) { return x | (first << r); }

// The word left of the row's first word, from the row's last word: column W - 1 at bit 31.
GOL_SEAM_FN uint32_t seam_left_word(uint32_t last, unsigned r) { return last << (32u - r); }

// The last word's result without its padding bits.
GOL_SEAM_FN uint32_t seam_clear_pad(uint32_t nx, unsigned r) { return nx & ((1u << r) - 1u); }

}  // namespace golk
