// gol_ckpt.hip — K8, the checkpoint kernels (golhip_checkpoint_begin,
// golhip_checkpoint_load).
//
//   gol_ckpt_kernel<IL>       reads a handle's rows where they lie, in the
//     layout they are stepped in (IL 0 canonical words, 2 interleaved pairs,
//     4 quads; gol_layout.h), writes nothing to them, and stores the canonical
//     words to a shadow buffer.  In the same pass it sums the alive count and
//     the digest of golhip_board_hash, sum of splitmix64((global word index
//     << 32) | word), one 64-bit atomic a wave for each, as K2 does.
//   gol_ckpt_load_kernel<IL>  the inverse: canonical words from a staging
//     buffer into the handle's rows in layout IL, the bits of columns >= width
//     cleared, with the count and digest of what it stored.
// A lane owns 16 bytes: one 16-byte load and one 16-byte store per four words;
// the at most three words behind the last whole group go one at a time.  Both
// buffers are 16-byte aligned (the callers pass whole strips).  Every tail,
// the padding mask at each lane position, a second block and a second lap of
// the grid: tests/test_gpu_ckpt_edges.py (it restates ckpt_blocks()).  Its own
// translation unit, behind gol_kernels.o on the link line: the step kernels'
// code object does not move.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gol_bits.h"
#include "gol_kernels.h"
#include "gol_layout.h"

namespace golk {

// canonical words of the four stored words w (a group never straddles a pair or a quad)
template <int IL>
__device__ __forceinline__ void ckpt_decode(const uint32_t (&w)[4], uint32_t (&c)[4]) {
    if constexpr (IL == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = w[k];
    } else if constexpr (IL == 2) {
        il_decode(w[0], w[1], c[0], c[1]);
        il_decode(w[2], w[3], c[2], c[3]);
    } else {
        il4_decode(w, c);
    }
}
template <int IL>
__device__ __forceinline__ void ckpt_encode(const uint32_t (&c)[4], uint32_t (&w)[4]) {
    if constexpr (IL == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = c[k];
    } else if constexpr (IL == 2) {
        il_encode(c[0], c[1], w[0], w[1]);
        il_encode(c[2], c[3], w[2], w[3]);
    } else {
        il4_encode(c, w);
    }
}

__device__ __forceinline__ void ckpt_add(uint32_t word, int64_t gidx, unsigned long long &cnt, unsigned long long &dig) {
    cnt += (unsigned)__builtin_popcount(word);
    dig += splitmix64(((uint64_t)gidx << 32) | (uint64_t)word);
}

__device__ __forceinline__ void ckpt_reduce(unsigned long long cnt, unsigned long long dig, unsigned long long *sums) {
    cnt = wave_sum_u64(cnt);
    dig = wave_sum_u64(dig);
    if ((threadIdx.x & 63) == 0) {
        if (cnt) atomicAdd(&sums[0], cnt);
        atomicAdd(&sums[1], dig);
    }
}

template <int IL>
__global__ __launch_bounds__(256) void gol_ckpt_kernel(const uint32_t *__restrict__ rows, uint32_t *__restrict__ shadow,
                                                        int64_t nwords, int64_t word0, unsigned long long *sums) {
    const int64_t ng = nwords >> 2;
    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long cnt = 0, dig = 0;
    for (int64_t g = gt; g < ng; g += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(rows)[g];
        uint32_t c[4];
        ckpt_decode<IL>({v.x, v.y, v.z, v.w}, c);
        reinterpret_cast<uint4 *>(shadow)[g] = make_uint4(c[0], c[1], c[2], c[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) ckpt_add(c[k], word0 + 4 * g + k, cnt, dig);
    }
    if (gt == 0) {  // nwords % 4 words: canonical singles, or one pair
        const int64_t i = ng << 2;
        if (IL == 2 && nwords - i == 2) {
            uint32_t a, b;
            il_decode(rows[i], rows[i + 1], a, b);
            shadow[i] = a;
            shadow[i + 1] = b;
            ckpt_add(a, word0 + i, cnt, dig);
            ckpt_add(b, word0 + i + 1, cnt, dig);
        } else if (IL == 0) {
            for (int64_t j = i; j < nwords; ++j) {
                shadow[j] = rows[j];
                ckpt_add(rows[j], word0 + j, cnt, dig);
            }
        }
    }
    ckpt_reduce(cnt, dig, sums);
}

// keep: mask of the last word of a row (all ones where width % 32 == 0; then Ww is not looked at)
template <int IL>
__global__ __launch_bounds__(256) void gol_ckpt_load_kernel(const uint32_t *__restrict__ stage, uint32_t *__restrict__ rows,
                                                             int64_t nwords, int64_t word0, int Ww, uint32_t keep,
                                                             unsigned long long *sums) {
    const int64_t ng = nwords >> 2;
    const int64_t gt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long cnt = 0, dig = 0;
    for (int64_t g = gt; g < ng; g += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(stage)[g];
        uint32_t c[4] = {v.x, v.y, v.z, v.w}, w[4];
        if (IL == 0 && keep != ~0u) {
            int col = (int)((4 * g) % Ww);  // one division a group; the column then walks (Ww may be below 4)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (col == Ww - 1) c[k] &= keep;
                if (++col == Ww) col = 0;
            }
        }
        ckpt_encode<IL>(c, w);
        reinterpret_cast<uint4 *>(rows)[g] = make_uint4(w[0], w[1], w[2], w[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) ckpt_add(c[k], word0 + 4 * g + k, cnt, dig);
    }
    if (gt == 0) {
        const int64_t i = ng << 2;
        if (IL == 2 && nwords - i == 2) {
            il_encode(stage[i], stage[i + 1], rows[i], rows[i + 1]);
            ckpt_add(stage[i], word0 + i, cnt, dig);
            ckpt_add(stage[i + 1], word0 + i + 1, cnt, dig);
        } else if (IL == 0) {
            for (int64_t j = i; j < nwords; ++j) {
                const uint32_t c = (j % Ww == Ww - 1) ? stage[j] & keep : stage[j];
                rows[j] = c;
                ckpt_add(c, word0 + j, cnt, dig);
            }
        }
    }
    ckpt_reduce(cnt, dig, sums);
}

static unsigned ckpt_blocks(int64_t nwords) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(((nwords >> 2) + 255) / 256, 4096));
}

hipError_t launch_ckpt(const uint32_t *rows, uint32_t *shadow, int64_t nwords, int64_t word0, int il,
                       unsigned long long *sums, hipStream_t s) {
    if (nwords <= 0) return hipSuccess;
    if ((il != 0 && il != 2 && il != 4) || (il == 2 && nwords % 2) || (il == 4 && nwords % 4)) return hipErrorInvalidValue;
    const dim3 grid(ckpt_blocks(nwords)), block(256);
    if (il == 0) hipLaunchKernelGGL(gol_ckpt_kernel<0>, grid, block, 0, s, rows, shadow, nwords, word0, sums);
    if (il == 2) hipLaunchKernelGGL(gol_ckpt_kernel<2>, grid, block, 0, s, rows, shadow, nwords, word0, sums);
    if (il == 4) hipLaunchKernelGGL(gol_ckpt_kernel<4>, grid, block, 0, s, rows, shadow, nwords, word0, sums);
    return hipGetLastError();
}

hipError_t launch_ckpt_load(const uint32_t *stage, uint32_t *rows, int64_t nwords, int64_t word0, int W, int Ww, int il,
                            unsigned long long *sums, hipStream_t s) {
    if (nwords <= 0) return hipSuccess;
    if ((il != 0 && il != 2 && il != 4) || (il == 2 && nwords % 2) || (il == 4 && nwords % 4) || (il != 0 && W % 32))
        return hipErrorInvalidValue;
    const uint32_t keep = W % 32 ? (1u << (W % 32)) - 1u : ~0u;
    const dim3 grid(ckpt_blocks(nwords)), block(256);
    if (il == 0) hipLaunchKernelGGL(gol_ckpt_load_kernel<0>, grid, block, 0, s, stage, rows, nwords, word0, Ww, keep, sums);
    if (il == 2) hipLaunchKernelGGL(gol_ckpt_load_kernel<2>, grid, block, 0, s, stage, rows, nwords, word0, Ww, keep, sums);
    if (il == 4) hipLaunchKernelGGL(gol_ckpt_load_kernel<4>, grid, block, 0, s, stage, rows, nwords, word0, Ww, keep, sums);
    return hipGetLastError();
}

}  // namespace golk
