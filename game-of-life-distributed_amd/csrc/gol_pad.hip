// gol_pad.hip — the padded torus: boards whose width is no
// multiple of 32 step on the fast kernels as a slightly wider torus whose extra
// columns are ghost copies of real ones (gol_pad_plan.h).  Three kernels move
// between the canonical board and the wide one, which lives in the layout its
// step kernels run in (IL: 0 canonical, 2 interleaved pairs, 4 quads):
//   gol_pad_kernel    canonical rows -> wide rows, ghosts included
//   gol_seam_kernel   rewrites the ghosts of the wide rows from their real
//                     columns, before every step launch: the hot-path part
//   gol_unpad_kernel  wide rows -> canonical rows, padding bits cleared, with
//                     the popcount of the real columns alone
// All three work on whole chunks of the layout (1, 2 or 4 words = 32, 64 or
// 128 cells) with one vector load or store a chunk.
#include "gol_bits.h"
#include "gol_kernels.h"
#include "gol_layout.h"

#include <algorithm>

namespace golk {

namespace {

template <int IL>
struct Chunk {
    static constexpr int kWords = IL ? IL : 1;
};

// The canonical words of chunk ch of a row in layout IL.
template <int IL>
__device__ __forceinline__ void load_chunk(const uint32_t *row, int ch, uint32_t (&c)[Chunk<IL>::kWords]) {
    if constexpr (IL == 0) {
        c[0] = row[ch];
    } else if constexpr (IL == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(row + 2 * (int64_t)ch);
        il_decode(v.x, v.y, c[0], c[1]);
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + 4 * (int64_t)ch);
        il4_decode({v.x, v.y, v.z, v.w}, c);
    }
}

template <int IL>
__device__ __forceinline__ void store_chunk(uint32_t *row, int ch, const uint32_t (&c)[Chunk<IL>::kWords]) {
    if constexpr (IL == 0) {
        row[ch] = c[0];
    } else if constexpr (IL == 2) {
        uint32_t e, o;
        il_encode(c[0], c[1], e, o);
        *reinterpret_cast<uint2 *>(row + 2 * (int64_t)ch) = make_uint2(e, o);
    } else {
        uint32_t w[4];
        il4_encode(c, w);
        *reinterpret_cast<uint4 *>(row + 4 * (int64_t)ch) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// Blocks of 64 chunks x 4 rows (one wave a row: a wave's loads and stores run
// along the row); a block walks the rows gridDim.y * 4 apart.
constexpr int kPadBlockX = 64, kPadBlockY = 4;

template <int IL>
__global__ __launch_bounds__(kPadBlockX *kPadBlockY) void gol_pad_kernel(PadArgs a) {
    constexpr int C = Chunk<IL>::kWords;
    const int ch = blockIdx.x * kPadBlockX + threadIdx.x;
    if (ch >= a.Wwp / C) return;
    for (int64_t row = (int64_t)blockIdx.y * kPadBlockY + threadIdx.y; row < a.rows;
         row += (int64_t)gridDim.y * kPadBlockY) {
        const uint32_t *src = a.canon + row * a.Ww;
        auto fetch = [&](int i) { return src[i]; };
        uint32_t c[C];
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = pad_wide_word(fetch, a.Ww, ch * C + k, a.plan);
        store_chunk<IL>(a.wide + row * a.Wwp, ch, c);
    }
}

// One thread a row: the chunks from the one that holds column W to the row's
// end, in order.  Every chunk it stores keeps the bits of the real columns as
// they are and every word it composes reads real columns alone, so the
// chunks it has already rewritten (the row's last real columns, the sources
// of the left ghost, share a chunk with the first ghost columns) read the same.
template <int IL>
__global__ __launch_bounds__(64) void gol_seam_kernel(PadArgs a) {
    constexpr int C = Chunk<IL>::kWords;
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.rows) return;
    uint32_t *w = a.wide + row * a.Wwp;
    auto fetch = [&](int i) { return canon_word(w, i, IL); };
    for (int ch = a.plan.W / 32 / C; ch < a.Wwp / C; ++ch) {
        uint32_t c[C];
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = pad_wide_word(fetch, a.Ww, ch * C + k, a.plan);
        store_chunk<IL>(w, ch, c);
    }
}

// The chunks that hold real columns, in the pad kernel's block shape; the
// canonical row's words are stored one by one (its rows are Ww words apart, any
// alignment).  One atomic a block: a count per wave of a large board would
// queue a hundred thousand atomics on one address.
template <int IL>
__global__ __launch_bounds__(kPadBlockX *kPadBlockY) void gol_unpad_kernel(PadArgs a) {
    constexpr int C = Chunk<IL>::kWords;
    __shared__ uint32_t part[kPadBlockY];
    const int ch = blockIdx.x * kPadBlockX + threadIdx.x;
    const uint32_t tail = (1u << (a.plan.W % 32)) - 1u;  // (W % 32 != 0)
    uint32_t cnt = 0;
    if (ch < (a.Ww + C - 1) / C)
        for (int64_t row = (int64_t)blockIdx.y * kPadBlockY + threadIdx.y; row < a.rows;
             row += (int64_t)gridDim.y * kPadBlockY) {
            uint32_t c[C];
            load_chunk<IL>(a.wide + row * a.Wwp, ch, c);
            uint32_t *dst = a.canon + row * a.Ww;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const int j = ch * C + k;
                if (j >= a.Ww) break;
                const uint32_t v = j == a.Ww - 1 ? c[k] & tail : c[k];
                dst[j] = v;
                cnt += __builtin_popcount(v);
            }
        }
    if (!a.alive) return;
    const uint32_t tot = wave_sum_u32(cnt);  // (a wave is one threadIdx.y)
    if (threadIdx.x == 0) part[threadIdx.y] = tot;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < kPadBlockY; ++k) sum += part[k];
        if (sum) atomicAdd(a.alive, (unsigned long long)sum);
    }
}

}  // namespace

static bool pad_args_ok(const PadArgs &a, int il) {
    const int C = il ? il : 1;
    return (il == 0 || il == 2 || il == 4) && a.rows >= 0 && a.plan.Wp % 64 == 0 && a.Wwp == a.plan.Wp / 32 &&
           a.Ww == (a.plan.W + 31) / 32 && a.Wwp % C == 0 && a.plan.W % 32 != 0;
}

// The grid of the pad and unpad kernels over `chunks` chunks a row.
static dim3 pad_grid(int chunks, int rows, int max_blocks) {
    const unsigned gx = (unsigned)((chunks + kPadBlockX - 1) / kPadBlockX);
    const unsigned gy = (unsigned)std::max(1, std::min((rows + kPadBlockY - 1) / kPadBlockY, max_blocks / (int)gx));
    return dim3(gx, gy);
}

hipError_t launch_pad(const PadArgs &a, int il, hipStream_t s) {
    if (!pad_args_ok(a, il) || !a.canon || !a.wide) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    const dim3 grid = pad_grid(a.Wwp / (il ? il : 1), a.rows, 4096), block(kPadBlockX, kPadBlockY);
    if (il == 0) hipLaunchKernelGGL(gol_pad_kernel<0>, grid, block, 0, s, a);
    else if (il == 2) hipLaunchKernelGGL(gol_pad_kernel<2>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(gol_pad_kernel<4>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_seam(const PadArgs &a, int il, hipStream_t s) {
    if (!pad_args_ok(a, il) || !a.wide) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    const dim3 grid((unsigned)((a.rows + 63) / 64)), block(64);
    if (il == 0) hipLaunchKernelGGL(gol_seam_kernel<0>, grid, block, 0, s, a);
    else if (il == 2) hipLaunchKernelGGL(gol_seam_kernel<2>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(gol_seam_kernel<4>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_unpad(const PadArgs &a, int il, hipStream_t s) {
    if (!pad_args_ok(a, il) || !a.canon || !a.wide) return hipErrorInvalidValue;
    if (a.rows == 0) return hipSuccess;
    const int C = il ? il : 1;
    const dim3 grid = pad_grid((a.Ww + C - 1) / C, a.rows, 1024), block(kPadBlockX, kPadBlockY);
    if (il == 0) hipLaunchKernelGGL(gol_unpad_kernel<0>, grid, block, 0, s, a);
    else if (il == 2) hipLaunchKernelGGL(gol_unpad_kernel<2>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(gol_unpad_kernel<4>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace golk
