// gol_stamp.hip — K10, the stamp kernel (golhip_stamp_bits).
//
//   gol_stamp_kernel<IL>  merges a rectangle of a pattern (canonical bit
//     words, pww = ceil(pw / 32) a row) into a handle's rows where they lie, in
//     the layout they are stepped in (IL 0 canonical words, 2 interleaved
//     pairs, 4 quads; gol_layout.h).  One launch covers one column segment
//     [dx, dx + sw) of `nr` consecutive local rows; destination column dx + c
//     takes pattern column sx + c.  Cells outside the segment are never
//     changed, and since dx + sw <= W the padding bits of a row's last word
//     stay as they are (zero).
// A lane owns whole encode units of a destination row and nothing else: a
// word (IL 0), a pair (IL 2, one 8-byte load and store) or a quad (IL 4, one
// 16-byte load and store).  Per unit: decode to canonical, merge, encode,
// store.  Canonical word j of a row takes the pattern columns 32 j - dx + sx
// on: a funnel shift of two adjacent pattern words, masked to the segment.
// Consecutive lanes own consecutive units of a row, so a wave's loads and
// stores are contiguous.  The host (golhip_stamp.cpp) splits a pattern that
// crosses the x seam into two segments and launches them one after the other
// on the stream, so a word that both touch is never written by two lanes at
// once; the y seam gives two row intervals.
// The grid is capped at kStampMaxBlocks blocks of 256 lanes (4096 x 256 =
// 1048576 units a lap) with a grid-stride loop behind it; a second lap:
// tests/test_gpu_stamp.py (it restates the cap).  Its own translation unit,
// behind gol_kernels.o on the link line: the step kernels' code object does
// not move.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gol_kernels.h"
#include "gol_layout.h"

namespace golk {

constexpr int kStampMaxBlocks = 4096;

// The 32 pattern bits from column s0 on (s0 may be negative or run past the
// row: words outside [0, pww) read as zero; the caller masks what it keeps).
__device__ __forceinline__ uint32_t stamp_fetch(const uint32_t *__restrict__ prow, int pww, int s0) {
    const int q = s0 >> 5, sh = s0 & 31;  // (arithmetic shift: floor for negative s0)
    const uint32_t lo = (q >= 0 && q < pww) ? prow[q] : 0u;
    if (sh == 0) return lo;
    const uint32_t hi = (q + 1 >= 0 && q + 1 < pww) ? prow[q + 1] : 0u;
    return (lo >> sh) | (hi << (32 - sh));
}

// Canonical word j of a destination row after the stamp.
__device__ __forceinline__ uint32_t stamp_merge(uint32_t c, const uint32_t *__restrict__ prow, int pww, int j,
                                                const StampArgs &a) {
    const int lo = max(a.dx, 32 * j) - 32 * j, hi = min(a.dx + a.sw, 32 * j + 32) - 32 * j;  // bits [lo, hi) of the word
    if (lo >= hi) return c;
    const uint32_t m = (hi - lo == 32) ? ~0u : (((1u << (hi - lo)) - 1u) << lo);
    const uint32_t v = stamp_fetch(prow, pww, 32 * j - a.dx + a.sx) & m;
    switch (a.op) {
        case 0: return (c & ~m) | v;  // GOLHIP_STAMP_COPY
        case 1: return c | v;         // GOLHIP_STAMP_OR
        case 2: return c ^ v;         // GOLHIP_STAMP_XOR
        default: return c & ~v;       // GOLHIP_STAMP_CLEAR
    }
}

template <int IL>
__global__ __launch_bounds__(256) void gol_stamp_kernel(StampArgs a) {
    constexpr int U = IL == 0 ? 1 : IL;  // words an encode unit
    const int u_lo = (a.dx >> 5) / U, u_hi = ((a.dx + a.sw - 1) >> 5) / U;
    const int64_t nu = u_hi - u_lo + 1, total = nu * a.nr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / nu;
        const int u = u_lo + (int)(i - r * nu);
        uint32_t *unit = a.rows + (a.row + r) * a.Ww + (int64_t)u * U;
        const uint32_t *prow = a.pat + r * a.pww;
        if constexpr (IL == 0) {
            *unit = stamp_merge(*unit, prow, a.pww, u, a);
        } else if constexpr (IL == 2) {
            const uint2 w = *reinterpret_cast<const uint2 *>(unit);
            uint32_t c0, c1, e, o;
            il_decode(w.x, w.y, c0, c1);
            c0 = stamp_merge(c0, prow, a.pww, 2 * u, a);
            c1 = stamp_merge(c1, prow, a.pww, 2 * u + 1, a);
            il_encode(c0, c1, e, o);
            *reinterpret_cast<uint2 *>(unit) = make_uint2(e, o);
        } else {
            const uint4 w = *reinterpret_cast<const uint4 *>(unit);
            uint32_t c[4], s[4];
            il4_decode({w.x, w.y, w.z, w.w}, c);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = stamp_merge(c[k], prow, a.pww, 4 * u + k, a);
            il4_encode(c, s);
            *reinterpret_cast<uint4 *>(unit) = make_uint4(s[0], s[1], s[2], s[3]);
        }
    }
}

hipError_t launch_stamp(const StampArgs &a, int il, hipStream_t s) {
    if (a.nr <= 0 || a.sw <= 0) return hipSuccess;
    const int Ww = a.Ww;
    if ((il != 0 && il != 2 && il != 4) || (il && Ww % il) || a.dx < 0 || a.sx < 0 || a.row < 0 || a.pww < 1 ||
        (int64_t)a.dx + a.sw > (int64_t)Ww * 32 || (int64_t)a.sx + a.sw > (int64_t)a.pww * 32 || a.op < 0 || a.op > 3)
        return hipErrorInvalidValue;
    const int U = il == 0 ? 1 : il;
    const int64_t nu = ((a.dx + a.sw - 1) >> 5) / U - (a.dx >> 5) / U + 1, total = nu * a.nr;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, kStampMaxBlocks))), block(256);
    if (il == 0) hipLaunchKernelGGL(gol_stamp_kernel<0>, grid, block, 0, s, a);
    if (il == 2) hipLaunchKernelGGL(gol_stamp_kernel<2>, grid, block, 0, s, a);
    if (il == 4) hipLaunchKernelGGL(gol_stamp_kernel<4>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace golk
