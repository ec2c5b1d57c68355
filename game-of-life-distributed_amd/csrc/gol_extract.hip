// gol_extract.hip — K12 and K13, the read half of the pattern calls
// (golhip_extract_bits, golhip_alive_box).  Neither kernel
// writes the board.
//
//   gol_extract_kernel<IL>  the mirror of K10: delivers columns [sx, sx + sw) of
//     `nr` consecutive local rows of a handle, read in the layout they are
//     stepped in (IL 0 canonical words, 2 interleaved pairs, 4 quads;
//     gol_layout.h), to columns [ox, ox + sw) of a zeroed scratch of pww
//     canonical words a row.  A lane owns one output word of one output row: it
//     loads the one or two encode units that hold the two source words the
//     word's 32 columns come from, decodes them, funnel-shifts, masks to the
//     segment and ORs the result into the scratch word.  Bits outside the
//     segment are never set, so the scratch's padding bits stay zero for every
//     width (W % 32 != 0 included: the seam then lies inside a source word, and
//     the mask, not the source's padding, bounds what is taken).  The host
//     (golhip_extract.cpp) splits a rectangle that crosses the x seam into two
//     segments and launches them one after the other on the stream, so an
//     output word that both touch is never written by two lanes at once; the y
//     seam gives two row intervals.
//   gol_occupancy_kernel<IL>  reads a handle's own rows once (no halo row) and
//     ORs into two zeroed bitmaps: col_or[Ww] canonical words (bit x: some row
//     has cell x alive) and row_or[ceil(rows / 32)] (bit r: local row r has an
//     alive cell).  A block task is 256 consecutive encode units of a chunk of
//     kOccRows = 32 rows, which is one word of row_or: consecutive lanes own
//     consecutive units, so a wave's loads are contiguous.  A lane ORs its unit
//     over the chunk in registers, decodes once and issues one atomicOr a
//     non-zero canonical word; a row's bit comes from a wave ballot, gathered
//     over the chunk in a register, and lane 0 of the wave issues the one
//     atomicOr.  It relies on the board's padding bits being zero, as K2 does.
// Both grids are capped (kExtractMaxBlocks, kOccMaxBlocks blocks of 256 lanes)
// with a grid-stride loop behind them; a second lap of K12:
// tests/test_gpu_extract.py (it restates the cap).  Their own translation
// unit, behind gol_kernels.o on the link line: the step kernels' code object
// does not move.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gol_kernels.h"
#include "gol_layout.h"

namespace golk {

constexpr int kExtractMaxBlocks = 4096;
constexpr int kOccMaxBlocks = 8192;
constexpr int kOccRows = 32;  // rows a chunk: one word of row_or

// Canonical words q and q + 1 of a source row stored in layout IL (words
// outside [0, Ww) read as zero): one encode unit, or two where q + 1 opens the
// next.
template <int IL>
__device__ __forceinline__ void extract_words(const uint32_t *__restrict__ srow, int Ww, int q, uint32_t &lo, uint32_t &hi) {
    if constexpr (IL == 0) {
        lo = (q >= 0 && q < Ww) ? srow[q] : 0u;
        hi = (q + 1 >= 0 && q + 1 < Ww) ? srow[q + 1] : 0u;
    } else {
        constexpr int U = IL;
        const int nu = Ww / U;
        const int u0 = q >> (U == 2 ? 1 : 2), u1 = (q + 1) >> (U == 2 ? 1 : 2);  // (arithmetic shift: floor for q = -1)
        uint32_t c0[U] = {}, c1[U] = {};
        auto unit = [&](int u, uint32_t (&c)[U]) {
            if (u < 0 || u >= nu) return;
            if constexpr (IL == 2) {
                const uint2 w = *reinterpret_cast<const uint2 *>(srow + 2 * (int64_t)u);
                il_decode(w.x, w.y, c[0], c[1]);
            } else {
                const uint4 w = *reinterpret_cast<const uint4 *>(srow + 4 * (int64_t)u);
                il4_decode({w.x, w.y, w.z, w.w}, c);
            }
        };
        unit(u0, c0);
        lo = c0[q & (U - 1)];
        if (u1 == u0) {
            hi = c0[(q + 1) & (U - 1)];
        } else {
            unit(u1, c1);
            hi = c1[0];
        }
    }
}

template <int IL>
__global__ __launch_bounds__(256) void gol_extract_kernel(ExtractArgs a) {
    const int j_lo = a.ox >> 5, j_hi = (a.ox + a.sw - 1) >> 5;
    const int64_t nj = j_hi - j_lo + 1, total = nj * a.nr;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / nj;
        const int j = j_lo + (int)(i - r * nj);
        // bits [lo, hi) of output word j belong to the segment
        const int lo = max(a.ox, 32 * j) - 32 * j, hi = min(a.ox + a.sw, 32 * j + 32) - 32 * j;
        if (lo >= hi) continue;
        const uint32_t m = (hi - lo == 32) ? ~0u : (((1u << (hi - lo)) - 1u) << lo);
        // output column 32 j takes source column s0 (negative: the bits below `lo`, masked away)
        const int s0 = 32 * j - a.ox + a.sx;
        const int q = s0 >> 5, sh = s0 & 31;
        uint32_t w0, w1;
        extract_words<IL>(a.rows + (a.row + r) * a.Ww, a.Ww, q, w0, w1);
        const uint32_t v = sh ? ((w0 >> sh) | (w1 << (32 - sh))) : w0;
        uint32_t *o = a.out + r * a.pww + j;
        *o |= v & m;
    }
}

hipError_t launch_extract(const ExtractArgs &a, int il, hipStream_t s) {
    if (a.nr <= 0 || a.sw <= 0) return hipSuccess;
    const int Ww = a.Ww;
    if ((il != 0 && il != 2 && il != 4) || (il && Ww % il) || a.ox < 0 || a.sx < 0 || a.row < 0 || a.pww < 1 ||
        (int64_t)a.sx + a.sw > (int64_t)Ww * 32 || (int64_t)a.ox + a.sw > (int64_t)a.pww * 32)
        return hipErrorInvalidValue;
    const int64_t nj = ((a.ox + a.sw - 1) >> 5) - (a.ox >> 5) + 1, total = nj * a.nr;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, kExtractMaxBlocks))), block(256);
    if (il == 0) hipLaunchKernelGGL(gol_extract_kernel<0>, grid, block, 0, s, a);
    if (il == 2) hipLaunchKernelGGL(gol_extract_kernel<2>, grid, block, 0, s, a);
    if (il == 4) hipLaunchKernelGGL(gol_extract_kernel<4>, grid, block, 0, s, a);
    return hipGetLastError();
}

template <int IL>
__global__ __launch_bounds__(256) void gol_occupancy_kernel(const uint32_t *__restrict__ rows, int64_t nrows, int Ww,
                                                            uint32_t *__restrict__ col_or, uint32_t *__restrict__ row_or) {
    constexpr int U = IL == 0 ? 1 : IL;
    const int nu = Ww / U;              // encode units a row
    const int64_t nbx = (nu + 255) / 256;  // block tasks a chunk
    const int64_t nchunks = (nrows + kOccRows - 1) / kOccRows, tasks = nbx * nchunks;
    for (int64_t t = blockIdx.x; t < tasks; t += gridDim.x) {  // (block-uniform: every lane of a wave reaches the ballots)
        const int64_t chunk = t / nbx;
        const int u = (int)(t - chunk * nbx) * 256 + (int)threadIdx.x;
        const int64_t r0 = chunk * kOccRows;
        const int nr = (int)min((int64_t)kOccRows, nrows - r0);
        const uint32_t *p = rows + r0 * Ww + (int64_t)u * U;
        uint32_t acc[U] = {};
        uint32_t rbits = 0;
        for (int k = 0; k < nr; ++k, p += Ww) {
            uint32_t any = 0;
            if (u < nu) {
                if constexpr (IL == 0) {
                    any = *p;
                    acc[0] |= any;
                } else if constexpr (IL == 2) {
                    const uint2 w = *reinterpret_cast<const uint2 *>(p);
                    acc[0] |= w.x;
                    acc[1] |= w.y;
                    any = w.x | w.y;
                } else {
                    const uint4 w = *reinterpret_cast<const uint4 *>(p);
                    acc[0] |= w.x;
                    acc[1] |= w.y;
                    acc[2] |= w.z;
                    acc[3] |= w.w;
                    any = (w.x | w.y) | (w.z | w.w);
                }
            }
            if (__ballot(any != 0)) rbits |= 1u << k;
        }
        if (rbits && (threadIdx.x & 63) == 0) atomicOr(row_or + chunk, rbits);
        if (u < nu) {
            uint32_t c[U];
            if constexpr (IL == 0) c[0] = acc[0];
            else if constexpr (IL == 2) il_decode(acc[0], acc[1], c[0], c[1]);
            else il4_decode(acc, c);
#pragma unroll
            for (int k = 0; k < U; ++k)
                if (c[k]) atomicOr(col_or + (int64_t)u * U + k, c[k]);
        }
    }
}

hipError_t launch_occupancy(const uint32_t *rows, int64_t nrows, int Ww, int il, uint32_t *col_or, uint32_t *row_or,
                            hipStream_t s) {
    if (nrows <= 0) return hipSuccess;
    if ((il != 0 && il != 2 && il != 4) || Ww < 1 || (il && Ww % il)) return hipErrorInvalidValue;
    const int U = il == 0 ? 1 : il;
    const int64_t tasks = ((Ww / U + 255) / 256) * ((nrows + kOccRows - 1) / kOccRows);
    const dim3 grid((unsigned)std::min<int64_t>(tasks, kOccMaxBlocks)), block(256);
    if (il == 0) hipLaunchKernelGGL(gol_occupancy_kernel<0>, grid, block, 0, s, rows, nrows, Ww, col_or, row_or);
    if (il == 2) hipLaunchKernelGGL(gol_occupancy_kernel<2>, grid, block, 0, s, rows, nrows, Ww, col_or, row_or);
    if (il == 4) hipLaunchKernelGGL(gol_occupancy_kernel<4>, grid, block, 0, s, rows, nrows, Ww, col_or, row_or);
    return hipGetLastError();
}

}  // namespace golk
