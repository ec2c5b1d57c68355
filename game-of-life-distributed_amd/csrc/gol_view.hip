// gol_view.hip — K7, the live view: a frame of out_w x out_h pixels from the
// bit board, one pixel per s x s block of cells (golhip_view_frame,
// golhip_view_stream; the reference's window sdl/window.go is the s = 1 case).
//
// The board is read where it lies, in the layout it is stepped in (canonical
// words, interleaved pairs or quads): the pointer is const and
// nothing is converted.  Two kernels, by how pixels relate to words:
//   gol_view_kernel       s >= 32: a pixel spans words.  A lane owns one
//     group column (1, 2 or 4 words: 4, 8 or 16 B a load, consecutive across
//     the lanes) and walks the s rows of a pixel row, popcounting the group
//     under per-pixel masks that are built once, in the board's own layout (so
//     no word is ever decoded); lanes of one pixel meet in LDS.
//   gol_view_small_kernel s < 32: a word holds several pixels.  A lane owns
//     16 B of output pixels and streams the row words under them, taking each
//     pixel's s-bit field from a 64-bit window, summed over s rows.
// Both handle the torus seams themselves: y wraps by row index, x wraps by
// group index, and on widths with W % 32 != 0 (canonical layout only) the last
// word of a row holds W % 32 cells and the block that straddles the seam
// continues with bit 0 of word 0.
// Pixels are stored once each, 16 B a lane where the frame allows, else one
// pixel a store: the frame may be host memory, so no atomics and no
// read-modify-write on it.
//
// A board held as row strips (golhip_group_view_frame): a pixel row whose s
// board rows lie in one strip is rendered by that strip with the kernels above.
// A pixel row that straddles strips is rendered in pieces: every strip runs
// its kernel in counts mode (template parameter COUNTS) over the rows
// [r_lo, r_hi) of the pixel row that it holds and stores the raw alive counts,
// uint32 a pixel, to a row of a device buffer; gol_view_resolve_kernel sums
// the k >= 2 count rows of each such pixel row, normalises and stores the
// pixels.  The masks and the x-seam logic do not know about the pieces.
#include "gol_kernels.h"
#include "gol_layout.h"

#include "../../include/golhip.h"

#include <algorithm>
#include <climits>

namespace golk {
namespace {

constexpr int kViewThreads = 256;
constexpr int kViewMaxPix = 1024;  // most pixels one block of gol_view_kernel owns (its LDS accumulators)

template <int IL>
struct Group {
    static constexpr int kWords = IL == 0 ? 1 : IL;
    static constexpr int kBits = 32 * kWords;
};

// Words of group g of a row, as stored.
template <int IL>
__device__ __forceinline__ void load_group(const uint32_t *__restrict__ row, int g, uint32_t (&w)[Group<IL>::kWords]) {
    if constexpr (IL == 4) {
        const uint4 q = reinterpret_cast<const uint4 *>(row)[g];
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else if constexpr (IL == 2) {
        const uint2 q = reinterpret_cast<const uint2 *>(row)[g];
        w[0] = q.x, w[1] = q.y;
    } else {
        w[0] = row[g];
    }
}

// Canonical words of group g of a row.
template <int IL>
__device__ __forceinline__ void load_group_canon(const uint32_t *__restrict__ row, int g,
                                                 uint32_t (&c)[Group<IL>::kWords]) {
    uint32_t w[Group<IL>::kWords];
    load_group<IL>(row, g, w);
    if constexpr (IL == 4) {
        il4_decode(w, c);
    } else if constexpr (IL == 2) {
        il_decode(w[0], w[1], c[0], c[1]);
    } else {
        c[0] = w[0];
    }
}

// Bits [lo, hi) of a 32-bit word (clamped to the word).
__device__ __forceinline__ uint32_t range_mask(int lo, int hi) {
    lo = max(lo, 0);
    hi = min(hi, 32);
    if (hi <= lo) return 0u;
    return (hi - lo == 32) ? ~0u : (((1u << (hi - lo)) - 1u) << lo);
}

// Cells [lo, hi) of a group as a mask over its words as stored.
template <int IL>
__device__ __forceinline__ void group_mask(int lo, int hi, uint32_t (&m)[Group<IL>::kWords]) {
    uint32_t c[Group<IL>::kWords];
#pragma unroll
    for (int j = 0; j < Group<IL>::kWords; ++j) c[j] = range_mask(lo - 32 * j, hi - 32 * j);
    if constexpr (IL == 4) {
        il4_encode(c, m);
    } else if constexpr (IL == 2) {
        il_encode(c[0], c[1], m[0], m[1]);
    } else {
        m[0] = c[0];
    }
}

// g = ceil(255 n / s^2): 0 only for an empty block, 255 for a full one.
__device__ __forceinline__ uint32_t gray_of(uint32_t n, uint32_t s2) { return (255u * n + s2 - 1u) / s2; }

template <int FORMAT>
struct Pixel {
    static constexpr int kPer16 = FORMAT == GOLHIP_VIEW_GRAY8 ? 16 : 4;  // pixels in a 16-byte store
};

// Pixels [i, i + n) of the frame from their grey values (n <= kPer16; vec:
// all kPer16 in one 16-byte store at an aligned address).
template <int FORMAT>
__device__ __forceinline__ void store_pixels(void *__restrict__ out, int64_t i, const uint32_t (&g)[Pixel<FORMAT>::kPer16],
                                             int n, bool vec) {
    if constexpr (FORMAT == GOLHIP_VIEW_GRAY8) {
        uint8_t *o = static_cast<uint8_t *>(out) + i;
        if (vec) {
            uint4 v;
            v.x = g[0] | g[1] << 8 | g[2] << 16 | g[3] << 24;
            v.y = g[4] | g[5] << 8 | g[6] << 16 | g[7] << 24;
            v.z = g[8] | g[9] << 8 | g[10] << 16 | g[11] << 24;
            v.w = g[12] | g[13] << 8 | g[14] << 16 | g[15] << 24;
            *reinterpret_cast<uint4 *>(o) = v;
        } else {
#pragma unroll
            for (int p = 0; p < 16; ++p)
                if (p < n) o[p] = (uint8_t)g[p];
        }
    } else {
        uint32_t *o = static_cast<uint32_t *>(out) + i;
        if (vec) {
            *reinterpret_cast<uint4 *>(o) =
                make_uint4(g[0] * 0x01010101u, g[1] * 0x01010101u, g[2] * 0x01010101u, g[3] * 0x01010101u);
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (p < n) o[p] = g[p] * 0x01010101u;
        }
    }
}

// 32 cells of a row from torus column x on, for any width: the last word of a
// row holds W - 32 (Ww - 1) cells (padding bits zero) and the cells after
// column W - 1 are those of column 0 on.
__device__ __forceinline__ uint32_t fetch32_seam(const uint32_t *__restrict__ row, int W, int x) {
    uint32_t out = 0;
    for (int got = 0; got < 32;) {
        const int wi = x >> 5, sh = x & 31;
        const int valid = min(32, W - 32 * wi) - sh;
        out |= (row[wi] >> sh) << got;
        got += valid;
        x += valid;
        if (x >= W) x = 0;
    }
    return out;
}

// The canonical words of a row in order from a start column, wrapping at the
// row's end; on a seam width, 32-cell windows from the start column instead.
template <int IL>
struct RowCursor {
    const uint32_t *row;
    int W, Ww, wi, x;
    bool seam;
    uint32_t c[Group<IL>::kWords];

    // Returns the bit of the first word at which the start column sits.
    __device__ __forceinline__ int begin(const uint32_t *__restrict__ r, int W_, int Ww_, int xs) {
        row = r, W = W_, Ww = Ww_, x = xs, wi = xs >> 5;
        seam = IL == 0 && (W & 31) != 0;
        if constexpr (IL != 0) load_group_canon<IL>(row, wi / IL, c);
        return seam ? 0 : (xs & 31);
    }
    __device__ __forceinline__ uint32_t next() {
        uint32_t v;
        if constexpr (IL == 0) {
            if (seam) {
                v = fetch32_seam(row, W, x);
                x = (x + 32) % W;
                return v;
            }
            v = row[wi];
        } else {
            const int sub = wi & (IL - 1);
            v = c[0];
#pragma unroll
            for (int j = 1; j < IL; ++j) v = sub == j ? c[j] : v;
        }
        if (++wi == Ww) wi = 0;
        if constexpr (IL != 0)
            if ((wi & (IL - 1)) == 0) load_group_canon<IL>(row, wi / IL, c);
        return v;
    }
};

// s < 32.  One thread: Pixel::kPer16 consecutive pixels of one pixel row.
// COUNTS: rows [a.r_lo, a.r_hi) of the one pixel row whose row 0 is local row
// a.y0 (which may lie outside the strip; the rows read do not), raw counts to
// the uint32 row a.out (4 a lane: FORMAT is ARGB8888).
template <int IL, int FORMAT, bool COUNTS = false>
__global__ __launch_bounds__(kViewThreads) void gol_view_small_kernel(ViewArgs a) {
    constexpr int G = Pixel<FORMAT>::kPer16;
    static_assert(!COUNTS || G == 4, "counts mode stores one uint4 a lane");
    const int64_t t = (int64_t)blockIdx.x * kViewThreads + threadIdx.x;
    const int ngx = (a.out_w + G - 1) / G;
    const int py = (int)(t / ngx);
    if (py >= a.out_h) return;
    const int px0 = (int)(t - (int64_t)py * ngx) * G;
    const int s = a.s;
    const uint32_t smask = (1u << s) - 1u;
    int64_t xs64 = (int64_t)a.x0 + (int64_t)px0 * s;
    if (xs64 >= a.W) xs64 -= a.W;
    const int xs = (int)xs64;
    int yy = a.y0 + py * s;  // < 2 H
    if constexpr (COUNTS) {
        yy = a.y0 + a.r_lo;
    } else {
        if (yy >= a.H) yy -= a.H;
    }
    const int nr = COUNTS ? a.r_hi - a.r_lo : s;
    uint32_t acc[G];
#pragma unroll
    for (int p = 0; p < G; ++p) acc[p] = 0;
    for (int r = 0; r < nr; ++r) {
        RowCursor<IL> cur;
        int off = cur.begin(a.rows + (int64_t)yy * a.Ww, a.W, a.Ww, xs);
        uint32_t lo = cur.next(), hi = cur.next();
#pragma unroll
        for (int p = 0; p < G; ++p) {
            const uint64_t win = ((uint64_t)hi << 32) | lo;
            acc[p] += __popc((uint32_t)(win >> off) & smask);
            off += s;
            if (off >= 32) {
                off -= 32;
                lo = hi;
                hi = cur.next();
            }
        }
        if (++yy == a.H) yy = 0;  // never in counts mode: a piece lies inside the strip
    }
    if constexpr (COUNTS) {
        // the count row is padded to kViewCountAlign pixels: always one 16-byte store
        *reinterpret_cast<uint4 *>(static_cast<uint32_t *>(a.out) + px0) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
    } else {
        const uint32_t s2 = (uint32_t)(s * s);
        uint32_t g[G];
#pragma unroll
        for (int p = 0; p < G; ++p) g[p] = gray_of(acc[p], s2);
        store_pixels<FORMAT>(a.out, (int64_t)py * a.out_w + px0, g, min(G, a.out_w - px0), a.vec != 0);
    }
}

// s >= 32.  One block: pixels [p0, p0 + np) of one pixel row (np <= a.pb <=
// kViewMaxPix); its threads share out the group columns under those pixels.
// Group k of the walk that starts at the viewport's first group (a.gfirst) is
// group (a.gfirst + k) mod a.ngr of a row, on lap (a.gfirst + k) / a.ngr, and
// starts at column lap * W + 32 * words * index of the unrolled torus.
// COUNTS: as in gol_view_small_kernel.
template <int IL, int FORMAT, bool COUNTS = false>
__global__ __launch_bounds__(kViewThreads) void gol_view_kernel(ViewArgs a) {
    constexpr int GW = Group<IL>::kWords, GB = Group<IL>::kBits;
    constexpr int NSEG = GW + 1;  // pixels one group can touch (s >= 32)
    __shared__ uint32_t pix[kViewMaxPix];
    const int nchunk = (a.out_w + a.pb - 1) / a.pb;
    const int py = blockIdx.x / nchunk;
    const int p0 = (blockIdx.x - py * nchunk) * a.pb;
    const int np = min(a.pb, a.out_w - p0);
    const int s = a.s;
    for (int i = threadIdx.x; i < np; i += kViewThreads) pix[i] = 0;
    __syncthreads();

    // viewport-relative columns [rel_lo, rel_hi) of this block, and the walk's groups under them
    const int64_t rel_lo = (int64_t)p0 * s, rel_hi = (int64_t)(p0 + np) * s;
    auto walk_of = [&](int64_t u) -> int {  // unrolled column u in [x0, x0 + W) -> group of the walk
        return u < a.W ? (int)(u / GB) - a.gfirst : (a.ngr - a.gfirst) + (int)((u - a.W) / GB);
    };
    const int k_lo = walk_of(a.x0 + rel_lo), k_hi = walk_of(a.x0 + rel_hi - 1);
    int y_first = a.y0 + py * s;  // < 2 H
    if constexpr (COUNTS) {
        y_first = a.y0 + a.r_lo;
    } else {
        if (y_first >= a.H) y_first -= a.H;
    }
    const int nr = COUNTS ? a.r_hi - a.r_lo : s;

    for (int k = k_lo + (int)threadIdx.x; k <= k_hi; k += kViewThreads) {
        const int gk = a.gfirst + k;
        const int lap = gk >= a.ngr ? 1 : 0;
        const int gi = gk - lap * a.ngr;
        const int valid = min(GB, a.W - gi * GB);
        const int64_t rel0 = (int64_t)lap * a.W + (int64_t)gi * GB - a.x0;  // viewport column of the group's cell 0
        const int64_t lo = max(rel0, rel_lo), hi = min(rel0 + valid, rel_hi);
        const int pf = (int)(lo / s);
        uint32_t m[NSEG][GW];
        uint32_t acc[NSEG];
#pragma unroll
        for (int j = 0; j < NSEG; ++j) {
            const int64_t b_lo = max((int64_t)(pf + j) * s, lo), b_hi = min((int64_t)(pf + j + 1) * s, hi);
            group_mask<IL>((int)(b_lo - rel0), b_hi > b_lo ? (int)(b_hi - rel0) : (int)(b_lo - rel0), m[j]);
            acc[j] = 0;
        }
        int yy = y_first;
        const uint32_t *row = a.rows + (int64_t)yy * a.Ww;
#pragma unroll 4
        for (int r = 0; r < nr; ++r) {
            uint32_t w[GW];
            load_group<IL>(row, gi, w);
#pragma unroll
            for (int j = 0; j < NSEG; ++j)
#pragma unroll
                for (int i = 0; i < GW; ++i) acc[j] += __popc(w[i] & m[j][i]);
            row += a.Ww;
            if (++yy == a.H) yy = 0, row = a.rows;
        }
#pragma unroll
        for (int j = 0; j < NSEG; ++j)
            if (acc[j] && pf + j - p0 < np) atomicAdd(&pix[pf + j - p0], acc[j]);  // LDS
    }
    __syncthreads();

    constexpr int G = Pixel<FORMAT>::kPer16;
    if constexpr (COUNTS) {
        // p0 and u are multiples of 4 and the count row is padded: 16-byte stores
        uint32_t *o = static_cast<uint32_t *>(a.out) + p0;
        for (int u = threadIdx.x * 4; u < np; u += kViewThreads * 4) {
            uint32_t c[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) c[p] = u + p < np ? pix[u + p] : 0u;
            *reinterpret_cast<uint4 *>(o + u) = make_uint4(c[0], c[1], c[2], c[3]);
        }
    } else {
        const uint32_t s2 = (uint32_t)(s * s);
        const int64_t base = (int64_t)py * a.out_w + p0;
        for (int u = threadIdx.x * G; u < np; u += kViewThreads * G) {
            uint32_t g[G];
#pragma unroll
            for (int p = 0; p < G; ++p) g[p] = u + p < np ? gray_of(pix[u + p], s2) : 0u;
            store_pixels<FORMAT>(a.out, base + u, g, min(G, np - u), a.vec != 0);
        }
    }
}

// Pixel rows that straddle strips: block row j sums the a.k[j] count rows from
// row a.slot[j] of a.counts on and stores pixel row a.py[j] of the frame.  One
// thread: Pixel::kPer16 consecutive pixels.
template <int FORMAT>
__global__ __launch_bounds__(kViewThreads) void gol_view_resolve_kernel(ViewResolveArgs a) {
    constexpr int G = Pixel<FORMAT>::kPer16;
    const int j = blockIdx.y;
    const int px0 = (int)(blockIdx.x * kViewThreads + threadIdx.x) * G;
    if (px0 >= a.out_w) return;
    uint32_t acc[G];
#pragma unroll
    for (int p = 0; p < G; ++p) acc[p] = 0;
    const uint32_t *c = a.counts + (int64_t)a.slot[j] * a.cw + px0;  // px0 + G <= cw (kViewCountAlign)
    for (int i = 0; i < a.k[j]; ++i) {
#pragma unroll
        for (int q = 0; q < G / 4; ++q) {
            const uint4 v = reinterpret_cast<const uint4 *>(c)[q];
            acc[4 * q] += v.x, acc[4 * q + 1] += v.y, acc[4 * q + 2] += v.z, acc[4 * q + 3] += v.w;
        }
        c += a.cw;
    }
    const uint32_t s2 = (uint32_t)(a.s * a.s);
    uint32_t g[G];
#pragma unroll
    for (int p = 0; p < G; ++p) g[p] = gray_of(acc[p], s2);
    store_pixels<FORMAT>(a.out, (int64_t)a.py[j] * a.out_w + px0, g, min(G, a.out_w - px0), a.vec != 0);
}

template <int IL, int FORMAT>
hipError_t launch_view_t(const ViewArgs &a, hipStream_t st) {
    if (a.s < 32) {
        const int64_t threads = (int64_t)a.out_h * ((a.out_w + Pixel<FORMAT>::kPer16 - 1) / Pixel<FORMAT>::kPer16);
        const int64_t blocks = (threads + kViewThreads - 1) / kViewThreads;
        if (blocks > INT32_MAX) return hipErrorInvalidValue;
        hipLaunchKernelGGL((gol_view_small_kernel<IL, FORMAT>), dim3((unsigned)blocks), dim3(kViewThreads), 0, st, a);
    } else {
        const int64_t blocks = (int64_t)a.out_h * ((a.out_w + a.pb - 1) / a.pb);
        if (blocks > INT32_MAX || a.pb < 16 || a.pb > kViewMaxPix || a.pb % 16) return hipErrorInvalidValue;
        hipLaunchKernelGGL((gol_view_kernel<IL, FORMAT>), dim3((unsigned)blocks), dim3(kViewThreads), 0, st, a);
    }
    return hipGetLastError();
}

template <int IL>
hipError_t launch_counts_t(const ViewArgs &a, hipStream_t st) {
    constexpr int F = GOLHIP_VIEW_ARGB8888;
    if (a.s < 32) {
        const int blocks = ((a.out_w + 3) / 4 + kViewThreads - 1) / kViewThreads;
        hipLaunchKernelGGL((gol_view_small_kernel<IL, F, true>), dim3((unsigned)blocks), dim3(kViewThreads), 0, st, a);
    } else {
        const int blocks = (a.out_w + a.pb - 1) / a.pb;
        hipLaunchKernelGGL((gol_view_kernel<IL, F, true>), dim3((unsigned)blocks), dim3(kViewThreads), 0, st, a);
    }
    return hipGetLastError();
}

// The fields of ViewArgs that the launchers derive.
bool view_derive(ViewArgs &a) {
    const int gw = a.il == 0 ? 1 : a.il, gb = 32 * gw;
    if (!(a.il == 0 || a.il == 2 || a.il == 4) || a.Ww % gw != 0 || (a.il != 0 && a.W % gb != 0)) return false;
    a.ngr = a.Ww / gw;
    a.gfirst = a.x0 / gb;
    // gol_view_kernel: about one group column per thread, whole 16-byte units per block
    a.pb = (int)std::min<int64_t>(kViewMaxPix, std::max<int64_t>(16, ((int64_t)kViewThreads * gb / a.s) / 16 * 16));
    return true;
}

}  // namespace

int view_count_stride(int out_w) { return (out_w + kViewCountAlign - 1) / kViewCountAlign * kViewCountAlign; }

hipError_t launch_view_counts(ViewArgs a, hipStream_t st) {
    if (!view_derive(a)) return hipErrorInvalidValue;
    // the rows read are rows of the strip; one pixel row; an aligned count row
    if (a.r_lo < 0 || a.r_hi > a.s || a.r_lo >= a.r_hi || a.y0 + a.r_lo < 0 || a.y0 + a.r_hi > a.H ||
        (uintptr_t)a.out % 16 != 0 || a.out_w < 1)
        return hipErrorInvalidValue;
    a.out_h = 1;
    a.vec = 1;
    switch (a.il) {
    case 0:
        return launch_counts_t<0>(a, st);
    case 2:
        return launch_counts_t<2>(a, st);
    default:
        return launch_counts_t<4>(a, st);
    }
}

hipError_t launch_view_resolve(ViewResolveArgs a, hipStream_t st) {
    if (a.nrows < 1 || a.nrows > kViewResolveRows || a.cw != view_count_stride(a.out_w) ||
        (uintptr_t)a.counts % 16 != 0)
        return hipErrorInvalidValue;
    const int per16 = a.format == GOLHIP_VIEW_GRAY8 ? 16 : 4;
    a.vec = ((uintptr_t)a.out % 16 == 0 && a.out_w % per16 == 0) ? 1 : 0;
    const dim3 grid((unsigned)(((a.out_w + per16 - 1) / per16 + kViewThreads - 1) / kViewThreads), (unsigned)a.nrows);
    if (a.format == GOLHIP_VIEW_GRAY8)
        hipLaunchKernelGGL((gol_view_resolve_kernel<GOLHIP_VIEW_GRAY8>), grid, dim3(kViewThreads), 0, st, a);
    else
        hipLaunchKernelGGL((gol_view_resolve_kernel<GOLHIP_VIEW_ARGB8888>), grid, dim3(kViewThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_view(ViewArgs a, hipStream_t st) {
    const int gw = a.il == 0 ? 1 : a.il, gb = 32 * gw;
    if (!(a.il == 0 || a.il == 2 || a.il == 4) || a.Ww % gw != 0 || (a.il != 0 && a.W % gb != 0))
        return hipErrorInvalidValue;
    a.ngr = a.Ww / gw;
    a.gfirst = a.x0 / gb;
    // 16-byte stores: every 16-byte unit of the frame starts a whole unit into a pixel row
    const int per16 = a.format == GOLHIP_VIEW_GRAY8 ? 16 : 4;
    a.vec = ((uintptr_t)a.out % 16 == 0 && a.out_w % per16 == 0) ? 1 : 0;
    // gol_view_kernel: about one group column per thread, whole 16-byte units per block
    a.pb = (int)std::min<int64_t>(kViewMaxPix, std::max<int64_t>(16, ((int64_t)kViewThreads * gb / a.s) / 16 * 16));
    const bool gray = a.format == GOLHIP_VIEW_GRAY8;
    switch (a.il) {
    case 0:
        return gray ? launch_view_t<0, GOLHIP_VIEW_GRAY8>(a, st) : launch_view_t<0, GOLHIP_VIEW_ARGB8888>(a, st);
    case 2:
        return gray ? launch_view_t<2, GOLHIP_VIEW_GRAY8>(a, st) : launch_view_t<2, GOLHIP_VIEW_ARGB8888>(a, st);
    default:
        return gray ? launch_view_t<4, GOLHIP_VIEW_GRAY8>(a, st) : launch_view_t<4, GOLHIP_VIEW_ARGB8888>(a, st);
    }
}

}  // namespace golk
