// gol_layout.h — the interleaved word layouts of the step kernels (DESIGN.md
// §4), shared by the translation units that read a board in the layout it is
// stepped in (gol_kernels.hip, gol_view.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace golk {

// ---------------------------------------------------------------------------
// Interleaved pair layout (boards run with two words per lane, W % 64 == 0).
// A row's canonical words (2c, 2c+1) hold cells 64c .. 64c+63 in order; the
// interleaved pair holds the even cells 64c+2k in bit k of word 2c and the
// odd cells 64c+2k+1 in bit k of word 2c+1.  Rows stay rows, so halo rows,
// strips and popcounts are layout-agnostic; only cell positions change.
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t unshuffle32(uint32_t x) {  // even bits -> low half, odd -> high
    uint32_t t;
    t = (x ^ (x >> 1)) & 0x22222222u; x ^= t ^ (t << 1);
    t = (x ^ (x >> 2)) & 0x0C0C0C0Cu; x ^= t ^ (t << 2);
    t = (x ^ (x >> 4)) & 0x00F000F0u; x ^= t ^ (t << 4);
    t = (x ^ (x >> 8)) & 0x0000FF00u; x ^= t ^ (t << 8);
    return x;
}
__host__ __device__ __forceinline__ uint32_t shuffle32(uint32_t x) {  // inverse of unshuffle32
    uint32_t t;
    t = (x ^ (x >> 8)) & 0x0000FF00u; x ^= t ^ (t << 8);
    t = (x ^ (x >> 4)) & 0x00F000F0u; x ^= t ^ (t << 4);
    t = (x ^ (x >> 2)) & 0x0C0C0C0Cu; x ^= t ^ (t << 2);
    t = (x ^ (x >> 1)) & 0x22222222u; x ^= t ^ (t << 1);
    return x;
}
__host__ __device__ __forceinline__ void il_encode(uint32_t a, uint32_t b, uint32_t &e, uint32_t &o) {
    const uint32_t ua = unshuffle32(a), ub = unshuffle32(b);
    e = (ua & 0xFFFFu) | (ub << 16);
    o = (ua >> 16) | (ub & 0xFFFF0000u);
}
__host__ __device__ __forceinline__ void il_decode(uint32_t e, uint32_t o, uint32_t &a, uint32_t &b) {
    a = shuffle32((e & 0xFFFFu) | (o << 16));
    b = shuffle32((e >> 16) | (o & 0xFFFF0000u));
}
// Interleaved quad layout (four words per lane, W % 128 == 0): word 4q + j of
// a row holds the cells 128q + 4k + j in bit k.  It is the pair layout applied
// twice: the pair encoding of (a, b) and (c, d) gives the even and odd cells
// of each 64-cell half; pairing the two even-cell words (e1, e2) again splits
// them into cells 4k (j = 0) and 4k + 2 (j = 2), the odd-cell words into
// 4k + 1 (j = 1) and 4k + 3 (j = 3).
__host__ __device__ __forceinline__ void il4_encode(const uint32_t (&c)[4], uint32_t (&w)[4]) {
    uint32_t e1, o1, e2, o2;
    il_encode(c[0], c[1], e1, o1);
    il_encode(c[2], c[3], e2, o2);
    il_encode(e1, e2, w[0], w[2]);
    il_encode(o1, o2, w[1], w[3]);
}
__host__ __device__ __forceinline__ void il4_decode(const uint32_t (&w)[4], uint32_t (&c)[4]) {
    uint32_t e1, o1, e2, o2;
    il_decode(w[0], w[2], e1, e2);
    il_decode(w[1], w[3], o1, o2);
    il_decode(e1, o1, c[0], c[1]);
    il_decode(e2, o2, c[2], c[3]);
}
// Canonical word i of a board stored in layout `il` (0 canonical, 2 pairs, 4 quads).
__device__ __forceinline__ uint32_t canon_word(const uint32_t *w, int64_t i, int il) {
    if (il == 0) return w[i];
    if (il == 2) {
        uint32_t a, b;
        il_decode(w[i & ~(int64_t)1], w[i | 1], a, b);
        return (i & 1) ? b : a;
    }
    const uint4 q = *reinterpret_cast<const uint4 *>(w + (i & ~(int64_t)3));
    uint32_t c[4];
    il4_decode({q.x, q.y, q.z, q.w}, c);
    return c[i & 3];
}

}  // namespace golk
