// gol_box.h — the alive box of a torus from its occupancy bitmaps (DESIGN.md
// §5.22; golhip_box_interval, golhip_alive_box).  Plain C++17 with no device
// header: the engine and a stand-alone test program include the same code.
//
// On a cyclic axis of n positions the box's side is the shortest cyclic
// interval (start, len) that covers every set bit of the axis' occupancy
// bitmap: the complement of the longest cyclic run of clear bits.  Where
// several runs tie for longest, the interval with the smallest start is taken.
// No set bit: len 0 (start 0).  No clear bit: (0, n).
#pragma once
#include <cstdint>

namespace golbox {

struct Interval {
    int64_t start = 0, len = 0;
};

// bits: ceil(n / 32) words, position p = bit p % 32 of word p / 32; the bits
// of positions >= n are not looked at.
inline Interval interval(const uint32_t *bits, int64_t n) {
    int64_t first = -1, prev = -1, best_gap = -1, best_start = 0;
    const int64_t nw = (n + 31) / 32;
    for (int64_t w = 0; w < nw; ++w) {
        uint32_t v = bits[w];
        if (w == nw - 1 && (n & 31)) v &= (1u << (n & 31)) - 1u;
        while (v) {
            const int64_t p = 32 * w + __builtin_ctz(v);
            v &= v - 1;
            if (first < 0) {
                first = p;
            } else if (p - prev - 1 > best_gap) {  // (starts grow along the scan: the first of equals stays)
                best_gap = p - prev - 1;
                best_start = p;
            }
            prev = p;
        }
    }
    if (first < 0) return {};
    // the run of clear bits across the seam; its interval starts at the smallest position of all
    const int64_t wrap = first + n - prev - 1;
    if (wrap >= best_gap) {
        best_gap = wrap;
        best_start = first;
    }
    return {best_start, n - best_gap};
}

// The same axis on a bounded plane, which has no seam to straddle: the plain
// interval from the smallest to the largest set position.
inline Interval interval_plane(const uint32_t *bits, int64_t n) {
    int64_t first = -1, last = -1;
    const int64_t nw = (n + 31) / 32;
    for (int64_t w = 0; w < nw; ++w) {
        uint32_t v = bits[w];
        if (w == nw - 1 && (n & 31)) v &= (1u << (n & 31)) - 1u;
        if (!v) continue;
        if (first < 0) first = 32 * w + __builtin_ctz(v);
        last = 32 * w + 31 - __builtin_clz(v);
    }
    if (first < 0) return {};
    return {first, last - first + 1};
}

// Sets bits [at, at + count) of `dst` from the low `count` bits of `src` words
// (the rows of one strip appended to the board's row bitmap).
inline void append_bits(uint32_t *dst, int64_t at, const uint32_t *src, int64_t count) {
    for (int64_t w = 0; 32 * w < count; ++w) {
        uint32_t v = src[w];
        if (count - 32 * w < 32) v &= (1u << (count - 32 * w)) - 1u;
        if (!v) continue;
        const int64_t p = at + 32 * w, sh = p & 31;
        dst[p >> 5] |= v << sh;
        if (sh && (v >> (32 - sh))) dst[(p >> 5) + 1] |= v >> (32 - sh);
    }
}

}  // namespace golbox
