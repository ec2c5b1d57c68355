// gol_pad_plan.h — the arithmetic of the padded torus: a
// W-column torus with W % 32 != 0 stepped as a Wp-column torus whose extra
// columns are ghost copies of real ones.  Plain integers and words, no HIP
// call: the host planner, the pad kernels (gol_pad.hip) and the CPU test
// (tests/test_pad_plan_cpu.py, compiled alone under the sanitizers) share it.
//
//   Wp  = roundup(W + 64, 64), pad = Wp - W in [64, 127]
//   gR  = ceil(pad / 2) ghost columns right of the real ones, gL = pad - gR
//         left of column 0 (at the far end of the wide row); both >= 32, the
//         deepest launch, so after d <= 32 turns the error of a stale ghost
//         (one cell a turn) has not reached a real column
//   column c in [W, W + gR)  holds real column (c - W)  mod W
//   column c in [W + gR, Wp) holds real column (c - Wp) mod W
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define GOL_PAD_FN __host__ __device__ __forceinline__
#else
#define GOL_PAD_FN inline
#endif

namespace golk {

struct PadPlan {
    int W;       // real columns
    int Wp;      // columns of the wide torus (a multiple of 64)
    int gR, gL;  // ghost columns behind column W - 1 / in front of column 0
};

// Widest board the plan takes: Wp must fit an int.
constexpr int kPadMaxW = 0x7FFFFFFF - 127;

// The plan of a W-column board; false if there is none (W < 1 or too wide).
GOL_PAD_FN bool pad_plan(int W, PadPlan *p) {
    if (W < 1 || W > kPadMaxW) return false;
    p->W = W;
    p->Wp = (W + 64 + 63) / 64 * 64;
    const int pad = p->Wp - W;
    p->gR = (pad + 1) / 2;
    p->gL = pad - p->gR;
    return true;
}

// The real column that column c of the wide row holds (0 <= c < Wp).
GOL_PAD_FN int pad_src_col(const PadPlan &p, int c) {
    if (c < p.W) return c;
    if (c < p.W + p.gR) return (c - p.W) % p.W;
    const int r = (c - p.Wp) % p.W;  // c - Wp in [-gL, 0)
    return r < 0 ? r + p.W : r;
}

// 32 columns of the real row from column `start` on (0 <= start < W) by a
// funnel shift across the word boundary; fetch(i) is word i < nsrc of the real
// columns.  Only the bits of columns < W mean anything: callers mask.
template <class Fetch>
GOL_PAD_FN uint32_t pad_bits(Fetch &&fetch, int nsrc, int start) {
    const int w = start >> 5, sh = start & 31;
    const uint32_t lo = fetch(w);
    if (sh == 0) return lo;
    const uint32_t hi = w + 1 < nsrc ? fetch(w + 1) : 0u;
    return (lo >> sh) | (hi << (32 - sh));
}

// Canonical word j (columns 32 j .. 32 j + 31) of the wide row, from the
// words of its real columns (fetch(i), i < nsrc = ceil(W / 32); bits of
// columns >= W in the last one are ignored).  W >= 64: a ghost is one run of
// real columns, so the word is at most two runs of the real row joined by
// funnel shifts (the real row's end and the right ghost, or the right ghost's
// end and the left one).  Narrower boards replicate inside a ghost (the mod)
// and go bit by bit.
template <class Fetch>
GOL_PAD_FN uint32_t pad_wide_word(Fetch &&fetch, int nsrc, int j, const PadPlan &p) {
    const int c0 = 32 * j;
    if (c0 + 32 <= p.W) return fetch(j);
    uint32_t out = 0;
    if (p.W < 64) {
        for (int b = 0; b < 32; ++b) {
            const int s = pad_src_col(p, c0 + b);
            out |= ((fetch(s >> 5) >> (s & 31)) & 1u) << b;
        }
        return out;
    }
    for (int c = c0; c < c0 + 32;) {
        int end, src;  // the run of columns [c, end) holds the real columns from src on
        if (c < p.W) {
            end = p.W;
            src = c;
        } else if (c < p.W + p.gR) {
            end = p.W + p.gR;
            src = c - p.W;
        } else {
            end = p.Wp;
            src = c - (p.Wp - p.W);
        }
        const int n = (end < c0 + 32 ? end : c0 + 32) - c;
        uint32_t bits = pad_bits(fetch, nsrc, src);
        if (n < 32) bits &= (1u << n) - 1u;
        out |= bits << (c - c0);
        c += n;
    }
    return out;
}

}  // namespace golk
