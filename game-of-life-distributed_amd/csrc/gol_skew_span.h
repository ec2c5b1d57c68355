// gol_skew_span.h — the interior span of a K1w band's main loop (DESIGN.md
// §5.20): the run of loop bodies in which nothing the general body decides
// row by row can change, so that a second loop body without those decisions
// (gol_kernels.hip stream_skew) computes the same.  Plain integers, no HIP
// call: the kernel, the host (golhip_skew_span) and the CPU test
// (tests/test_skew_interior_cpu.py) share it.
//
// The main loop pushes the band's input rows three at a time (push k takes
// rows k, k + 1, k + 2 of the band's input frame, row 0 = `ab`); a body is one
// group (the 9-LUT stages) or two (the pair rule).  The body at push k
//   loads the input rows k + 3 .. k + B + 2 (B = 3 or 6 rows a body) through
//         the row map: r = (ab + dr + off + row) mod wrap, min(r, rmax);
//   stores the output rows oi = k - 3 - 2 D .. k - 4 - 2 D + B of the band,
//         each only where 0 <= oi < S = eb - ab;
//   counts the stored words of the rows in [count_lo, count_hi).
// It is interior when its B input rows neither wrap nor clamp, all its output
// rows are inside the band and the launch counts nothing.  With half-wave
// tiles the upper lanes run the same band `dr` rows further down: one span for
// the wave, so the rows of both halves must qualify.
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#define GOL_SPAN_FN __host__ __device__ __forceinline__
#else
#define GOL_SPAN_FN inline
#endif

namespace golk {

// Stages of a K1w fill / drain phase at depth D (SkewPlan<D>::STEP).
constexpr int skew_phase_step(int D) { return D > 20 ? 6 : 3; }
// The main loop's first push: the fill ends at 2 D, rounded to a whole group.
constexpr int skew_main_start(int D) { return 3 * ((2 * D + 2) / 3); }
// The pair rule's main loop takes two groups a body and so starts at an even
// group: where the fill would end on an odd one (D = 16: push 33) its last
// phase runs one more full-depth group (36).  The other pair depths (8, 12,
// 15, 18) end their fill on an even group already.
constexpr int skew_main_start(int D, bool pair) {
    return pair ? 6 * ((skew_main_start(D) + 5) / 6) : skew_main_start(D);
}
// The pair-rule depths at two words per lane on full-width tiles that only a
// whole torus' step plan asks for (golhip_plan.cpp depth_plan), beside 18.
constexpr bool skew_pair_tail_depth(int D) { return D == 12 || D == 15 || D == 16; }
// The main loop's end: the drain of a band with a band below it in the stack
// starts at its first phase; a stack's bottom band (`self`) runs to the end.
constexpr int skew_main_end(int S, int D, bool self) { return S + (self ? 2 * D : 2 * skew_phase_step(D)); }

// The band of stack position `pos` (0 = top) of stack `stack` of a K1w launch
// over L rows (half tiles: L = half the launch's rows): the stacks split the
// input rows [-D, L - D), a stack's sy bands split its rows plus `hcap` by
// their weights wgt[], at multiples of G = 3 rows from the stack's start (6
// for the pair rule's two-group bodies); the bottom band takes the rest.
// (The host's restatement of gol_skew_kernel's own band arithmetic, for
// golhip_skew_interior_plan; the kernel keeps its lines as they are.)
struct SkewBand {
    int ab, eb;
    bool bottom;
};
GOL_SPAN_FN SkewBand skew_band(int L, int nst, int stack, int sy, int pos, const int *wgt, int hcap, int D, bool pair) {
    const int A0 = (int)((long long)stack * L / nst) - D, E0 = (int)((long long)(stack + 1) * L / nst) - D;
    const long long Ls = (long long)(E0 - A0) + hcap;
    int cum = 0, tot = 0;
    for (int q = 0; q < sy; ++q) {
        tot += wgt[q];
        cum += q < pos ? wgt[q] : 0;
    }
    const int G = pair ? 6 : 3;
    SkewBand b;
    b.bottom = pos == sy - 1;
    b.ab = A0 + (int)(Ls * cum / tot) / G * G;
    b.eb = b.bottom ? E0 : A0 + (int)(Ls * (cum + wgt[pos]) / tot) / G * G;
    return b;
}

// The K1w instances whose main loop has the interior body beside the general
// one: the pair rule at two words per lane on full-width tiles (18 turns a
// launch: 65536^2 and every strip of that width).  The others measured no gain
// or a loss (half-wave tiles, whose bands are mostly ramps,
// and quads at 9) and keep the one general loop; their spans are empty.
// The remainder launches of such a torus (12, 15 and 16 turns) carry it too.
constexpr bool skew_interior_instance(int D, int wpl, bool half, bool pair) {
    return pair && wpl == 2 && !half && (D == 18 || skew_pair_tail_depth(D));
}

struct SkewSpan {
    int k_lo, k_hi;  // the interior bodies are those at pushes [k_lo, k_hi): k_lo = k_hi if there are none
};

struct SkewSpanIn {
    int ab, eb;      // the band's input rows [ab, eb) (StepArgs frame)
    int D;           // turns a launch
    bool self;       // a stack's bottom band
    bool pair;       // the pair rule: bodies of two groups
    int off, wrap, rmax;  // the row map (RowMap; its base moves every row alike)
    bool half;       // half-wave tiles: the upper lanes' rows are `dr` further down
    int dr;
    int Ww;          // words a row (half tiles: both halves' rows are addressed from one base, 31-bit offsets)
    bool counts;     // the launch has an alive counter and a non-empty count range
    bool enabled;    // option "skew_interior"
};

namespace span_detail {

// One half's rows: the body at push k loads from row (c + k) mod wrap on.
struct Rows {
    unsigned c;  // wrap > 0: already reduced mod wrap
    long long cl;  // wrap = 0: the row itself is cl + k
    unsigned wrap;  // 0: no wrap
    int lim;   // the body is good iff its first row r has r <= lim
};

GOL_SPAN_FN long long first_row(const Rows &h, int k) {
    return h.wrap ? (long long)((h.c + (unsigned)k) % h.wrap) : h.cl + k;  // (c < wrap, k < 2^31: no carry out of 32 bits)
}

// Pushes to skip from k to the half's next good body (0: k is good; -1: none).
GOL_SPAN_FN int skip_to_good(const Rows &h, int k, int B) {
    const long long r = first_row(h, k);
    if (r <= h.lim) return 0;
    if (!h.wrap || h.lim < 0) return -1;
    return (int)(((long long)h.wrap - r + B - 1) / B) * B;  // over the wrap (the body there is checked again)
}

// Bodies of the half's run of good bodies that starts at the good body k, capped at `cap`.
GOL_SPAN_FN int run_bodies(const Rows &h, int k, int B, int cap) {
    const long long n = ((long long)h.lim - first_row(h, k)) / B + 1;
    return n < cap ? (int)n : cap;
}

}  // namespace span_detail

// The longest run of interior bodies of the band's main loop (the first of
// equally long ones).  A run ends at a torus wrap of either half, at the halo
// clamp, and at the band's first and last output rows.
GOL_SPAN_FN SkewSpan skew_interior_span(const SkewSpanIn &in) {
    using namespace span_detail;
    const int B = in.pair ? 6 : 3;
    const int S = in.eb - in.ab, D = in.D;
    const int k0 = skew_main_start(D, in.pair);
    SkewSpan none = {k0, k0};
    if (!in.enabled || in.counts || S <= 0 || S > 0x7FFFFFFF - 4 * D - 64) return none;
    // the bodies whose stores are all real: 0 <= k - 3 - 2 D and k - 4 - 2 D + B < S, within the loop
    if (in.half) {
        // the two halves' rows lie dr apart or, after one has wrapped, wrap - dr: byte offsets from one base
        const long long apart = in.wrap > 0 && in.wrap > in.dr ? in.wrap : in.dr;
        if (in.dr < 0 || apart * in.Ww * 4 >= 0x7FFFFFFFll - 64) return none;
    }
    const int kmain = skew_main_end(S, D, in.self);
    int lo = 2 * D + 3, hi = S + 2 * D + 4 - B;  // k in [lo, hi)
    if (hi > kmain) hi = kmain;
    // (and the rows a body stores are the group's before it, which the main loop must have run: its first body
    // stores nothing, the fill has stored its own groups' rows; only the pair rule at D = 16 starts past 2 D + 3)
    if (lo < k0 + 3) lo = k0 + 3;
    const int K0 = k0 + (lo - k0 + B - 1) / B * B;
    if (hi <= K0) return none;
    const int K1 = K0 + (hi - K0 + B - 1) / B * B;  // one past the last body that starts below hi
    // the rows a body loads, per half: first row (c + k) mod wrap, good iff <= min(wrap, rmax + 1) - B
    const int nh = in.half ? 2 : 1;
    Rows h[2];
    for (int i = 0; i < nh; ++i) {
        const long long c = (long long)in.ab + (i ? in.dr : 0) + in.off + 3;
        h[i].wrap = in.wrap > 0 ? (unsigned)in.wrap : 0u;
        h[i].cl = c;
        h[i].c = 0;
        if (in.wrap > 0) {
            const long long m = c % in.wrap;
            h[i].c = (unsigned)(m < 0 ? m + in.wrap : m);
        }
        const long long top = in.wrap > 0 && in.wrap < (long long)in.rmax + 1 ? in.wrap : (long long)in.rmax + 1;
        const long long lim = top - B;
        h[i].lim = lim < -1 ? -1 : (int)lim;
    }
    SkewSpan best = none;
    int k = K0;
    for (int run = 0; run < 8 && k < K1; ++run) {
        // the next body that is good for every half
        bool found = false;
        for (int step = 0; step < 8 && k < K1; ++step) {
            int skip = 0;
            for (int i = 0; i < nh; ++i) {
                const int s = skip_to_good(h[i], k, B);
                if (s < 0) return best;
                if (s > skip) skip = s;
            }
            if (skip == 0) {
                found = true;
                break;
            }
            if (skip >= K1 - k) return best;
            k += skip;
        }
        if (!found) return best;
        int n = (K1 - k) / B;
        for (int i = 0; i < nh; ++i) n = run_bodies(h[i], k, B, n);
        if (n * B > best.k_hi - best.k_lo) best = SkewSpan{k, k + n * B};
        k += n * B;
    }
    return best;
}

}  // namespace golk
