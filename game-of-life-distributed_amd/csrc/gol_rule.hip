// gol_rule.hip — K11: the temporally blocked step kernel for any Life-like
// (outer-totalistic) rule B.../S... (gol_rule_bits.h).
//
// The shape is K1's (gol_kernels.hip): one wavefront is a tile of 64 lanes,
// one canonical word a lane, lanes 1..62 stored; it streams the rows of its
// band top to bottom through a D-stage register pipeline that keeps the row
// sums h0 / h1 and the centre words cc of three rows a stage (9 D VGPRs), the
// three rows of a group skewed by one stage so each stage's VALU -> DPP chain
// has two independent ones beside it.  The rest is plain: masked stores right
// after a group, no claim counters, dummy rows, deferred or buffer stores, no
// fill skip, no skewed stacks, resident forms, pairs or quads.
//
// Per stage and word: 2 DPP + 2 alignbit (half rate), 2 LUTs row sum, 4 LUTs
// column sums, 3 LUTs T's bits, then the rule: 5 LUTs (StaticRule) or 17
// (DynRule).  W % 32 != 0 (depth 1 only): a row's last word takes the first
// word's low bits above its own, so cell W - 1 finds cell 0 to its east in the
// word, and the first word's west edge bit comes from bit (W - 1) % 32 of the
// last word; the bits of columns >= W are cleared at the store.
#include <climits>

#include "gol_bits.h"
#include "gol_rule.h"
#include "gol_rule_bits.h"

namespace golk {

static_assert(kRuleT0 == kXor2 && kRuleT2 == tt3([](int a, int b, int c) { return a && b && c; }) &&
                  kRuleT1 == tt3([](int a, int b, int c) { return (c ^ (a & b)) != 0; }) &&
                  kRuleMux == tt3([](int a, int b, int c) { return a ? b : c; }),
              "gol_rule_bits.h keeps tt3's table order");

namespace {

struct DevOps {
    template <unsigned IMM>
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b, uint32_t c) {
        return bop<IMM>(a, b, c);
    }
};

// The row seam of a width that is no multiple of 32 (wave-uniform but `first`).
struct Seam {
    bool first;    // this lane's word is word 0 of the row
    int west_shl;  // 32 - W % 32: brings the last word's bit (W - 1) % 32 to bit 31
};

// One stage (turn t) for the row entering with role R (input index % 3): K1's
// stage<> with the rule as a policy.
template <int D, int R, bool ODD, class Rule>
__device__ __forceinline__ void rule_stage(int t, uint32_t &x, uint32_t (&h0)[3][D], uint32_t (&h1)[3][D],
                                           uint32_t (&cc)[3][D], const Rule &rule, const Seam &sm) {
    constexpr int N = R;            // slot of the row entering now
    constexpr int C = (R + 2) % 3;  // previous row (the one emitted)
    constexpr int P = (R + 1) % 3;  // the row before it
    uint32_t l = from_left_lane(x);
    const uint32_t r = from_right_lane(x);
    if constexpr (ODD) l = sm.first ? l << sm.west_shl : l;
    const uint32_t west = __builtin_amdgcn_alignbit(x, l, 31);  // bit b = cell b - 1
    const uint32_t east = __builtin_amdgcn_alignbit(r, x, 1);   // bit b = cell b + 1
    h0[N][t] = bop<kXor3>(west, x, east);
    h1[N][t] = bop<kMaj>(west, x, east);
    const uint32_t u0 = bop<kXor3>(h0[P][t], h0[C][t], h0[N][t]);
    const uint32_t u1 = bop<kMaj>(h0[P][t], h0[C][t], h0[N][t]);
    const uint32_t v0 = bop<kXor3>(h1[P][t], h1[C][t], h1[N][t]);
    const uint32_t v1 = bop<kMaj>(h1[P][t], h1[C][t], h1[N][t]);
    uint32_t t0, t1, t2;
    rule_t<DevOps>(u1, v0, v1, t0, t1, t2);
    const uint32_t nx = rule.template next<DevOps>(u0, t0, t1, t2, cc[C][t]);
    cc[N][t] = x;
    x = nx;
}

// Three consecutive input rows through the D stages, skewed by one stage.
template <int D, bool ODD, class Rule>
__device__ __forceinline__ void rule_group(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t (&h0)[3][D],
                                           uint32_t (&h1)[3][D], uint32_t (&cc)[3][D], const Rule &rule,
                                           const Seam &sm) {
#pragma unroll
    for (int s = 0; s < D + 2; ++s) {
        if (s < D) rule_stage<D, 0, ODD>(s, x0, h0, h1, cc, rule, sm);
        if (s >= 1 && s - 1 < D) rule_stage<D, 1, ODD>(s - 1, x1, h0, h1, cc, rule, sm);
        if (s >= 2) rule_stage<D, 2, ODD>(s - 2, x2, h0, h1, cc, rule, sm);
    }
}

}  // namespace

template <int D, bool ODD, class Rule>
__global__ __launch_bounds__(256) void gol_rule_kernel(StepArgs a, uint32_t birth, uint32_t survive) {
    static_assert(!ODD || D == 1, "the row seam is closed for one turn only");
    const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int Ww = a.Ww;
    const int tiles_x = (Ww + kTileValid - 1) / kTileValid;
    const int S = a.rows_per_wave;
    const int strip = wave / tiles_x;
    const int tile = wave - strip * tiles_x;
    const int r0 = strip * S;
    if (r0 >= a.rows_out) return;  // wave-uniform
    const int rows_here = min(S, a.rows_out - r0);
    const int t0 = tile * kTileValid;
    int col = (t0 + lane - 1) % Ww;
    if (col < 0) col += Ww;
    const bool keep = lane >= 1 && lane <= kTileValid && t0 + lane - 1 < Ww;
    const Rule rule(birth, survive);

    const int tb = a.W & 31;  // ODD: cells of a row's last word
    const bool last = ODD && col == Ww - 1;
    const uint32_t tail = ODD ? (1u << tb) - 1u : ~0u;
    Seam sm;
    sm.first = ODD && col == 0;
    sm.west_shl = 32 - tb;

    // input row cursor (wave-uniform), as K1's
    int r = r0 - D + a.in.off;
    const int wrap = a.in.wrap > 0 ? a.in.wrap : INT_MAX;
    if (a.in.wrap > 0) {
        r %= a.in.wrap;
        if (r < 0) r += a.in.wrap;
    }
    auto load_next = [&]() -> uint32_t {
        const uint32_t *row = a.src + (size_t)(a.in.base + min(r, a.in.rmax)) * Ww;
        uint32_t v = row[col];
        if constexpr (ODD) {
            const uint32_t w0 = row[0];
            v = last ? (v & tail) | (w0 << tb) : v;
        }
        r = (r + 1 == wrap) ? 0 : r + 1;
        return v;
    };

    uint32_t *const out0 = a.dst + (size_t)(a.dst_base + r0) * Ww + col;
    const int clo = a.count_lo - r0, chi = a.count_hi - r0;
    uint32_t cnt = 0;
    auto emit = [&](uint32_t y, int out_idx) {
        if constexpr (ODD) y = last ? y & tail : y;
        const bool ok = keep && (unsigned)out_idx < (unsigned)rows_here;
        if (ok) out0[(size_t)out_idx * Ww] = y;
        cnt += (ok && out_idx >= clo && out_idx < chi) ? __builtin_popcount(y) : 0u;
    };

    uint32_t h0[3][D], h1[3][D], cc[3][D];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int t = 0; t < D; ++t) h0[s][t] = h1[s][t] = cc[s][t] = 0u;

    // input index i is row r0 - D + i; the row leaving stage D - 1 with it is
    // output row i - 2 D.  The next group's rows are loaded ahead of the group.
    uint32_t x0 = load_next(), x1 = load_next(), x2 = load_next();
    for (int oi = -2 * D; oi < rows_here; oi += 3) {
        const uint32_t n0 = load_next(), n1 = load_next(), n2 = load_next();
        rule_group<D, ODD>(x0, x1, x2, h0, h1, cc, rule, sm);
        emit(x0, oi);
        emit(x1, oi + 1);
        emit(x2, oi + 2);
        x0 = n0;
        x1 = n1;
        x2 = n2;
    }
    if (a.alive) {
        const uint32_t tot = wave_sum_u32(cnt);
        if (lane == 0 && tot) atomicAdd(a.alive, (unsigned long long)tot);
    }
}

namespace {

// f(kernel) for the instance of (depth, odd, rule, policy); hipErrorInvalidValue if there is none.
template <class Rule, typename F>
hipError_t dispatch_depth(int depth, bool odd, F &&f) {
    if (odd) return depth == 1 ? f(gol_rule_kernel<1, true, Rule>) : hipErrorInvalidValue;
    switch (depth) {
        case 1: return f(gol_rule_kernel<1, false, Rule>);
        case 2: return f(gol_rule_kernel<2, false, Rule>);
        case 4: return f(gol_rule_kernel<4, false, Rule>);
        case 6: return f(gol_rule_kernel<6, false, Rule>);
        case 8: return f(gol_rule_kernel<8, false, Rule>);
        case 12: return f(gol_rule_kernel<12, false, Rule>);
        case 16: return f(gol_rule_kernel<16, false, Rule>);
    }
    return hipErrorInvalidValue;
}

template <typename F>
hipError_t dispatch_rule(int depth, bool odd, uint32_t birth, uint32_t survive, bool dyn, F &&f) {
    if (birth > kRuleMaskAll || survive > kRuleMaskAll) return hipErrorInvalidValue;
    if (!dyn) {
#define GOL_RULE_X(name, b, s) \
    if (birth == b && survive == s) return dispatch_depth<StaticRule<b, s>>(depth, odd, f);
        GOL_STATIC_RULES(GOL_RULE_X)
#undef GOL_RULE_X
    }
    return dispatch_depth<DynRule>(depth, odd, f);
}

}  // namespace

int rule_wave_slots_per_cu(int depth, int W, uint32_t birth, uint32_t survive, bool dyn) {
    int b = 0;
    const hipError_t e = dispatch_rule(depth, W % 32 != 0, birth, survive, dyn, [&](auto kern) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kern, 256, 0);
    });
    return 4 * ((e == hipSuccess && b > 0) ? b : 1);
}

hipError_t launch_step_rule(const StepArgs &a, int depth, uint32_t birth, uint32_t survive, hipStream_t s, bool dyn) {
    if (a.rows_out < 1 || a.Ww < 1 || a.rows_per_wave < 1 || a.Ww != (a.W + 31) / 32) return hipErrorInvalidValue;
    const int64_t strips = ((int64_t)a.rows_out + a.rows_per_wave - 1) / a.rows_per_wave;
    const int64_t waves = strips * ((a.Ww + kTileValid - 1) / kTileValid);
    if ((waves + 3) / 4 > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    return dispatch_rule(depth, a.W % 32 != 0, birth, survive, dyn, [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, a, birth, survive);
        return hipGetLastError();
    });
}

}  // namespace golk
