// gol_rule_plane.hip — K15: K11 (gol_rule.hip) on a bounded plane.  The same
// 64-lane tiles, one canonical word a lane, lanes 1..62 stored, the same
// D-stage register pipeline of h0 / h1 / cc for three rows a stage with the
// groups of three rows skewed by a stage, masked stores after a group and one
// atomicAdd a wave; the rule is a policy of gol_rule_bits.h.
//
// The one difference: at every turn of the launch every cell outside
// [0, W) x [0, H) is dead (gol_plane_mask.h).
//   Columns: a per-lane mask, computed once a wave, on the loaded word and on
//   the word leaving every stage.  A lane whose word index is outside [0, Ww)
//   has mask 0 and loads a clamped, valid word.  So cell W - 1 finds a dead
//   cell to its east and cell 0 one to its west at any width: there is no row
//   seam, and any width runs at any depth.
//   Rows: the launch carries the board row of the frame's row 0 and H.  A row
//   outside [0, H) loads as zero and is forced to zero as it leaves each stage
//   (wave-uniform), so what the row map fetches for it (the torus wrap of a
//   whole board, the ring-copied halo of a strip) does not matter.
// Both masks go into one three-input AND a word-turn (the row's as a scalar).
#include <climits>

#include "gol_bits.h"
#include "gol_plane_mask.h"
#include "gol_rule_bits.h"
#include "gol_rule_plane.h"

namespace golk {

namespace {

struct PlaneOps {
    template <unsigned IMM>
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b, uint32_t c) {
        return bop<IMM>(a, b, c);
    }
};

constexpr unsigned kAnd3 = tt3([](int a, int b, int c) { return a && b && c; });

// What bounds a wave's words: the lane's columns and the board's rows.
struct Bounds {
    uint32_t cmask;  // plane_col_mask of this lane's word
    int H;
    // the word x of board row `brow` with everything outside the board dead
    __device__ __forceinline__ uint32_t clip(uint32_t x, int brow) const {
        const uint32_t rmask = plane_row_inside(brow, H) ? ~0u : 0u;  // wave-uniform
        return bop<kAnd3>(x, cmask, rmask);
    }
};

// One stage (turn t) for the row entering with role R (input index % 3) as
// board row `brow`: K11's rule_stage, the word leaving clipped to the board.
template <int D, int R, class Rule>
__device__ __forceinline__ void plane_stage(int t, uint32_t &x, int brow, uint32_t (&h0)[3][D], uint32_t (&h1)[3][D],
                                            uint32_t (&cc)[3][D], const Rule &rule, const Bounds &bd) {
    constexpr int N = R;            // slot of the row entering now
    constexpr int C = (R + 2) % 3;  // previous row (the one emitted)
    constexpr int P = (R + 1) % 3;  // the row before it
    const uint32_t l = from_left_lane(x);
    const uint32_t r = from_right_lane(x);
    const uint32_t west = __builtin_amdgcn_alignbit(x, l, 31);  // bit b = cell b - 1
    const uint32_t east = __builtin_amdgcn_alignbit(r, x, 1);   // bit b = cell b + 1
    h0[N][t] = bop<kXor3>(west, x, east);
    h1[N][t] = bop<kMaj>(west, x, east);
    const uint32_t u0 = bop<kXor3>(h0[P][t], h0[C][t], h0[N][t]);
    const uint32_t u1 = bop<kMaj>(h0[P][t], h0[C][t], h0[N][t]);
    const uint32_t v0 = bop<kXor3>(h1[P][t], h1[C][t], h1[N][t]);
    const uint32_t v1 = bop<kMaj>(h1[P][t], h1[C][t], h1[N][t]);
    uint32_t t0, t1, t2;
    rule_t<PlaneOps>(u1, v0, v1, t0, t1, t2);
    const uint32_t nx = rule.template next<PlaneOps>(u0, t0, t1, t2, cc[C][t]);
    cc[N][t] = x;
    x = bd.clip(nx, plane_stage_row(brow, t));
}

// Three consecutive input rows (board rows brow, brow + 1, brow + 2) through
// the D stages, skewed by one stage.
template <int D, class Rule>
__device__ __forceinline__ void plane_group(uint32_t &x0, uint32_t &x1, uint32_t &x2, int brow, uint32_t (&h0)[3][D],
                                            uint32_t (&h1)[3][D], uint32_t (&cc)[3][D], const Rule &rule,
                                            const Bounds &bd) {
#pragma unroll
    for (int s = 0; s < D + 2; ++s) {
        if (s < D) plane_stage<D, 0>(s, x0, brow, h0, h1, cc, rule, bd);
        if (s >= 1 && s - 1 < D) plane_stage<D, 1>(s - 1, x1, brow + 1, h0, h1, cc, rule, bd);
        if (s >= 2) plane_stage<D, 2>(s - 2, x2, brow + 2, h0, h1, cc, rule, bd);
    }
}

}  // namespace

// brow0: the board row of the frame's row 0 (negative for a deep-halo launch
// of the board's first strip); H: the board's rows.
template <int D, class Rule>
__global__ __launch_bounds__(256) void gol_plane_kernel(StepArgs a, uint32_t birth, uint32_t survive, int brow0, int H) {
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
    const int wi = tile * kTileValid + lane - 1;  // this lane's word of the row; outside [0, Ww): dead
    const int col = plane_col_clamp(wi, Ww);
    const bool keep = lane >= 1 && lane <= kTileValid && wi < Ww;
    const Rule rule(birth, survive);
    Bounds bd;
    bd.cmask = plane_col_mask(wi, a.W, Ww);
    bd.H = H;

    // input row cursor (wave-uniform), as K11's, and the board row it stands for
    int r = r0 - D + a.in.off;
    const int wrap = a.in.wrap > 0 ? a.in.wrap : INT_MAX;
    if (a.in.wrap > 0) {
        r %= a.in.wrap;
        if (r < 0) r += a.in.wrap;
    }
    int brow = brow0 + r0 - D;
    auto load_next = [&]() -> uint32_t {
        const uint32_t *row = a.src + (size_t)(a.in.base + min(r, a.in.rmax)) * Ww;
        const uint32_t v = bd.clip(row[col], brow);
        r = (r + 1 == wrap) ? 0 : r + 1;
        ++brow;
        return v;
    };

    uint32_t *const out0 = a.dst + (size_t)(a.dst_base + r0) * Ww + col;
    const int clo = a.count_lo - r0, chi = a.count_hi - r0;
    uint32_t cnt = 0;
    auto emit = [&](uint32_t y, int out_idx) {
        const bool ok = keep && (unsigned)out_idx < (unsigned)rows_here;
        if (ok) out0[(size_t)out_idx * Ww] = y;
        cnt += (ok && out_idx >= clo && out_idx < chi) ? __builtin_popcount(y) : 0u;
    };

    uint32_t h0[3][D], h1[3][D], cc[3][D];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int t = 0; t < D; ++t) h0[s][t] = h1[s][t] = cc[s][t] = 0u;

    // input index i is frame row r0 - D + i, board row brow0 + r0 - D + i; the
    // row leaving stage D - 1 with it is output row i - 2 D.  The next group's
    // rows are loaded ahead of the group.
    uint32_t x0 = load_next(), x1 = load_next(), x2 = load_next();
    for (int oi = -2 * D; oi < rows_here; oi += 3) {
        const uint32_t n0 = load_next(), n1 = load_next(), n2 = load_next();
        plane_group<D>(x0, x1, x2, brow0 + r0 + oi + D, h0, h1, cc, rule, bd);
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

// f(kernel) for the instance of (depth, rule, policy); hipErrorInvalidValue if there is none.
template <class Rule, typename F>
hipError_t dispatch_depth(int depth, F &&f) {
    switch (depth) {
        case 1: return f(gol_plane_kernel<1, Rule>);
        case 2: return f(gol_plane_kernel<2, Rule>);
        case 4: return f(gol_plane_kernel<4, Rule>);
        case 6: return f(gol_plane_kernel<6, Rule>);
        case 8: return f(gol_plane_kernel<8, Rule>);
        case 12: return f(gol_plane_kernel<12, Rule>);
        case 16: return f(gol_plane_kernel<16, Rule>);
    }
    return hipErrorInvalidValue;
}

template <typename F>
hipError_t dispatch_rule(int depth, uint32_t birth, uint32_t survive, bool dyn, F &&f) {
    if (birth > kRuleMaskAll || survive > kRuleMaskAll) return hipErrorInvalidValue;
    if (!dyn) {
#define GOL_RULE_X(name, b, s) \
    if (birth == b && survive == s) return dispatch_depth<StaticRule<b, s>>(depth, f);
        GOL_STATIC_RULES(GOL_RULE_X)
#undef GOL_RULE_X
    }
    return dispatch_depth<DynRule>(depth, f);
}

}  // namespace

int plane_wave_slots_per_cu(int depth, uint32_t birth, uint32_t survive, bool dyn) {
    int b = 0;
    const hipError_t e = dispatch_rule(depth, birth, survive, dyn, [&](auto kern) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kern, 256, 0);
    });
    return 4 * ((e == hipSuccess && b > 0) ? b : 1);
}

hipError_t launch_step_plane(const StepArgs &a, int depth, uint32_t birth, uint32_t survive, int brow0, int H,
                             hipStream_t s, bool dyn) {
    if (a.rows_out < 1 || a.Ww < 1 || a.rows_per_wave < 1 || a.Ww != (a.W + 31) / 32 || H < 1)
        return hipErrorInvalidValue;
    const int64_t strips = ((int64_t)a.rows_out + a.rows_per_wave - 1) / a.rows_per_wave;
    const int64_t waves = strips * ((a.Ww + kTileValid - 1) / kTileValid);
    if ((waves + 3) / 4 > INT_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    return dispatch_rule(depth, birth, survive, dyn, [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, block, 0, s, a, birth, survive, brow0, H);
        return hipGetLastError();
    });
}

}  // namespace golk
