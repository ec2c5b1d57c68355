// gol_rule_flip.hip — K14: one turn of any Life-like rule B.../S... fused with
// its CellFlipped list.  The kernel is K5's per-launch body (gol_flip_turn.h:
// block of 1024 canonical words, CONTIG and strided forms, DPP column
// neighbours, packed block scan, co-resident prefix or ticket + look-back, LDS
// staging, copy blocks, the ctl[0] stop, the alive count) with the rule as a
// policy (gol_rule_bits.h), as K11 made the step kernel's rule one:
// rule_next_words on the instruction itself, 18 LUTs a word (StaticRule) or
// 30 (DynRule) against K5's 13.  No resident form (K5r stays Conway's).
//
// A B0 rule raises every bit the neighbourhood of which is empty: the padding
// and ghost bits of a row's last word (W % 32 != 0) and whole words in lanes
// kept active past the board's end.  The body clears the former after the
// rule (seam_clear_pad) and masks the latter out of flips, count and stores.
#include "gol_bits.h"
#include "gol_flip_turn.h"
#include "gol_rule_bits.h"
#include "gol_rule_flip.h"

namespace golk {

static_assert(kRuleXor3 == kXor3 && kRuleMaj == kMaj, "gol_rule_bits.h keeps tt3's table order");

namespace {

struct DevOps {
    template <unsigned IMM>
    static __device__ __forceinline__ uint32_t op(uint32_t a, uint32_t b, uint32_t c) {
        return bop<IMM>(a, b, c);
    }
};

// The body's rule functor over a policy.
template <class Rule>
struct FtLifeLike {
    const Rule rule;
    __device__ __forceinline__ FtLifeLike(uint32_t birth, uint32_t survive) : rule(birth, survive) {}
    __device__ __forceinline__ uint32_t operator()(const uint32_t (&w)[3], const uint32_t (&x)[3],
                                                   const uint32_t (&e)[3]) const {
        return rule_next_words<DevOps>(rule, w, x, e);
    }
};

}  // namespace

template <bool CONTIG, bool ODD, class Rule>
__global__ __launch_bounds__(256) void gol_rule_flip_turn_kernel(RuleFlipTurnArgs r) {
    flip_turn_launch_block<CONTIG, ODD>(r.turn, FtLifeLike<Rule>(r.birth, r.survive));
}

namespace {

// f(kernel) for the instance of (contig, odd, rule, policy).
template <class Rule, typename F>
hipError_t dispatch_shape(bool contig, bool odd, F &&f) {
    hipError_t e = hipErrorUnknown;
    ft_dispatch(contig, odd, [&](auto c, auto o) {
        e = f(gol_rule_flip_turn_kernel<decltype(c)::value, decltype(o)::value, Rule>);
    });
    return e;
}

template <typename F>
hipError_t dispatch_rule_flip(bool contig, bool odd, uint32_t birth, uint32_t survive, bool dyn, F &&f) {
    if (birth > kRuleMaskAll || survive > kRuleMaskAll) return hipErrorInvalidValue;
    if (!dyn) {
#define GOL_RULE_X(name, b, s) \
    if (birth == b && survive == s) return dispatch_shape<StaticRule<b, s>>(contig, odd, f);
        GOL_STATIC_RULES(GOL_RULE_X)
#undef GOL_RULE_X
    }
    return dispatch_shape<DynRule>(contig, odd, f);
}

}  // namespace

int rule_flip_turn_blocks_per_cu(bool contig, bool odd, uint32_t birth, uint32_t survive, bool dyn) {
    int b = 0;
    const hipError_t e = dispatch_rule_flip(contig, odd, birth, survive, dyn, [&](auto kern) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kern, kFtThreads, 0);
    });
    return e == hipSuccess ? b : 0;
}

hipError_t launch_rule_flip_turn(const FlipTurnArgs &a, uint32_t birth, uint32_t survive, bool dyn, hipStream_t s) {
    const int64_t grid = (int64_t)a.ncompute + (a.cp_run ? a.cp_blocks : 0);
    if (grid == 0) return hipSuccess;
    const RuleFlipTurnArgs r{a, birth, survive};
    return dispatch_rule_flip(a.Ww % 4 == 0, a.W % 32 != 0, birth, survive, dyn, [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kFtThreads), 0, s, r);
        return hipGetLastError();
    });
}

}  // namespace golk
