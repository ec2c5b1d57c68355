// gol_rule_bits.h — the Life-like (outer-totalistic) rule of K11 (gol_rule.hip):
// a rule is two 9-bit masks, bit n of `birth`: a dead cell with n alive
// neighbours (of 8, centre excluded) comes alive; bit n of `survive`: an alive
// cell with n stays alive.  Conway is birth 0x008, survive 0x00C.
//
// Plain C++ on purpose (no HIP header): the host tests compile this file with
// g++ and check both policies against the definition on an emulated v_bitop3
// (tests/test_rule_cpu.py); the kernel instantiates the same templates on the
// instruction itself.
//
// The circuit.  K1's stage forms, per cell, u = u0 + 2 u1 (the sum of the
// three rows' h0 bits) and v = v0 + 2 v1 (of their h1 bits), centre included:
//   sum9 = u0 + 2 T,  T = u1 + v0 + 2 v1 in 0..4  (sum9 in 0..9)
// T goes to three bits in three LUTs (rule_t):
//   t0 = u1 ^ v0,  t1 = v1 ^ (u1 & v0),  t2 = v1 & u1 & v0
// t2 is set only for sum9 in {8, 9}, where t0 = t1 = 0.  next is a function of
// (u0, t0, t1, t2, c): survive[sum9 - 1] for an alive centre, birth[sum9] for
// a dead one.  Of the 20 (sum9, c) pairs two cannot occur (alive with sum9 0,
// dead with sum9 9).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GOL_RULE_HD __host__ __device__ __forceinline__
#else
#define GOL_RULE_HD inline
#endif

namespace golk {

constexpr uint32_t kRuleMaskAll = 0x1FF;
constexpr uint32_t kConwayBirth = 0x008, kConwaySurvive = 0x00C;

// The definition: the next state of a cell whose 3x3 block holds sum9 alive
// cells, itself (c) included.
constexpr bool rule_def(uint32_t birth, uint32_t survive, int sum9, int c) {
    return c ? (sum9 >= 1 && ((survive >> (sum9 - 1)) & 1u)) : (sum9 <= 8 && ((birth >> sum9) & 1u));
}

// v_bitop3_b32 truth tables in gol_bits.h's order (tt3): operands (a, b, c) ->
// bit a*4 + b*2 + c of the immediate.
constexpr unsigned kRuleMux = 0xCA;   // a ? b : c
constexpr unsigned kRuleT0 = 0x3C;    // a ^ b                (u1, v0, v0)
constexpr unsigned kRuleT1 = 0x6A;    // c ^ (a & b)          (u1, v0, v1)
constexpr unsigned kRuleT2 = 0x80;    // a & b & c            (u1, v0, v1)

// The static policy's three rule-dependent immediates:
//   gA(u0, t0, c): next where t1 = 1 (sum9 = u0 + 2 t0 + 4)
//   gB(u0, t0, c): next where t1 = 0 and t2 = 0 (sum9 = u0 + 2 t0)
//   h (u0, c, c) : next where t2 = 1 (sum9 = 8 + u0); the centre repeats, so
//                  only the rows b == c of the table are ever read
struct RuleLuts {
    unsigned gA, gB, h;
};
constexpr RuleLuts rule_luts(uint32_t birth, uint32_t survive) {
    RuleLuts r{0, 0, 0};
    for (int i = 0; i < 8; ++i) {
        const int a = (i >> 2) & 1, b = (i >> 1) & 1, c = i & 1;
        if (rule_def(birth, survive, a + 2 * b + 4, c)) r.gA |= 1u << i;
        if (rule_def(birth, survive, a + 2 * b, c)) r.gB |= 1u << i;
        if (rule_def(birth, survive, 8 + a, b)) r.h |= 1u << i;
    }
    return r;
}

// v_bitop3_b32 on the host, 32 cells at once (immediate at run time).
inline uint32_t bitop3_emul(uint32_t a, uint32_t b, uint32_t c, unsigned imm) {
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i)
        if ((imm >> i) & 1u) r |= ((i & 4) ? a : ~a) & ((i & 2) ? b : ~b) & ((i & 1) ? c : ~c);
    return r;
}
struct HostOps {
    template <unsigned IMM>
    static uint32_t op(uint32_t a, uint32_t b, uint32_t c) {
        return bitop3_emul(a, b, c, IMM);
    }
};

// T's three bits from the column sums (three LUTs).
template <class Ops>
GOL_RULE_HD void rule_t(uint32_t u1, uint32_t v0, uint32_t v1, uint32_t &t0, uint32_t &t1, uint32_t &t2) {
    t0 = Ops::template op<kRuleT0>(u1, v0, v0);
    t1 = Ops::template op<kRuleT1>(u1, v0, v1);
    t2 = Ops::template op<kRuleT2>(u1, v0, v1);
}

// Static policy: five LUTs with compile-time immediates.
template <uint32_t B, uint32_t S>
struct StaticRule {
    static_assert(B <= kRuleMaskAll && S <= kRuleMaskAll, "rule masks are 9 bits");
    static constexpr bool kDynamic = false;
    GOL_RULE_HD StaticRule(uint32_t, uint32_t) {}
    template <class Ops>
    GOL_RULE_HD uint32_t next(uint32_t u0, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t c) const {
        constexpr RuleLuts L = rule_luts(B, S);
        const uint32_t ga = Ops::template op<L.gA>(u0, t0, c);
        const uint32_t gb = Ops::template op<L.gB>(u0, t0, c);
        const uint32_t m = Ops::template op<kRuleMux>(t1, ga, gb);
        const uint32_t hh = Ops::template op<L.h>(u0, c, c);
        return Ops::template op<kRuleMux>(t2, hh, m);
    }
};

// Dynamic policy: any rule from two wave-uniform masks.  Each (sum9, c) pair's
// bit becomes a word that is all ones or zero; per sum9 a mux on the centre
// picks survive[sum9 - 1] or birth[sum9] (sum9 0 and 9 need none: the other
// centre cannot occur), then a mux tree on u0, t0, t1, t2 picks the word of
// this cell's sum9: 8 + 5 + 2 + 1 + 1 = 17 LUTs.
struct DynRule {
    static constexpr bool kDynamic = true;
    uint32_t bm[9], sm[9];
    GOL_RULE_HD DynRule(uint32_t birth, uint32_t survive) {
        for (int n = 0; n < 9; ++n) {
            bm[n] = 0u - ((birth >> n) & 1u);
            sm[n] = 0u - ((survive >> n) & 1u);
        }
    }
    template <class Ops>
    GOL_RULE_HD uint32_t next(uint32_t u0, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t c) const {
        uint32_t l[10];
        l[0] = bm[0];
        l[9] = sm[8];
        for (int s = 1; s <= 8; ++s) l[s] = Ops::template op<kRuleMux>(c, sm[s - 1], bm[s]);
        const uint32_t p0 = Ops::template op<kRuleMux>(u0, l[1], l[0]);  // T = 0
        const uint32_t p1 = Ops::template op<kRuleMux>(u0, l[3], l[2]);  // T = 1
        const uint32_t p2 = Ops::template op<kRuleMux>(u0, l[5], l[4]);  // T = 2
        const uint32_t p3 = Ops::template op<kRuleMux>(u0, l[7], l[6]);  // T = 3
        const uint32_t p4 = Ops::template op<kRuleMux>(u0, l[9], l[8]);  // T = 4
        const uint32_t q0 = Ops::template op<kRuleMux>(t0, p1, p0);
        const uint32_t q1 = Ops::template op<kRuleMux>(t0, p3, p2);
        const uint32_t m = Ops::template op<kRuleMux>(t1, q1, q0);
        return Ops::template op<kRuleMux>(t2, p4, m);
    }
};

// The whole turn of one word from three rows' words x with their west (w, bit
// b = cell b - 1) and east (e, bit b = cell b + 1) neighbours already aligned,
// as the fused turn + list kernel K14 has them (gol_rule_flip.hip): the row
// sums h0 + 2 h1 with K1's two LUTs, the column sums u and v, rule_t and the
// policy's next with the middle row's word as the centre.  6 + 4 + 3 LUTs and
// the policy's 5 (StaticRule: 18 a word) or 17 (DynRule: 30).
constexpr unsigned kRuleXor3 = 0x96;  // a ^ b ^ c
constexpr unsigned kRuleMaj = 0xE8;   // a + b + c >= 2
template <class Ops, class Rule>
GOL_RULE_HD uint32_t rule_next_words(const Rule &rule, const uint32_t (&w)[3], const uint32_t (&x)[3],
                                     const uint32_t (&e)[3]) {
    uint32_t h0[3], h1[3];
    for (int j = 0; j < 3; ++j) {
        h0[j] = Ops::template op<kRuleXor3>(w[j], x[j], e[j]);
        h1[j] = Ops::template op<kRuleMaj>(w[j], x[j], e[j]);
    }
    const uint32_t u0 = Ops::template op<kRuleXor3>(h0[0], h0[1], h0[2]);
    const uint32_t u1 = Ops::template op<kRuleMaj>(h0[0], h0[1], h0[2]);
    const uint32_t v0 = Ops::template op<kRuleXor3>(h1[0], h1[1], h1[2]);
    const uint32_t v1 = Ops::template op<kRuleMaj>(h1[0], h1[1], h1[2]);
    uint32_t t0, t1, t2;
    rule_t<Ops>(u1, v0, v1, t0, t1, t2);
    return rule.template next<Ops>(u0, t0, t1, t2, x[1]);
}

// The rules with a static instantiation (launch_step_rule picks the dynamic
// policy for every other): name, birth, survive.
#define GOL_STATIC_RULES(X)            \
    X(Conway, 0x008, 0x00C)            \
    X(HighLife, 0x048, 0x00C)          \
    X(DayAndNight, 0x1C8, 0x1D8)       \
    X(Seeds, 0x004, 0x000)             \
    X(LifeWithoutDeath, 0x008, 0x1FF)  \
    X(Replicator, 0x0AA, 0x0AA)        \
    X(TwoByTwo, 0x048, 0x026)

constexpr bool rule_is_static(uint32_t birth, uint32_t survive) {
#define GOL_RULE_X(name, b, s) \
    if (birth == b && survive == s) return true;
    GOL_STATIC_RULES(GOL_RULE_X)
#undef GOL_RULE_X
    return false;
}

}  // namespace golk
