"""The fused turn + list kernel of the Life-like rules (K14), host side (no
GPU): rule_next_words of csrc/gol_rule_bits.h, the whole turn of one word from
three rows' words with their west / east neighbours aligned, on the emulated
v_bitop3 against the definition rule_def, cell by cell; and the two C-ABI
functions golhip_set_rule_flips / golhip_rule_flips in the header and the
library.  The stand-alone program also runs under AddressSanitizer and UBSan.
"""
import os
import re
import subprocess

import pytest

golhip = pytest.importorskip("golhip")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "game-of-life-distributed_amd", "csrc")

WORDS = r'''
#include <cstdio>
#include <cstdint>
#include "gol_rule_bits.h"
using namespace golk;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (uint32_t)((state * 0x2545F4914F6CDD1Dull) >> 32);
}
// words of every density: a B0 rule and the all-ones masks show on empty and full neighbourhoods
static uint32_t word(int kind) {
    switch (kind & 3) {
        case 0: return rnd();
        case 1: return rnd() & rnd() & rnd();
        case 2: return rnd() | rnd() | rnd();
    }
    return (rnd() & 1) ? 0u : ~0u;
}

struct Triple {
    uint32_t l[3], x[3], r[3];  // three rows: the word, its left and right neighbour words
    uint32_t w[3], e[3];        // aligned on the host: bit b = cell b - 1 / cell b + 1
};
static Triple triple(int n) {
    Triple t;
    for (int j = 0; j < 3; ++j) {
        t.l[j] = word(n >> (2 * j));
        t.x[j] = word(n >> (2 * j + 6));
        t.r[j] = word(n >> (2 * j + 12));
        t.w[j] = (t.x[j] << 1) | (t.l[j] >> 31);
        t.e[j] = (t.x[j] >> 1) | (t.r[j] << 31);
    }
    return t;
}
// the definition, cell by cell, from the 96 cells of each row
static uint32_t wanted(uint32_t birth, uint32_t survive, const Triple &t) {
    uint32_t out = 0;
    for (int b = 0; b < 32; ++b) {
        int sum9 = 0;
        for (int j = 0; j < 3; ++j)
            for (int d = -1; d <= 1; ++d) {
                const int p = 32 + b + d;  // position in (l, x, r)
                const uint32_t wd = p < 32 ? t.l[j] : p < 64 ? t.x[j] : t.r[j];
                sum9 += (wd >> (p & 31)) & 1u;
            }
        if (rule_def(birth, survive, sum9, (t.x[1] >> b) & 1u)) out |= 1u << b;
    }
    return out;
}

template <class Rule>
static long check(uint32_t birth, uint32_t survive, int triples) {
    const Rule rule(birth, survive);
    long bad = 0;
    for (int n = 0; n < triples; ++n) {
        const Triple t = triple(n * 2654435761u >> 8);
        const uint32_t got = rule_next_words<HostOps>(rule, t.w, t.x, t.e);
        if (got != wanted(birth, survive, t)) {
            if (!bad) std::printf("B%x S%x triple %d: %08x, wanted %08x\n", birth, survive, n, got, wanted(birth, survive, t));
            ++bad;
        }
    }
    return bad;
}

int main() {
    long bad = 0, rules = 0;
    // every static rule on its own instance, and on the dynamic policy
#define GOL_RULE_X(name, b, s)                    \
    bad += check<StaticRule<b, s>>(b, s, 4096);  \
    bad += check<DynRule>(b, s, 512);            \
    ++rules;
    GOL_STATIC_RULES(GOL_RULE_X)
#undef GOL_RULE_X
    if (rules != 7) return 2;
    // the extremes: empty and full masks, B0 alone, B0/S8
    const uint32_t ext[][2] = {{0, 0}, {0, kRuleMaskAll}, {kRuleMaskAll, 0}, {kRuleMaskAll, kRuleMaskAll},
                               {0x001, 0}, {0x001, 0x100}, {0x001, kRuleMaskAll}, {0x100, 0x001}};
    for (const auto &r : ext) bad += check<DynRule>(r[0], r[1], 2048);
    // 4096 seeded rules on the dynamic policy
    for (int i = 0; i < 4096; ++i) {
        const uint32_t birth = rnd() & kRuleMaskAll, survive = rnd() & kRuleMaskAll;
        bad += check<DynRule>(birth, survive, 48);
    }
    if (bad) return 1;
    std::puts("ok 4096 seeded rules");
    return 0;
}
'''

SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.mark.parametrize("flags", [(), SANITIZE], ids=["plain", "asan-ubsan"])
def test_rule_next_words(tmp_path, flags):
    """Every static rule on StaticRule and DynRule, the extremes (birth /
    survive 0 and 0x1FF, B0) and 4096 seeded rules on DynRule: random word
    triples, neighbours aligned on the host, every cell against rule_def."""
    src = tmp_path / "words.cpp"
    src.write_text(WORDS)
    exe = tmp_path / "words"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, str(src), "-o", str(exe)],
                   check=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip() == "ok 4096 seeded rules", (p.returncode, p.stdout, p.stderr[-2000:])


def test_header_and_library_have_the_two_functions():
    header = open(os.path.join(ROOT, "include", "golhip.h")).read()
    assert re.search(r"^int golhip_set_rule_flips\(golhip_t h, int32_t mode\);", header, re.M)
    assert re.search(r"^int golhip_rule_flips\(golhip_t h, int32_t \*mode\);", header, re.M)
    run = open(os.path.join(ROOT, "include", "golrun.h")).read()
    assert re.search(r"^#define GOLRUN_FLAG_RULE_FLIPS \(1u << 6\)", run, re.M)
    lib = golhip.load()
    for name in ("golhip_set_rule_flips", "golhip_rule_flips"):
        assert hasattr(lib, name), name
    import ctypes
    m = ctypes.c_int32(7)
    assert lib.golhip_set_rule_flips(None, 1) == -1 and lib.golhip_rule_flips(None, ctypes.byref(m)) == -1
    assert golhip.FLAG_RULE_FLIPS == 0x40
    # not an option key: golhip_build_info()'s lists stay as they are
    assert "rule_flips" not in lib.golhip_build_info().decode()
