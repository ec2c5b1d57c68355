"""The row seam of the fused turn + list kernel without a GPU:
the three word operations of csrc/gol_flip_seam.h that let K5 step a board
whose width is no multiple of 32 on the canonical layout.

The header is compiled with a stand-alone main under
g++ -fsanitize=address,undefined (as test_pad_plan_cpu.py compiles
gol_pad_plan.h; nothing is loaded into Python).  The main steps boards word by
word the way the kernel does: per word the three input rows, the left and right
neighbour words of the row (wrapping to the row's last / first word), the
seam helpers on the row's first and last word, one turn of the rule, the last
word's padding cleared.  Every board after each of three turns must equal
oracle.step_np, padding bits zero.  In half the cases the input's padding bits
are garbage and the loader's clearing (the same helper) is applied first.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import pack_bits, step_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "game-of-life-distributed_amd", "csrc")

WIDTHS = [1, 2, 3, 16, 17, 31, 33, 63, 65, 95, 100, 127, 129, 1000]
HEIGHTS = [1, 2, 3, 5]
TURNS = 3

MAIN = r'''
#include <cstdio>
#include <vector>
#include "gol_flip_seam.h"
// stdin: cases of "W H turns clear" then H * ceil(W / 32) words; stdout per
// case and turn one line of H * Ww words.  W % 32 != 0.
static uint32_t rule(const uint32_t (&w)[3], const uint32_t (&x)[3], const uint32_t (&e)[3]) {
    uint32_t out = 0;
    for (int b = 0; b < 32; ++b) {
        int n = 0;
        for (int j = 0; j < 3; ++j) n += (int)((w[j] >> b) & 1u) + (int)((x[j] >> b) & 1u) + (int)((e[j] >> b) & 1u);
        const int self = (int)((x[1] >> b) & 1u);
        n -= self;
        if (n == 3 || (self && n == 2)) out |= 1u << b;
    }
    return out;
}
int main() {
    int W, H, turns, clear;
    while (std::scanf("%d %d %d %d", &W, &H, &turns, &clear) == 4) {
        const int Ww = (W + 31) / 32;
        const unsigned r = (unsigned)W % 32u;
        if (r == 0) return 3;
        std::vector<uint32_t> cur((size_t)H * Ww), nxt((size_t)H * Ww);  // exactly the board: a read past it is the sanitizer's
        for (auto &v : cur) {
            unsigned t;
            if (std::scanf("%u", &t) != 1) return 2;
            v = t;
        }
        if (clear)
            for (int y = 0; y < H; ++y) cur.at((size_t)y * Ww + Ww - 1) = golk::seam_clear_pad(cur.at((size_t)y * Ww + Ww - 1), r);
        for (int t = 0; t < turns; ++t) {
            for (int y = 0; y < H; ++y)
                for (int c = 0; c < Ww; ++c) {
                    const int ys[3] = {(y + H - 1) % H, y, (y + 1) % H};
                    const int cl = c == 0 ? Ww - 1 : c - 1, cr = c == Ww - 1 ? 0 : c + 1;
                    uint32_t w[3], x[3], e[3];
                    for (int j = 0; j < 3; ++j) {
                        const size_t row = (size_t)ys[j] * Ww;
                        x[j] = cur.at(row + c);
                        uint32_t le = cur.at(row + cl), re = cur.at(row + cr);
                        if (c == 0) le = golk::seam_left_word(le, r);
                        if (c == Ww - 1) x[j] = golk::seam_last_word(x[j], re, r);
                        w[j] = (x[j] << 1) | (le >> 31);  // bit b = cell b - 1
                        e[j] = (x[j] >> 1) | (re << 31);  // bit b = cell b + 1
                    }
                    uint32_t nx = rule(w, x, e);
                    if (c == Ww - 1) nx = golk::seam_clear_pad(nx, r);
                    nxt.at((size_t)y * Ww + c) = nx;
                }
            cur.swap(nxt);
            for (uint32_t v : cur) std::printf("%u ", (unsigned)v);
            std::printf("\n");
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def seam_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("flip_seam")
    src = d / "seam_main.cpp"
    src.write_text(MAIN)
    exe = d / "seam_main"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, str(src), "-o", str(exe)], check=True, timeout=180)
    return str(exe)


def test_seam_steps_equal_oracle(seam_exe):
    rng = np.random.default_rng(0x5EA3)
    cases, text = [], []
    for i, (W, H) in enumerate((W, H) for W in WIDTHS for H in HEIGHTS):
        board = np.where(rng.random((H, W)) < 0.4, 255, 0).astype(np.uint8)
        words = pack_bits(board).copy()
        pad = np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
        assert not (words[:, -1] & pad).any()
        garbage = i % 2 == 1
        if garbage:
            words[:, -1] |= rng.integers(0, 1 << 32, size=H, dtype=np.uint64).astype(np.uint32) & pad
            words[0, -1] |= np.uint32(1 << (W % 32))  # (at least the first padding bit of row 0)
        cases.append((W, H, board))
        text.append(f"{W} {H} {TURNS} {int(garbage)}\n" + " ".join(str(int(v)) for v in words.ravel()) + "\n")
    res = subprocess.run([seam_exe], input="".join(text), capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")
    assert len(lines) == TURNS * len(cases) + 1
    for i, (W, H, board) in enumerate(cases):
        cur = board
        for t in range(TURNS):
            cur = step_np(cur)
            got = np.array(lines[TURNS * i + t].split(), dtype=np.uint64).astype(np.uint32).reshape(H, -1)
            assert np.array_equal(got, pack_bits(cur)), (W, H, t)  # (pack_bits leaves the padding zero)


def test_helpers_word_by_word(seam_exe):
    """A glider crossing the seam of a 33-column board (r = 1: the last word
    holds one column) keeps its five cells on every turn."""
    W, H = 33, 8
    board = np.zeros((H, W), dtype=np.uint8)
    for x, y in ((1, 0), (2, 1), (0, 2), (1, 2), (2, 2)):
        board[1 + y, 28 + x] = 255
    turns = 24  # the glider moves 6 columns: from columns 28..30 across column 32 to columns 1..3
    text = f"{W} {H} {turns} 0\n" + " ".join(str(int(v)) for v in pack_bits(board).ravel()) + "\n"
    res = subprocess.run([seam_exe], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    cur = board
    for t, line in enumerate(res.stdout.split("\n")[:turns]):
        cur = step_np(cur)
        got = np.array(line.split(), dtype=np.uint64).astype(np.uint32).reshape(H, -1)
        assert np.array_equal(got, pack_bits(cur)), t
        assert int((cur == 255).sum()) == 5
    assert (cur[:, :4] == 255).any() and not (cur[:, 28:] == 255).any()
