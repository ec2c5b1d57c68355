"""The launch plan of a whole torus on the pair rule's full-width tiles
(golhip_plan.cpp depth_plan with pair_tail), through
golhip_depth_schedule / golhip_launch_cost, and the pair-aware main-loop start
of gol_skew_span.h through golhip_skew_span.  No GPU.

In scope (cap 18, pair_tail 1) the tail of a step may take the pair kernel's
remainder depths 12, 15 and 16 and is ranked by estimated cost.  Everything
else (rings, groups of strips, skew_pairs 0, tb_depth 16 and 20, one and four
words per lane) plans through the same function with pair_tail 0 and must
give the parent's sequences: tests/golden/depth_plan_parent.npz holds, for the
caps those conditions lead to (8, 9, 16, 18, 20, 24, 32) and every turn count
from 1 to 2,200, the (depth, launches) answer of golhip_halo_schedule
(a strip of 2^20 rows, not resident) as the parent commit's build gave it.
"""
import ctypes
import os

import numpy as np
import pytest

golhip = pytest.importorskip("golhip")

i32, i64 = ctypes.c_int32, ctypes.c_int64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_plan_parent.npz")
PAIR_DEPTHS = {12, 15, 16, 18}             # K1w pair instances at two words per lane on full tiles
KERNEL_DEPTHS = {1, 2, 4, 6, 8, 12, 15, 16, 18}  # every depth an in-scope plan may name has a kernel at two words
TURNS = 2200


@pytest.fixture(scope="module")
def lib():
    lib = golhip.load()
    lib.golhip_depth_schedule.argtypes = [i32, i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i64)]
    lib.golhip_depth_schedule.restype = ctypes.c_int
    lib.golhip_launch_cost.argtypes = [i32, i32]
    lib.golhip_launch_cost.restype = i64
    lib.golhip_halo_schedule.argtypes = [i32, i32, i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.golhip_halo_schedule.restype = ctypes.c_int
    return lib


def next_run(lib, cap, pair_tail, left):
    d, n = i32(), i64()
    assert lib.golhip_depth_schedule(cap, pair_tail, left, ctypes.byref(d), ctypes.byref(n)) == 0, (cap, pair_tail, left)
    return d.value, n.value


def replay(lib, cap, pair_tail, turns):
    """The depths golhip_step launches: it asks again before every launch."""
    seq, left = [], turns
    while left > 0:
        d, n = next_run(lib, cap, pair_tail, left)
        assert 1 <= d <= min(cap, left) and 1 <= n and n * d <= left, (turns, left, d, n)
        seq.append(d)
        left -= d
    return seq


def test_in_scope_schedules(lib):
    cost = {(d, p): lib.golhip_launch_cost(d, p) for d in range(1, 33) for p in (0, 1)}
    assert all(c > 0 for c in cost.values())
    improved = 0
    for turns in range(1, TURNS + 1):
        new, old = replay(lib, 18, 1, turns), replay(lib, 18, 0, turns)
        assert sum(new) == turns and sum(old) == turns, turns
        assert set(new) <= KERNEL_DEPTHS, (turns, new)
        assert 15 not in old and set(old) <= KERNEL_DEPTHS, (turns, old)
        c_new = sum(cost[d, 1 if d in PAIR_DEPTHS else 0] for d in new)
        c_old = sum(cost[d, 1 if d == 18 else 0] for d in old)  # the parent ran 18 alone on the pair kernel
        assert c_new <= c_old, (turns, new, old, c_new, c_old)
        improved += c_new < c_old
    assert improved > TURNS // 2


def test_thousand_turns_run_on_the_pair_kernel_throughout(lib):
    seq = replay(lib, 18, 1, 1000)
    assert [d for d in seq if d not in PAIR_DEPTHS] == [], seq
    assert seq == sorted(seq, reverse=True) and seq.count(18) >= 50, seq
    assert len(seq) <= len(replay(lib, 18, 0, 1000))


def test_cost_model(lib):
    """(d + r) x slots: linear in d with the same ramp for both kernels, 12 slots against 13."""
    c = lib.golhip_launch_cost
    assert c(0, 1) == -1 and c(33, 0) == -1
    for p, slots in ((1, 12), (0, 13)):
        assert c(18, p) - c(17, p) == 10 * slots       # tenths of a turn-slot
        assert c(1, p) % slots == 0
    assert c(1, 1) // 12 == c(1, 0) // 13              # the same r
    assert 0 <= c(1, 1) // 12 - 10 < 1000              # r in tenths of a turn


def test_request_is_checked(lib):
    d, n = i32(), i64()
    ok = (18, 1, 100, ctypes.byref(d), ctypes.byref(n))
    assert lib.golhip_depth_schedule(*ok) == 0
    for bad in ((0, 0, 100), (33, 0, 100), (18, 1, 0), (16, 1, 100), (20, 1, 100)):
        assert lib.golhip_depth_schedule(*bad, ctypes.byref(d), ctypes.byref(n)) == -1, bad
    assert lib.golhip_depth_schedule(18, 1, 100, None, ctypes.byref(n)) == -1


def test_out_of_scope_schedules_are_the_parents(lib):
    with np.load(GOLDEN, allow_pickle=False) as z:
        caps, depth, launches = z["caps"], z["depth"], z["launches"]
    assert list(caps) == [8, 9, 16, 18, 20, 24, 32] and depth.shape == (7, TURNS + 1)
    d, k = i32(), i32()
    for i, cap in enumerate(int(c) for c in caps):
        for left in range(1, TURNS + 1):
            assert lib.golhip_halo_schedule(1 << 20, cap, 0, left, ctypes.byref(d), ctypes.byref(k)) == 0
            assert (d.value, k.value) == (depth[i, left], launches[i, left]), (cap, left)
            dd, n = next_run(lib, cap, 0, left)      # groups, and tori out of scope: the same plan, not halo-capped
            assert dd == depth[i, left] and n >= launches[i, left], (cap, left)
            assert dd != 15
        assert 15 not in depth[i]


# ---------------------------------------------------------------- the main loop's start
class SpanIn(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("ab", "eb", "depth", "self", "pair", "off", "wrap", "rmax", "half", "dr",
                                   "row_words", "counts", "enabled")]


@pytest.fixture(scope="module")
def span():
    fn = golhip.load().golhip_skew_span
    fn.argtypes = [ctypes.POINTER(SpanIn), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    fn.restype = ctypes.c_int
    lo, hi = i32(), i32()

    def call(**kw):
        a = SpanIn(**kw)
        assert fn(ctypes.byref(a), ctypes.byref(lo), ctypes.byref(hi)) == 0, kw
        return lo.value, hi.value
    return call


def base_case(S, D, pair, self_, ab=0):
    return dict(ab=ab, eb=ab + S, depth=D, self=self_, pair=pair, off=128, wrap=0, rmax=1 << 30, half=0, dr=0,
                row_words=64, counts=0, enabled=1)


def main_start(span, D, pair):
    """An empty span (option off) stands at the main loop's first push."""
    lo, hi = span(**dict(base_case(60, D, pair, 1), enabled=0))
    assert lo == hi
    return lo


def test_main_loop_start(span):
    for D in (12, 15, 16, 18):
        assert main_start(span, D, 1) % 6 == 0, D
        assert 2 * D <= main_start(span, D, 1) < 2 * D + 6, D   # the fill's 2 D pushes, then at most one group more
    assert [main_start(span, D, 1) for D in (12, 15, 16, 18)] == [24, 30, 36, 36]
    for D in (8, 9, 16, 18, 20):                                  # the one-argument start: as it was
        assert main_start(span, D, 0) == 3 * ((2 * D + 2) // 3), D
    assert main_start(span, 8, 1) == 18 and main_start(span, 18, 1) == 36  # pair instances from before: unchanged


def body_is_interior(c, k, k0):
    """The general body's own decisions, row by row (gol_kernels.hip stream_skew), for the pair rule's six-row body.
    The rows a body stores are those of the group before it: the main loop's first body (push k0) stores nothing, and
    the fill has stored the rows of its own groups (at D = 16 the rows 1-3, which that body must not overwrite)."""
    D, S = c["depth"], c["eb"] - c["ab"]
    if c["counts"] or not c["enabled"] or k - 3 < k0:
        return False
    r = c["ab"] + c["off"] + k + 3
    r = r % c["wrap"] if c["wrap"] > 0 else r
    for i in range(6):
        if r > c["rmax"]:
            return False                                          # clamped
        nxt = 0 if (c["wrap"] > 0 and r + 1 == c["wrap"]) else r + 1
        if i + 1 < 6 and nxt != r + 1:
            return False                                          # wraps inside the body
        r = nxt
    return all(0 <= oi < S for oi in range(k - 3 - 2 * D, k + 3 - 2 * D))


def check(span, c, k0):
    """Every body inside the span qualifies; the span is made of whole bodies of the main loop."""
    D, S = c["depth"], c["eb"] - c["ab"]
    kmain = S + (2 * D if c["self"] else 6)
    lo, hi = span(**c)
    assert lo <= hi and (lo - k0) % 6 == 0 and (hi - k0) % 6 == 0, (c, lo, hi)
    if lo < hi:
        assert k0 <= lo and hi - 6 < kmain, (c, lo, hi)
    for k in range(lo, hi, 6):
        assert body_is_interior(c, k, k0), (c, lo, hi, k)
    return (hi - lo) // 6


BANDS = [21, 22, 24, 30, 36, 42, 43, 48, 54, 60, 66, 90, 120, 150, 198, 199, 200]


@pytest.mark.parametrize("D", [12, 15, 16])
def test_interior_span_of_the_new_depths(span, D):
    k0 = main_start(span, D, 1)
    some = 0
    for S in BANDS:
        for self_ in (0, 1):             # inner bands are multiples of 6 rows on the pair rule; bottom bands any
            if not self_ and S % 6:
                continue
            c = base_case(S, D, 1, self_, ab=-D)
            n = check(span, c, k0)
            kmain = S + (2 * D if self_ else 6)
            assert n == sum(body_is_interior(c, k, k0) for k in range(k0, kmain, 6)), (c, n)  # nothing in the way: all of them
            some += n
            assert check(span, dict(c, counts=1), k0) == 0
            rows = S + 2 * D + 12
            if S > 66 and S != 200:
                continue
            for wrap in (rows + 5, 4 * rows):                        # the wrap at every row of the band's input
                for p in range(rows + 1):
                    cw = dict(c, wrap=wrap, rmax=wrap - 1, off=(-(c["ab"] + p)) % wrap)
                    some += check(span, cw, k0)
            for p in range(-2, rows + 1):                            # the clamp at every row
                cc = base_case(S, D, 1, self_, ab=5)
                cc.update(rmax=cc["ab"] + cc["off"] + p)
                check(span, cc, k0)
    assert some > 0
