"""GPU parity of the pair rule's remainder launches against
the C oracle: on a whole torus whose K1w plan runs the pair rule on full-width
tiles, the last launches of a step take gol_skew_kernel<12 | 15 | 16, 2, false,
true> where they ran the 9-LUT instances.

Shapes of tests/test_gpu_skew_interior.py ("skew" 2, so that small boards take
K1w): 4096 x 1500, 7936 x 4099 (a partial last tile, a prime height) and 8192 x
331, whose bands are 30-48 rows short and whose last band wraps inside its main
loop.  Turn counts: one launch of exactly 12, 15 and 16 turns, and steps that
end in them: 33 = 18 + 15, 28 = 16 + 12, 46 = 18 + 16 + 12 and 82 = 18 +
4 x 16 (2 x 18 + 16 + 15 + 15 costs the same, and ties keep the schedule of
fewest launches; the plans are asserted, from golhip_depth_schedule).  Every case
runs with the interior main-loop body on and off, and compares the alive count
of the step's last launch (the one launch that counts) beside the board.
"""
import ctypes
import os

import numpy as np
import pytest

from oracle.oracle import COracle

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

i32, i64 = ctypes.c_int32, ctypes.c_int64
SEED = 0x5EED0230
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "depth_plan_parent.npz")
SHAPES = [(4096, 1500), (7936, 4099), (8192, 331)]
PLANS = {12: [12], 15: [15], 16: [16], 28: [16, 12], 33: [18, 15], 46: [18, 16, 12], 82: [18, 16, 16, 16, 16]}


@pytest.fixture(scope="module")
def coracle():
    return COracle()


_boards, _refs = {}, {}


def reference(coracle, W, H, turns):
    """(start, the oracle's board after `turns`): computed once per shape, continued from the turns already run."""
    if (W, H) not in _boards:
        _boards[W, H] = coracle.fill_random(W, H, SEED + W + H)
        _refs[W, H] = {0: _boards[W, H]}
    done = _refs[W, H]
    if turns not in done:
        t0 = max(t for t in done if t <= turns)
        done[turns] = coracle.run(done[t0], turns - t0)
        done[turns].setflags(write=False)
    return _boards[W, H], done[turns]


def planned(turns, pair_tail=1, cap=18):
    """The depths golhip_step launches for a step of `turns` (it asks before every launch)."""
    fn = golhip.load().golhip_depth_schedule
    fn.argtypes = [i32, i32, i64, ctypes.POINTER(i32), ctypes.POINTER(i64)]
    fn.restype = ctypes.c_int
    seq, left = [], turns
    d, n = i32(), i64()
    while left > 0:
        assert fn(cap, pair_tail, left, ctypes.byref(d), ctypes.byref(n)) == 0
        seq.append(d.value)
        left -= d.value
    return seq


def interior_plan(b, depth):
    fn = golhip.load().golhip_skew_interior_plan
    fn.argtypes = [ctypes.c_void_p, i32, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    fn.restype = ctypes.c_int
    inner, total = i64(), i64()
    assert fn(b.handle, depth, 0, 0, ctypes.byref(inner), ctypes.byref(total)) == 0
    return inner.value, total.value


def configure(b, interior, skew_pairs=3):
    b.set_option("persistent", 0)
    b.set_option("skew", 2)
    b.set_option("wpl", 2)
    b.set_option("skew_pairs", skew_pairs)
    b.set_option("skew_half", -1)
    b.set_option("skew_interior", interior)
    b.set_tb_depth(20)


def test_the_plans_of_these_turn_counts():
    for turns, seq in PLANS.items():
        assert planned(turns) == seq, turns
    assert {d for seq in PLANS.values() for d in seq} == {12, 15, 16, 18}
    assert all(d in {seq[-1] for seq in PLANS.values() if len(seq) > 1} for d in (12, 15))  # as a longer step's tail
    assert any(16 in seq[1:] for seq in PLANS.values())


@pytest.mark.parametrize("interior", [1, 0])
@pytest.mark.parametrize("turns", sorted(PLANS))
@pytest.mark.parametrize("W,H", SHAPES)
def test_remainder_launches_match_oracle(coracle, W, H, turns, interior):
    board, want = reference(coracle, W, H, turns)
    with golhip.Board(W, H) as b:
        configure(b, interior)
        assert b.perf()["tb_depth"] == 18
        b.load_bytes(board)
        b.step(turns)
        p = b.perf()
        n = len(PLANS[turns])
        # every launch of the step ran on the pair kernel: none is left to the 9-LUT stages
        assert (p["step_launches"], p["skew_launches"], p["pair_launches"]) == (n, n, n), p
        assert p["pair_turns"] == turns and p["step_turns"] == turns, p
        assert p["kernel_variant"] == 3 and p["words_per_lane"] == 2, p
        assert np.array_equal(b.snapshot_bytes(), want)
        assert b.alive_count() == (int((want == 255).sum()), turns)


@pytest.mark.parametrize("interior", [1, 0])
def test_interior_bodies_and_counting_launches(coracle, interior):
    """The new instances carry the interior body (their plans have interior bodies with the option on, none with it
    off); steps of one launch each count in every launch (empty spans), then one step whose last launch alone counts."""
    W, H = 4096, 1500
    board, _ = reference(coracle, W, H, 0)
    with golhip.Board(W, H) as b:
        configure(b, interior)
        for depth in (12, 15, 16, 18):
            inner, total = interior_plan(b, depth)
            assert total > 0 and 0 <= inner < total and (inner > 0) == (interior == 1), (depth, inner, total)
        b.load_bytes(board)
        at = 0
        for depth in (12, 15, 16):
            b.step(depth)
            at += depth
            want = reference(coracle, W, H, at)[1]
            assert b.alive_count() == (int((want == 255).sum()), at)
        assert np.array_equal(b.snapshot_bytes(), reference(coracle, W, H, at)[1])
        b.step(46)
        at += 46
        want = reference(coracle, W, H, at)[1]
        p = b.perf()
        assert p["pair_launches"] == 6 and p["pair_turns"] == at == p["step_turns"], p
        assert b.alive_count() == (int((want == 255).sum()), at)
        assert np.array_equal(b.snapshot_bytes(), want)


@pytest.mark.parametrize("turns", [28, 46, 82])
def test_without_the_pair_rule_nothing_changes(coracle, turns):
    """skew_pairs 0: the parent's launches (tests/golden/depth_plan_parent.npz, cap 20), none on the pair kernel."""
    W, H = 4096, 1500
    with np.load(GOLDEN, allow_pickle=False) as z:
        depth = z["depth"][list(z["caps"]).index(20)]
    launches, left = 0, turns
    while left > 0:
        left -= int(depth[left])
        launches += 1
    assert len(planned(turns, pair_tail=0, cap=20)) == launches
    board, want = reference(coracle, W, H, turns)
    with golhip.Board(W, H) as b:
        configure(b, 1, skew_pairs=0)
        assert b.perf()["tb_depth"] == 20
        b.load_bytes(board)
        b.step(turns)
        p = b.perf()
        assert p["step_launches"] == launches and p["step_turns"] == turns, p
        assert p["pair_launches"] == 0 and p["pair_turns"] == 0, p
        assert np.array_equal(b.snapshot_bytes(), want)
        assert b.alive_count() == (int((want == 255).sum()), turns)
