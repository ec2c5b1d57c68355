"""The launch planner only asks for kernels that exist, and each per-launch
kernel instantiation is run by a test that proves through golhip_perf that it
was the one that ran.

golhip_plan.cpp picks (kernel family, depth, words per lane) per launch; the
kernels exist only at the points the dispatch tables of gol_kernels.hip
instantiate.  These tests walk the planner's inputs (tb_depth, words per lane,
strip heights, ring heights) across every value, the special depths 9 (quads
only) and 18 (the pair rule only) included, and pin every per-launch
instantiation (gol_tb_kernel<D, skip, wpl>, gol_tb_pair_kernel<D, wpl>) with
one launch of exactly that depth.  Bit-exact against the C oracle, alive
counts included; the counters of golhip_perf say which family ran and how
many launches it took.
"""
import numpy as np
import pytest

from oracle.oracle import COracle, flips_np

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

# Depths the per-launch kernels are instantiated at (dispatch / dispatch_pair
# in gol_kernels.hip); 18 at two words per lane belongs to the pair rule and
# is never a tb_depth a plan settles on by itself (depth_cap).
TB_DEPTHS = {1: [1, 2, 4, 6, 8, 12, 16, 20, 24, 32], 2: [1, 2, 4, 6, 8, 12, 16, 20], 4: [1, 2, 4, 6, 8, 9]}
FAMILIES = {"unpaired-skip": {"paired_bands": 0, "fill_skip": 1},
            "unpaired-fill": {"paired_bands": 0, "fill_skip": 0},
            "paired": {"paired_bands": 1, "fill_skip": 1}}
RESIDENT_OR_SKEW = ("persist_launches", "skew_launches", "lds_launches")

_oracle = None
_boards = {}  # (W, H) -> {turn: board}; turn 0 is the random start


def oracle_at(W, H, turn):
    """The oracle's board of the (W, H) start after `turn` turns, computed once
    (from the nearest earlier turn already known) and never modified."""
    global _oracle
    if _oracle is None:
        _oracle = COracle()
    known = _boards.setdefault((W, H), {})
    if 0 not in known:
        known[0] = _oracle.fill_random(W, H, 0x5EED0C10 + 131 * W + H)
        known[0].setflags(write=False)
    if turn not in known:
        base = max(t for t in known if t <= turn)
        known[turn] = _oracle.run(known[base], turn - base)
        known[turn].setflags(write=False)
    return known[turn]


def alive(board):
    return int((board == 255).sum())


def set_options(b, **options):
    for k, v in options.items():
        b.set_option(k, v)


def check_board(b, W, H, turn, what):
    want = oracle_at(W, H, turn)
    assert np.array_equal(b.snapshot_bytes(), want), what
    assert b.alive_count() == (alive(want), turn), what


def expected_depth(wpl, t):
    """The deepest launch a tb_depth of t allows at `wpl` words per lane."""
    if wpl == 4:
        return 9 if t >= 9 else max(d for d in TB_DEPTHS[4] if d <= t and d != 9)
    return max(d for d in TB_DEPTHS[wpl] if d <= t)


# ---------------------------------------------------------------- A1: one instantiation at a time
@pytest.mark.parametrize("W,H", [(128, 3), (8064, 37)])
@pytest.mark.parametrize("wpl", [1, 2, 4])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_per_launch_instantiations(family, wpl, W, H):
    """Every (depth, words per lane) the per-launch families are instantiated
    at, as launches of exactly that depth: step(D) three times is three
    launches of D turns of kernel variant 1, never a resident or K1w launch.
    128 x 3: one partial tile, fewer rows than the depths from 4 on, the torus
    seam in every launch; 8064 x 37: one full tile plus one lane of a second
    at four words per lane (several tiles at one and two), a prime height."""
    with golhip.Board(W, H) as b:
        set_options(b, persistent=0, skew=0, wpl=wpl, **FAMILIES[family])
        for D in TB_DEPTHS[wpl]:
            for rpw in (0, 1, 5):
                what = (family, wpl, W, H, D, rpw)
                b.set_tb_depth(D)
                b.set_rows_per_wave(rpw)
                b.load_bytes(oracle_at(W, H, 0))
                before = b.perf()
                for i in (1, 2, 3):
                    b.step(D)
                    check_board(b, W, H, i * D, what)
                    p = b.perf()
                    assert p["step_launches"] - before["step_launches"] == 1, (what, p)
                    assert p["step_turns"] - before["step_turns"] == D, (what, p)
                    assert p["kernel_variant"] == 1 and p["words_per_lane"] == wpl, (what, p)
                    assert all(p[k] == 0 for k in RESIDENT_OR_SKEW), (what, p)
                    before = p


# ---------------------------------------------------------------- A2: every tb_depth has a kernel
@pytest.mark.parametrize("wpl", [1, 2, 4])
def test_every_tb_depth_has_a_kernel(wpl):
    """tb_depth 1..32 on a 128 x 40 torus, per-launch kernels only: the deepest
    launch is the largest instantiated depth within the setting (18 gives 16:
    depth 18 is the pair rule's), step(E) is one launch, and a longer step is
    exact in at least ceil(turns / E) launches."""
    W, H = 128, 40
    with golhip.Board(W, H) as b:
        set_options(b, persistent=0, skew=0, wpl=wpl)
        for t in range(1, 33):
            E, more = expected_depth(wpl, t), 2 * t + 5
            what = (wpl, t, E)
            b.set_tb_depth(t)
            b.load_bytes(oracle_at(W, H, 0))
            p0 = b.perf()
            b.step(E)
            p1 = b.perf()
            check_board(b, W, H, E, what)
            assert p1["step_launches"] - p0["step_launches"] == 1, (what, p1)
            assert p1["step_turns"] - p0["step_turns"] == E, (what, p1)
            assert p1["kernel_variant"] == 1 and p1["words_per_lane"] == wpl, (what, p1)
            b.step(more)
            p2 = b.perf()
            check_board(b, W, H, E + more, what)
            assert p2["step_launches"] - p1["step_launches"] >= -(-more // E), (what, p2)
            assert p2["step_turns"] - p1["step_turns"] == more, (what, p2)
            assert all(p2[k] == 0 for k in RESIDENT_OR_SKEW), (what, p2)


@pytest.mark.parametrize("wpl", [1, 2, 4])
def test_every_tb_depth_with_k1w_no_pairs(wpl):
    """The same walk with K1w wherever a stack plans (skew 2) and the pair rule
    off: 128 x 450 is tall enough for a K1w stack at depth 32.  Exact at every
    tb_depth, and no launch takes the pair kernel."""
    W, H = 128, 450
    with golhip.Board(W, H) as b:
        set_options(b, persistent=0, skew=2, skew_pairs=0, wpl=wpl)
        for t in range(1, 33):
            E, more = expected_depth(wpl, t), 2 * t + 5
            what = (wpl, t, E)
            b.set_tb_depth(t)
            b.load_bytes(oracle_at(W, H, 0))
            p0 = b.perf()
            b.step(E)
            check_board(b, W, H, E, what)
            b.step(more)
            check_board(b, W, H, E + more, what)
            p = b.perf()
            assert p["pair_launches"] == 0 and p["pair_turns"] == 0, (what, p)
            assert p["step_turns"] - p0["step_turns"] == E + more, (what, p)
            assert p["persist_launches"] == 0 and p["lds_launches"] == 0, (what, p)
            assert p["words_per_lane"] == wpl, (what, p)


@pytest.mark.parametrize("t", [18, 19, 20])
def test_pair_rule_owns_depth_18(t):
    """With the pair rule on (skew_pairs 1, full tiles) every tb_depth from 18
    on plans 18 turns a launch at two words per lane, and the first launch is
    the pair kernel."""
    W, H = 128, 450
    with golhip.Board(W, H) as b:
        set_options(b, persistent=0, skew=2, skew_pairs=1, skew_half=-1, wpl=2)
        b.set_tb_depth(t)
        b.load_bytes(oracle_at(W, H, 0))
        assert b.perf()["tb_depth"] == 18
        b.step(18)
        p = b.perf()
        check_board(b, W, H, 18, t)
        assert (p["step_launches"], p["skew_launches"], p["pair_launches"], p["pair_turns"]) == (1, 1, 1, 18), p
        assert p["kernel_variant"] == 3 and p["words_per_lane"] == 2, p
        b.step(2 * t + 5)
        p = b.perf()
        check_board(b, W, H, 18 + 2 * t + 5, t)
        assert p["pair_launches"] >= 2 and p["step_turns"] == 18 + 2 * t + 5, p
        assert p["persist_launches"] == 0 and p["lds_launches"] == 0, p


# ---------------------------------------------------------------- A3: strip heights, all of them
STRIP_BOARDS = [(96, 0), (128, 2), (128, 4)]  # (width, option wpl); 96 wide forces one word per lane
MAX_DEPTH = {1: 32, 2: 20, 4: 9}              # golk::max_depth_for


def make_strips(W, heights, wpl, tb):
    H = sum(heights)
    start = oracle_at(W, H, 0)
    strips, r0 = [], 0
    for rows in heights:
        s = golhip.Board(W, H, row0=r0, rows=rows)
        strips.append(s)
        if wpl:
            s.set_option("wpl", wpl)
        if tb:
            s.set_tb_depth(tb)
        s.load_bytes(start[r0:r0 + rows])
        r0 += rows
    return strips


def check_strips(strips, W, heights, wpl, tb, turns, what):
    """Board, alive count, and the counters: per-launch kernels only, every
    strip the same launches, no fewer than the deepest launch allows."""
    H = sum(heights)
    want = oracle_at(W, H, turns)
    got = np.concatenate([s.snapshot_bytes() for s in strips])
    assert np.array_equal(got, want), what
    counts = [s.alive_count() for s in strips]
    assert all(at == turns for _, at in counts), (what, counts)
    assert sum(c for c, _ in counts) == alive(want), what
    perfs = [s.perf() for s in strips]
    width = wpl or 1
    deepest = min(tb or 20, MAX_DEPTH[width], min(heights))
    for p in perfs:
        assert p["words_per_lane"] == width, (what, p)
        # (strips this small never fill the CUs with K1w stacks: the default "skew" 1 leaves them alone)
        assert p["kernel_variant"] == 1 and all(p[k] == 0 for k in RESIDENT_OR_SKEW), (what, p)
        assert p["halo_bytes"] > 0, (what, p)
    return perfs, deepest


@pytest.mark.parametrize("tb", [None, 32])
@pytest.mark.parametrize("W,wpl", STRIP_BOARDS)
def test_strip_heights_all(W, wpl, tb):
    """group_step on strips of [r, 40, 23] rows for every r in 1..33 with the
    product's defaults: the group's launch depth is capped by its shortest
    strip, so r walks the cap across every value, 9 and 18 included."""
    turns = 45
    for r in range(1, 34):
        heights = [r, 40, 23]
        what = (W, wpl, tb, r)
        strips = make_strips(W, heights, wpl, tb)
        try:
            golhip.group_step(strips, turns)
            perfs, deepest = check_strips(strips, W, heights, wpl, tb, turns, what)
            for p in perfs:
                assert p["step_turns"] == turns, (what, p)
                assert p["step_launches"] == perfs[0]["step_launches"] >= -(-turns // deepest), (what, p)
        finally:
            for s in strips:
                s.close()


@pytest.mark.parametrize("tb", [None, 32])
@pytest.mark.parametrize("W,wpl", STRIP_BOARDS)
def test_strip_heights_flips(W, wpl, tb):
    """The same groups through group_step(want_flips=True) at the heights
    around the special depths: the strips' flip lists, concatenated, are the
    oracle's diff of the last turn."""
    turns = 45
    for r in (9, 17, 18, 19):
        heights = [r, 40, 23]
        H = sum(heights)
        what = (W, wpl, tb, r)
        strips = make_strips(W, heights, wpl, tb)
        try:
            golhip.group_step(strips, turns, want_flips=True)
            perfs, deepest = check_strips(strips, W, heights, wpl, tb, turns, what)
            fl = np.concatenate([s.flips() for s in strips])
            assert np.array_equal(fl, flips_np(oracle_at(W, H, turns - 1), oracle_at(W, H, turns))), what
            for p in perfs:
                assert p["step_turns"] == turns, (what, p)  # 44 turns fused, then the last one alone
                assert p["step_launches"] == perfs[0]["step_launches"] >= -(-(turns - 1) // deepest) + 1, (what, p)
        finally:
            for s in strips:
                s.close()


# ---------------------------------------------------------------- A4 / A5: the one-rank ring
def replay_schedule(H, cap, turns, resident, Ww):
    """(rounds, launches, halo bytes) of golhip_halo_schedule's rounds for `turns` turns."""
    rounds = launches = nbytes = 0
    left = turns
    while left > 0:
        d, k = golhip.halo_schedule(H, cap, left, resident)
        assert 1 <= k * d <= left
        rounds += 1
        launches += k
        nbytes += 2 * k * d * Ww * 4
        left -= k * d
    return rounds, launches, nbytes


@pytest.mark.parametrize("persistent", [0, -1])
@pytest.mark.parametrize("W,H,wpl", [(96, 18, 0), (128, 18, 2), (128, 9, 4), (96, 9, 0)])
def test_one_rank_ring_special_heights(W, H, wpl, persistent):
    """A one-rank RCCL ring (force_halo) whose strip has exactly 18 or 9 rows:
    the halo rows cap the launch depth at the strip's rows, the two depths
    only one kernel family has."""
    turns = 61
    with golhip.Board(W, H) as b:
        b.comm_init(golhip.unique_id(), 1, 0)
        set_options(b, force_halo=1, persistent=persistent)
        if wpl:
            b.set_option("wpl", wpl)
        b.load_bytes(oracle_at(W, H, 0))
        b.step(turns)
        p = b.perf()
        check_board(b, W, H, turns, (W, H, wpl, persistent))
        # (a resident launch starved by a co-tenant re-runs the step on the per-launch schedule)
        resident = persistent != 0 and p["persist_fallbacks"] == 0
        rounds, launches, nbytes = replay_schedule(H, p["tb_depth"], turns, resident, W // 32)
        assert p["words_per_lane"] == (wpl or 1), p
        # 18 rows: 16 turns a launch (18 is the pair rule's); 9 rows: 9 on per-launch quads alone, else 8
        assert p["tb_depth"] == (16 if H == 18 else 9 if (wpl == 4 and not resident) else 8), p
        assert p["lds_launches"] == 0, p
        assert p["halo_exchanges"] == rounds and p["halo_bytes"] == nbytes, (p, rounds, nbytes)
        assert p["step_turns"] + p["persist_turns"] == turns, p
        if persistent == 0:
            assert p["persist_launches"] == 0 and p["step_launches"] == launches, (p, launches)
            assert p["kernel_variant"] == 1 and p["skew_launches"] == 0, p
        else:  # a resident launch takes a round's k super-steps at once
            assert rounds <= p["step_launches"] + p["persist_launches"] <= launches, (p, rounds, launches)


@pytest.mark.parametrize("W,H,wpl,tb", [(2048, 300, 0, 16), (96, 18, 0, None), (128, 9, 4, None)])
def test_engine_runs_the_schedule_it_publishes(W, H, wpl, tb):
    """include/golhip.h: golhip_halo_schedule is the schedule "exactly as
    golhip_step runs it".  Replayed from golhip_perf's tb_depth, its rounds,
    launches and halo bytes are the engine's counters after 203 turns."""
    turns = 203
    with golhip.Board(W, H) as b:
        b.comm_init(golhip.unique_id(), 1, 0)
        set_options(b, force_halo=1, persistent=0, skew=0)
        if wpl:
            b.set_option("wpl", wpl)
        if tb:
            b.set_tb_depth(tb)
        b.load_bytes(oracle_at(W, H, 0))
        b.step(turns)
        p = b.perf()
        check_board(b, W, H, turns, (W, H, wpl, tb))
        rounds, launches, nbytes = replay_schedule(H, p["tb_depth"], turns, False, W // 32)
        assert p["halo_exchanges"] == rounds, (p, rounds)
        assert p["halo_bytes"] == nbytes, (p, nbytes)
        assert p["step_launches"] == launches and p["step_turns"] == turns, (p, launches)
        assert p["kernel_variant"] == 1 and all(p[k] == 0 for k in RESIDENT_OR_SKEW), p
