"""GPU parity of K1w's interior main-loop body (option "skew_interior",
gol_skew_span.h) against the C oracle: every case runs with
the interior body on (1, the default) and with the general body alone (0).

Between the ends of a band's interior span the row map neither wraps nor
clamps, every stored row lies inside the band and the launch counts nothing,
so the bodies there load and store without those decisions.  Covered: shapes
whose plans have interior bodies at (18, 2) on the pair rule, (20, 2) and
(9, 4), turn counts that mix full launches with remainders; a shape whose
bands are so short (30-48 rows at 18 turns) that a span is one body or none;
launches that all count (empty spans) and a step of which only the last launch
counts; the halo clamp and the extended row ranges of a one-rank ring and of
in-process strips; half tiles.

No shape the planner accepts has a plan without any interior body: bands
average at least depth + 3 rows plus the bottom band's handicap, a band of 42
rows has one interior body, and so has a stack's bottom band from 9 rows on
(its main loop runs to its end).  Launches whose every span is empty are
therefore the counting ones and those with the option off; the empty span of
a short band is pinned on the host by tests/test_skew_interior_cpu.py.

The torus seam inside a main loop: on every torus the bottom band of the last
stack reads D rows past the board's last row, and its main loop (which runs to
the band's end, having no band below) meets the wrap D rows before its end:
test_the_last_band_meets_the_seam_in_its_main_loop shows on the host that the
span ends ahead of it, and every torus case here runs such a band.

Coverage cap: each parametrised shape states whether its plan has interior
bodies (golhip_skew_interior_plan: the kernel's own span function over the
launch's bands).  Every shape on the instance that carries the interior body
(the pair rule at two words per lane on full-width tiles) must have some; the
short-band shape has the fewest, about half its main-loop bodies.  The shapes
at (20, 2), (9, 4) and on half-wave tiles run instances that were left without
the body (no gain measured): their plans have none, and they
stay here to pin that the option changes nothing for them."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import COracle

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

i32, i64 = ctypes.c_int32, ctypes.c_int64
SEED = 0x5EED0190


@pytest.fixture(scope="module")
def coracle():
    return COracle()


_boards, _refs = {}, {}


def reference(coracle, W, H, turns):
    """(board, the oracle's board after `turns`), computed once per shape and continued from the turns already run."""
    if (W, H) not in _boards:
        _boards[W, H] = coracle.fill_random(W, H, SEED + W + H)
        _refs[W, H] = {0: _boards[W, H]}
    done = _refs[W, H]
    if turns not in done:
        t0 = max(t for t in done if t <= turns)
        done[turns] = coracle.run(done[t0], turns - t0)
    return _boards[W, H], done[turns]


def interior_plan(b, depth, ext=0, counts=0):
    """(main-loop bodies inside an interior span, all main-loop bodies) of the handle's K1w launch at `depth`."""
    fn = golhip.load().golhip_skew_interior_plan
    fn.argtypes = [ctypes.c_void_p, i32, i32, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    fn.restype = ctypes.c_int
    inner, total = i64(), i64()
    assert fn(b.handle, depth, ext, counts, ctypes.byref(inner), ctypes.byref(total)) == 0
    return inner.value, total.value


def configure(b, depth, wpl, interior, **opts):
    b.set_option("persistent", 0)
    b.set_option("skew", 2)
    b.set_option("wpl", wpl)
    b.set_option("skew_pairs", 3 if depth == 18 else 0)
    b.set_option("skew_half", -1)
    for k, v in opts.items():
        b.set_option(k, v)
    b.set_option("skew_interior", interior)
    b.set_tb_depth(20 if depth == 18 else depth)


def check_plan(b, depth, interior, has_interior, ext=0):
    """The coverage cap: the plan has interior bodies exactly where the case says so."""
    inner, total = interior_plan(b, depth, ext)
    assert total > 0, "no K1w launch at this depth"
    assert 0 <= inner < total
    assert (inner > 0) == (has_interior and interior == 1), (inner, total)
    assert interior_plan(b, depth, ext, counts=1)[0] == 0  # a counting launch: the general body throughout
    return inner, total


# (W, H, depth, words per lane, the plan has interior bodies)
SHAPES = [(4096, 1500, 18, 2, True), (7936, 4099, 18, 2, True),
          (8192, 331, 18, 2, True),   # bands of 31-48 rows: spans of one body, and bands with none
          (4096, 2020, 20, 2, False), (4096, 2009, 9, 4, False)]  # instances without the interior body


@pytest.mark.parametrize("interior", [1, 0])
@pytest.mark.parametrize("turns", [18, 41, 54])
@pytest.mark.parametrize("W,H,depth,wpl,has_interior", SHAPES)
def test_interior_body_matches_oracle(coracle, W, H, depth, wpl, has_interior, turns, interior):
    board, want = reference(coracle, W, H, turns)
    with golhip.Board(W, H) as b:
        configure(b, depth, wpl, interior)
        check_plan(b, depth, interior, has_interior)
        b.load_bytes(board)
        b.step(turns)
        p = b.perf()
        assert p["skew_launches"] >= turns // depth and p["skew_launches"] >= 1, p
        assert (p["pair_launches"] >= 1) == (depth == 18), p
        assert np.array_equal(b.snapshot_bytes(), want)
        assert b.alive_count() == (int((want == 255).sum()), turns)


@pytest.mark.parametrize("interior", [1, 0])
@pytest.mark.parametrize("W,H,depth,wpl", [(4096, 1500, 18, 2), (4096, 2009, 9, 4)])
def test_every_launch_counts_or_only_the_last(coracle, W, H, depth, wpl, interior):
    """Steps of exactly one launch each (every launch counts: the general body
    throughout), then one step of three launches (only the last one counts)."""
    board, _ = reference(coracle, W, H, 0)
    with golhip.Board(W, H) as b:
        configure(b, depth, wpl, interior)
        check_plan(b, depth, interior, depth == 18)
        b.load_bytes(board)
        for t in range(1, 4):
            b.step(depth)
            want = reference(coracle, W, H, depth * t)[1]
            assert b.alive_count() == (int((want == 255).sum()), depth * t)
        assert b.perf()["skew_launches"] == 3
        assert np.array_equal(b.snapshot_bytes(), reference(coracle, W, H, 3 * depth)[1])
        b.step(3 * depth)
        want = reference(coracle, W, H, 6 * depth)[1]
        assert b.perf()["skew_launches"] == 6
        assert b.alive_count() == (int((want == 255).sum()), 6 * depth)
        assert np.array_equal(b.snapshot_bytes(), want)


@pytest.mark.parametrize("interior", [1, 0])
def test_one_rank_ring(coracle, interior):
    """The halo clamp and the extended row ranges [-e, rows + e) of a strip's launches (force_halo)."""
    W, H, turns = 4096, 1500, 3 * 18
    board, want = reference(coracle, W, H, turns)
    with golhip.Board(W, H) as b:
        b.comm_init(golhip.unique_id(), 1, 0)
        b.set_option("force_halo", 1)
        configure(b, 18, 2, interior)
        check_plan(b, 18, interior, True)
        check_plan(b, 18, interior, True, ext=36)
        b.load_bytes(board)
        b.step(turns)
        p = b.perf()
        assert p["halo_bytes"] > 0 and p["pair_launches"] == 3, p
        assert np.array_equal(b.snapshot_bytes(), want)
        assert b.alive_count() == (int((want == 255).sum()), turns)


@pytest.mark.parametrize("interior", [1, 0])
@pytest.mark.parametrize("depth,wpl", [(18, 2), (20, 2)])
def test_three_strips(coracle, depth, wpl, interior):
    W, H, turns = 4096, 3001, 3 * depth + 1
    board, want = reference(coracle, W, H, turns)
    bounds = [H * i // 3 for i in range(4)]
    strips = [golhip.Board(W, H, row0=bounds[i], rows=bounds[i + 1] - bounds[i]) for i in range(3)]
    try:
        for i, s in enumerate(strips):
            configure(s, depth, wpl, interior)
            s.load_bytes(board[bounds[i]:bounds[i + 1]])
        golhip.group_step(strips, turns)
        assert sum(s.perf()["skew_launches"] for s in strips) >= 9
        got = np.concatenate([s.snapshot_bytes() for s in strips])
        assert np.array_equal(got, want)
        assert sum(s.alive_count()[0] for s in strips) == int((want == 255).sum())
    finally:
        for s in strips:
            s.close()


@pytest.mark.parametrize("interior", [1, 0])
@pytest.mark.parametrize("W,H", [(16384, 1000), (2048, 818)])
def test_half_tiles(coracle, W, H, interior):
    """Half-wave tiles on the pair rule: an instance left without the interior
    body (its plans have no interior bodies); the option must change nothing."""
    turns = 2 * 18 + 5
    board, want = reference(coracle, W, H, turns)
    with golhip.Board(W, H) as b:
        configure(b, 18, 2, interior, skew_pairs=5, skew_half=1)
        check_plan(b, 18, interior, False)  # (half-wave tiles: the general body alone)
        b.load_bytes(board)
        b.step(turns)
        p = b.perf()
        assert p["skew_half_launches"] >= 2 and p["pair_launches"] >= 2, p
        assert np.array_equal(b.snapshot_bytes(), want)
        assert b.alive_count() == (int((want == 255).sum()), turns)


def test_the_last_band_meets_the_seam_in_its_main_loop():
    """A torus's last band [eb - S, eb = H - D) has no band below it: its main
    loop runs to push S + 2 D and loads the board's row 0 again at push S + D;
    the span ends ahead of that row, D rows short of where it ends on a strip."""
    fn = golhip.load().golhip_skew_span

    class SpanIn(ctypes.Structure):
        _fields_ = [(n, i32) for n in ("ab", "eb", "depth", "self", "pair", "off", "wrap", "rmax", "half", "dr",
                                       "row_words", "counts", "enabled")]
    fn.argtypes = [ctypes.POINTER(SpanIn), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    fn.restype = ctypes.c_int
    H, D, S = 1500, 18, 186
    lo, hi = i32(), i32()
    torus = SpanIn(ab=H - D - S, eb=H - D, depth=D, self=1, pair=1, off=0, wrap=H, rmax=H - 1, row_words=128, enabled=1)
    assert fn(ctypes.byref(torus), ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert lo.value == 42 and S + D - 9 < hi.value <= S + D - 3   # its last body's six rows end before row H
    strip = SpanIn(ab=H - D - S, eb=H - D, depth=D, self=1, pair=1, off=128, wrap=0, rmax=H + 255, row_words=128,
                   enabled=1)
    assert fn(ctypes.byref(strip), ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert lo.value == 42 and S + 2 * D - 6 < hi.value <= S + 2 * D   # its last body's six stores end inside the band


def test_coverage_cap():
    """Of the shapes above, those on the instance with the interior body all have interior bodies."""
    assert all(has for W, H, depth, wpl, has in SHAPES if (depth, wpl) == (18, 2))
    assert sum(1 for W, H, depth, wpl, has in SHAPES if has) >= 3
