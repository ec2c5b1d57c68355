"""The padded torus on the GPU (golhip_set_pad_step): boards
whose width is no multiple of 32 stepped on the fast per-launch kernels as a
Wp-column torus with ghost columns, against the per-cell oracle.

Every case runs with mode 1 (always) unless it says otherwise; odd widths take
the per-cell oracle, so the cases stay under about 5e7 cell-updates.
"""
import functools

import numpy as np
import pytest

from oracle.oracle import COracle, flips_np, pack_bits, pgm_bytes, read_pgm, step_np

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

SHAPES = [(1, 1), (3, 5), (16, 16), (17, 9), (33, 64), (63, 64), (65, 3), (95, 2), (100, 37), (127, 40), (129, 1),
          (191, 33), (1000, 300)]
# (words per lane, tb_depth).  (4, 9) is this file's own: quads where Wp % 128 == 0, else pairs at 9 -> 8.
PLANS = [(1, 32), (1, 16), (2, 18), (2, 20), (4, 9)]


@functools.lru_cache(maxsize=None)
def oracle():
    return COracle()


def soup(W, H, seed, p=0.35):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((H, W)) < p, 255, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def truth(W, H, seed, turns):
    """The oracle's board after `turns` turns (computed once, never written)."""
    out = oracle().run_exact(soup(W, H, seed), turns)
    out.setflags(write=False)
    return out


def alive(board):
    return int(np.count_nonzero(board == 255))


def check_board(b, want, turns, what):
    """snapshot_bytes, alive_count and board_hash against a fresh handle loaded with the oracle's board."""
    H, W = want.shape
    assert np.array_equal(b.snapshot_bytes(), want), what
    assert b.alive_count() == (alive(want), turns), what
    assert b.turn() == turns, what
    with golhip.Board(W, H) as ref:
        ref.load_bytes(want)
        assert b.board_hash() == ref.board_hash() == golhip.board_hash_np(pack_bits(want)), what
        assert np.array_equal(b.snapshot_bits(), ref.snapshot_bits()), what  # (padding bits clear)


# ---------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("skew", [0, 2])
@pytest.mark.parametrize("wpl,depth", PLANS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_parity_with_oracle(W, H, wpl, depth, skew):
    """2 depth + 5 turns: three launches or more, so the pad pass, the seam
    refresh and the unpad pass all run.  (63, 64) and (127, 40) at depth 32 are
    the tight cases (ghosts of 33 / 32 cells); boards narrower than a ghost
    (1, 3, 16, 17 wide) replicate inside it (the mod)."""
    turns = 2 * depth + 5
    what = (W, H, wpl, depth, skew)
    with golhip.Board(W, H) as b:
        b.set_pad_step(1)
        b.set_option("wpl", wpl)
        b.set_option("skew", skew)
        b.set_tb_depth(depth)
        b.load_bytes(soup(W, H, 1000 * W + H))
        b.step(turns)
        p = b.perf()
        print(what, {k: p[k] for k in ("step_launches", "pad_launches", "skew_launches", "pair_launches",
                                       "kernel_variant")})
        check_board(b, truth(W, H, 1000 * W + H, turns), turns, what)
        assert p["step_turns"] == turns and p["persist_launches"] == 0, (what, p)
        assert p["pad_launches"] == p["step_launches"] >= -(-turns // depth), (what, p)
        assert p["kernel_variant"] in (1, 3) and (skew or p["skew_launches"] == 0), (what, p)


# ---------------------------------------------------------------- the refresh itself
@pytest.mark.parametrize("W,H", [(100, 37), (63, 64)])
def test_refresh_between_launches(W, H):
    """100 turns in launches of 16.  The control first: with the ghosts written
    once the numpy emulation of the same schedule is wrong at turn 100 (small
    or sparse boards can die out and hide a missing refresh), so the GPU's
    result shows the seam kernel at work."""
    board, want = soup(W, H, 11), truth(W, H, 11, 100)
    assert alive(want) > 0
    assert not np.array_equal(golhip.pad_run_np(board, 100, 16, refresh_all=False), want)
    assert np.array_equal(golhip.pad_run_np(board, 100, 16), want)
    with golhip.Board(W, H) as b:
        b.set_pad_step(1)
        b.set_tb_depth(16)
        b.load_bytes(board)
        b.step(100)
        check_board(b, want, 100, (W, H))
        p = b.perf()
        assert p["pad_launches"] == p["step_launches"] == 7 and p["step_turns"] == 100, p  # 4 x 16 + 3 x 12


# ---------------------------------------------------------------- sequences on one handle
def test_sequence_on_one_handle():
    """Steps, a snapshot between them, a new board, a want_flips step (its last
    turn on K1g from the unpadded board), then the same handle with the padded
    path off: the canonical board is whole after every call."""
    W, H = 100, 37
    with golhip.Board(W, H) as b:
        b.set_pad_step(1)
        b.load_bytes(soup(W, H, 5))
        b.step(7)
        assert np.array_equal(b.snapshot_bytes(), truth(W, H, 5, 7))
        p = b.perf()
        assert p["pad_launches"] == p["step_launches"] == 2 and p["step_turns"] == 7, p  # 6 + 1
        b.step(40)
        check_board(b, truth(W, H, 5, 47), 47, "47")
        b.load_bytes(soup(W, H, 6))
        assert b.turn() == 0 and b.alive_count() == (alive(soup(W, H, 6)), 0)
        b.perf_reset()
        b.step(33, want_flips=True)
        before, after = truth(W, H, 6, 32), truth(W, H, 6, 33)
        assert np.array_equal(after, step_np(before))
        assert np.array_equal(b.flips(), flips_np(before, after))
        check_board(b, after, 33, "flips")
        p = b.perf()
        # 32 turns on the wide board in two launches, then the last one alone on the any-width kernel
        assert p["pad_launches"] == 2 and p["step_launches"] == 3 and p["step_turns"] == 33, p
        assert p["kernel_variant"] == 0, p
        b.set_pad_step(0)
        b.perf_reset()
        b.step(5)
        check_board(b, truth(W, H, 6, 38), 38, "mode 0")
        p = b.perf()
        assert p["pad_launches"] == 0 and p["step_launches"] == 5 and p["kernel_variant"] == 0, p


# ---------------------------------------------------------------- against K1g at a size the oracle cannot reach
def test_large_board_against_generic_kernel():
    W, H, turns = 5001, 4999, 40
    res = []
    for mode in (0, 1):
        with golhip.Board(W, H) as b:
            b.set_pad_step(mode)
            b.fill_random(12345)
            b.step(turns)
            res.append((b.board_hash(), b.alive_count()))
            p = b.perf()
            print(mode, {k: p[k] for k in ("step_launches", "pad_launches", "skew_launches", "kernel_variant",
                                           "words_per_lane")})
            if mode == 0:
                assert p["step_launches"] == turns and p["pad_launches"] == 0 and p["kernel_variant"] == 0, p
            else:
                assert p["pad_launches"] == p["step_launches"] <= 3 and p["step_turns"] == turns, p
    assert res[0] == res[1] and res[0][1][0] > 0 and res[0][1][1] == turns, res


# ---------------------------------------------------------------- the default rule
# profiles/widths/bench_widths.json: the padded path won every repetition for
# calls of two turns or more at every size, for one-turn calls from 1000^2 on;
# one-turn calls of smaller boards stay on the any-width kernel (100^2 lost).
RULE_ON = [(100, 37, 2), (1000, 300, 64), (1000, 1000, 1)]
RULE_OFF = [(100, 37, 1), (1000, 300, 1)]


def test_default_rule():
    for cases, padded in ((RULE_ON, True), (RULE_OFF, False)):
        for W, H, n in cases:
            with golhip.Board(W, H) as b:
                b.load_bytes(soup(W, H, 3))
                b.step(n)
                p = b.perf()
                assert (p["pad_launches"] > 0) == padded, ((W, H, n), p)
                assert p["kernel_variant"] == (1 if padded else 0) or p["skew_launches"] > 0, ((W, H, n), p)
                assert np.array_equal(b.snapshot_bytes(), truth(W, H, 3, n))
                assert b.alive_count() == (alive(truth(W, H, 3, n)), n)


def test_timing_and_reset():
    """The wide board's timed launches are the owner's step launches, and
    golhip_perf_reset zeroes the new counter with the rest."""
    W, H = 100, 37
    with golhip.Board(W, H, timing=True) as b:
        b.set_pad_step(1)
        b.load_bytes(soup(W, H, 2))
        b.step(32)
        p = b.perf()
        assert p["pad_launches"] == p["step_launches"] == 2 and p["step_kernel_ms"] > 0, p
        assert p["cell_updates"] == W * H * 32, p
        b.perf_reset()
        p = b.perf()
        assert p["pad_launches"] == p["step_launches"] == p["step_turns"] == 0 and p["step_kernel_ms"] == 0, p
        assert p["turns"] == 32


# ---------------------------------------------------------------- refusals
def test_refusals():
    with golhip.Board(96, 8) as b:  # a width the fast kernels take as it is
        with pytest.raises(golhip.GolHipError) as e:
            b.set_pad_step(1)
        assert e.value.code == golhip.GOLHIP_EINVAL
        b.set_pad_step(0)
        b.set_pad_step(-1)
    with golhip.Board(100, 37, row0=5, rows=20) as s:  # a strip
        with pytest.raises(golhip.GolHipError) as e:
            s.set_pad_step(1)
        assert e.value.code == golhip.GOLHIP_EINVAL
    with golhip.Board(100, 37) as r:  # a ring, even of one rank
        r.comm_init(golhip.unique_id(), 1, 0)
        with pytest.raises(golhip.GolHipError) as e:
            r.set_pad_step(1)
        assert e.value.code == golhip.GOLHIP_EINVAL
    with golhip.Board(100, 37) as b:
        for bad in (-2, 2):
            with pytest.raises(golhip.GolHipError):
                b.set_pad_step(bad)
        b.set_pad_step(1)
        b.comm_init(golhip.unique_id(), 1, 0)  # a ring after the switch: its steps keep the any-width kernel
        b.load_bytes(soup(100, 37, 4))
        b.step(3)
        assert b.perf()["pad_launches"] == 0
        assert np.array_equal(b.snapshot_bytes(), truth(100, 37, 4, 3))


# ---------------------------------------------------------------- callers through the hook
def test_view_stream_through_the_hook():
    """golhip_view_stream steps through the same hook: frames and the final board equal the oracle's."""
    W, H = 100, 37
    with golhip.Board(W, H) as b:
        b.set_pad_step(1)
        b.load_bytes(soup(W, H, 8))
        frames, done = b.view_stream(60, 20, fmt=golhip.VIEW_GRAY8)
        assert done == 60 and frames.shape == (3, H, W)
        for i, t in enumerate((20, 40, 60)):
            assert np.array_equal(frames[i], truth(W, H, 8, t)), t
        check_board(b, truth(W, H, 8, 60), 60, "view")
        assert b.perf()["pad_launches"] == 3


def test_run_headless_100x100x300(tmp_path):
    """gol.Run's 256-turn batches (no cell events) of a 100 x 100 board: the final PGM is the oracle's board."""
    board = soup(100, 100, 9)
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / "100x100.pgm").write_bytes(pgm_bytes(board))
    r = golhip.Run(300, 8, 100, 100, str(tmp_path), cell_events=False)
    counts, last, final_alive, _, _ = r.drain()
    assert r.wait() == ""
    r.close()
    want = truth(100, 100, 9, 300)
    assert counts["FinalTurnComplete"] == 1 and last == 300 and final_alive == alive(want)
    assert np.array_equal(read_pgm(str(tmp_path / "out" / "100x100x300.pgm"), 100, 100), want)
