"""GPU parity of the spaced pair-rule schedule (gol_kernels.hip unit_pr /
push_group_pr_hi) against the C oracle.

The schedule issues a row's lane shifts one unit ahead of the LUTs that use
them and carries the first row's shifts from group to group, from body to
body and into the pair drain.  (a) and (b) put single bits on every kind of
horizontal boundary those shifts carry a bit across, at every start row
modulo 6 (a body is two 3-row groups, KQ 0 and 1), on full and on half-wave
tiles; (c) steps a random board in three calls, so the carried state crosses
launches, bodies and the drain, and checks the alive count after each call.
Same options as run_skew in tests/test_gpu_skew.py with the pair rule on.
"""
import numpy as np
import pytest

from oracle.oracle import COracle

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

GLIDER = ((0, 1), (1, 2), (2, 0), (2, 1), (2, 2))  # moves +1 row, +1 column every 4 turns


@pytest.fixture(scope="module")
def coracle():
    return COracle()


def boundary_board(W, H, cols, regions):
    """An empty torus but for gliders (both horizontal directions), rows
    of four and blinkers at the boundary before each column of
    `cols`; in every region six sets, whose start rows cover every residue
    modulo 6."""
    b = np.zeros((H, W), dtype=np.uint8)

    def put(r, c):
        b[r % H, c % W] = 255

    for reg in regions:
        for i in range(6):
            base = reg + 61 * i  # 61 = 1 (mod 6)
            for c in cols:
                for dr, dc in GLIDER:  # from the left of the boundary, moving right across it
                    put(base + dr, c - 4 + dc)
                for dc in (-1, 0, 1):  # four in a row across the boundary c - 1 | c (settles into a beehive)
                    put(base + 20, c - 1 + dc)
                    put(base + 20, c + dc)
                for dr, dc in GLIDER:  # mirrored: from the right, moving left across it
                    put(base + 30 + dr, c + 3 - dc)
                for dr in (-1, 0, 1):  # standing blinkers on either side of the boundary
                    put(base + 50 + dr, c - 1)
                    put(base + 50 + dr, c + 2)
    return b


def open_board(board, **opts):
    H, W = board.shape
    b = golhip.Board(W, H)
    b.set_option("persistent", 0)
    b.set_option("skew", 2)
    b.set_option("wpl", 2)
    b.set_option("skew_pairs", 5)
    for k, v in opts.items():
        b.set_option(k, v)
    b.set_tb_depth(20)
    b.load_bytes(board)
    return b


# a lane holds 64 cells (two words: 31 | 32 inside it, 63 | 64 to the next
# lane); a full tile stores 62 lanes = 3968 cells, a half-wave tile 30 = 1920;
# column 0 is the torus seam (and the first tile's first stored lane)
@pytest.mark.parametrize("W,H,half,cols,regions", [
    (4096, 1206, 0, (0, 32, 64, 1952, 2016, 3968, 4000, 4032), (0, 400, 800)),
    (2048, 818, 1, (0, 32, 64, 992, 1024, 1920, 1952, 1984), (0, 410)),
])
def test_shift_bits_cross_every_boundary(coracle, W, H, half, cols, regions):
    board = boundary_board(W, H, cols, regions)
    turns = 2 * 18 + 5
    want = coracle.run(board, turns)
    assert (want == 255).sum() > 0
    with open_board(board, skew_half=1 if half else -1) as b:  # (by default the plan picks by wave-rows)
        b.step(turns)
        p = b.perf()
        got = b.snapshot_bytes()
        assert p["pair_launches"] >= 2 and p["tb_depth"] == 18, p
        assert (p["skew_half_launches"] >= 2) == bool(half), p
        assert b.alive_count() == (int((want == 255).sum()), turns)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} cells differ, first (row, column) {bad[:8].tolist()}"


@pytest.mark.parametrize("half", [-1, 1])
def test_state_carried_across_steps_and_drain(coracle, half):
    W, H = 4096, 1206
    board = coracle.fill_random(W, H, 0x5EED0151)
    with open_board(board, skew_half=half) as b:
        done, cur = 0, board
        for turns in (18, 18, 23):
            b.step(turns)
            cur = coracle.run(cur, turns)
            done += turns
            assert b.alive_count() == (int((cur == 255).sum()), done)
        p = b.perf()
        assert p["pair_launches"] >= 2 and (p["skew_half_launches"] >= 2) == (half == 1), p
        assert np.array_equal(b.snapshot_bytes(), cur)
