"""Padded strips without a GPU (golhip_group_set_pad_step):
the scheme restated in numpy (golhip.pad_group_run_np) against the plain torus.

* With the seam refresh over every row a launch reads ("window", the scheme)
  the strips' real columns equal the torus, on two and three uneven strips, for
  widths on both sides of a word and of a ghost's width.
* The controls of tests/test_gpu_pad_strips.py: the same schedule with the
  refresh kept to the strip's own rows ("own": the halo rows keep the
  neighbour's stale ghosts) or run before a round's first launch alone
  ("once") goes wrong, on boards whose ghosts are 33 / 32 columns deep, with
  the rounds golhip_halo_schedule plans for them.
* The Python, C and Go surface of golhip_group_set_pad_step.
"""
import os

import numpy as np
import pytest

from oracle.oracle import run_np

golhip = pytest.importorskip("golhip")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = [3, 17, 63, 65, 100, 127, 129]
# (W, H, cuts, tb_depth, turns, the rounds the engine plans, alive at the end, controls that must be wrong)
CONTROLS = [
    (63, 96, [0, 32, 64, 96], 16, 96, [(16, 2)] * 3, 549, ("own",)),
    (63, 96, [0, 32, 64, 96], 32, 96, [(32, 1)] * 3, 549, ("own",)),
    (127, 80, [0, 40, 80], 20, 100, [(20, 2), (20, 2), (20, 1)], 972, ("own", "once")),
]


def soup(W, H, seed, p=0.35):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((H, W)) < p, 255, 0).astype(np.uint8)


def rows_of(cuts):
    return [b - a for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("W", WIDTHS)
def test_window_refresh_equals_plain_torus(W):
    """Two and three uneven strips, launches of up to 32 turns, deep-halo rounds
    of more than one launch (tb_depth 8: k = 2 .. 3) and of one."""
    H = 75
    board = soup(W, H, 1000 * W + H)
    for cuts in ([0, 41, 75], [0, 19, 52, 75]):
        for tb, turns in ((32, 47), (8, 45)):
            rounds = golhip.group_halo_rounds(rows_of(cuts), tb, turns)
            assert sum(d * k for d, k in rounds) == turns and (tb == 32 or max(k for _, k in rounds) > 1), rounds
            got = golhip.pad_group_run_np(board, cuts, turns, rounds)
            assert np.array_equal(got, run_np(board, turns)), (W, cuts, rounds)


def test_one_strip_is_the_padded_torus():
    board = soup(100, 37, 5)
    rounds = golhip.group_halo_rounds([37], 16, 40)
    assert all(k == 1 for _, k in rounds)
    assert np.array_equal(golhip.pad_group_run_np(board, [0, 37], 40, rounds), run_np(board, 40))
    assert np.array_equal(golhip.pad_group_run_np(board, [0, 37], 40, rounds), golhip.pad_run_np(board, 40, 16))


@pytest.mark.parametrize("W,H,cuts,tb,turns,rounds,alive,wrong", CONTROLS)
def test_controls_are_wrong(W, H, cuts, tb, turns, rounds, alive, wrong):
    board = soup(W, H, 1000 * W + H)
    want = run_np(board, turns)
    assert int(np.count_nonzero(want == 255)) == alive > 0
    assert golhip.group_halo_rounds(rows_of(cuts), tb, turns) == rounds
    assert np.array_equal(golhip.pad_group_run_np(board, cuts, turns, rounds, "window"), want)
    for seam in ("own", "once"):
        same = np.array_equal(golhip.pad_group_run_np(board, cuts, turns, rounds, seam), want)
        assert same == (seam not in wrong), seam


def test_bad_arguments():
    board = soup(63, 8, 1)
    with pytest.raises(ValueError):
        golhip.pad_group_run_np(board, [0, 4, 8], 4, [(4, 1)], seam="never")
    with pytest.raises(ValueError):
        golhip.pad_group_run_np(board, [0, 4, 8], 5, [(4, 1)])
    with pytest.raises(ValueError):
        golhip.pad_group_run_np(board, [0, 4, 7], 4, [(4, 1)])
    with pytest.raises(ValueError):
        golhip.pad_group_run_np(board, [0, 4, 8], 8, [(4, 2)])  # 8 halo rows from a strip of 4


def test_python_c_and_go_surface():
    assert callable(golhip.group_set_pad_step)
    assert "golhip_group_set_pad_step" in golhip.header_symbols()
    lib = golhip.load()
    assert lib.golhip_group_set_pad_step(None, 1, 1) == golhip.GOLHIP_EINVAL  # refused before anything touches a device
    go = open(os.path.join(ROOT, "integration", "gol", "golhip.go")).read()
    assert "golhip_group_set_pad_step(golhip_t *hs, int32_t n, int32_t mode)" in go
