"""gol.Run on row strips with cell events on a non-square board: 1024 x 300
on GOL_STRIPS=4, and 1024 x 302, whose strips are unequal (75/76/75/76 rows).

The mirror's strips branch is one golhip_group_flip_stream a batch; the
per-turn CellFlipped lists and the final board must equal the oracle's
(distributor.go:212-220, :186-191).  tests/test_gpu_run.py's *_strips tests
cover the square fixtures 16 / 64 / 512.
"""
import numpy as np
import pytest

from oracle.oracle import COracle, flips_np, pgm_bytes, read_pgm, step_np

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")


@pytest.mark.parametrize("W,H", [(1024, 300), (1024, 302)])
def test_run_cell_events_on_four_strips(tmp_path, monkeypatch, W, H):
    monkeypatch.setenv("GOL_STRIPS", "4")
    monkeypatch.setenv("GOL_NGPU", "1")
    T = 30
    board = COracle().fill_random(W, H, 0x5EED00B0)
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / f"{W}x{H}.pgm").write_bytes(pgm_bytes(board))
    want, cur = [], board
    for _ in range(T):
        nxt = step_np(cur)
        want.append(flips_np(cur, nxt))
        cur = nxt
    r = golhip.Run(T, 8, W, H, str(tmp_path))
    flips = [[] for _ in range(T + 1)]  # [0]: the initial alive cells (turn 0)
    turns = 0
    for ev in r:
        if ev["type"] == "CellFlipped":
            flips[ev["CompletedTurns"]].append(tuple(ev["Cell"]))
        elif ev["type"] == "TurnComplete":
            turns += 1
            assert ev["CompletedTurns"] == turns
    assert r.wait() == ""
    r.close()
    assert turns == T
    ys, xs = np.nonzero(board == 255)
    assert sorted(flips[0]) == sorted(zip(xs.tolist(), ys.tolist()))
    for t in range(T):  # the CellFlipped of turn t + 1 precede its TurnComplete, in row-major order
        assert flips[t + 1] == list(map(tuple, want[t].tolist())), t
    out = read_pgm(str(tmp_path / "out" / f"{W}x{H}x{T}.pgm"), W, H)
    assert np.array_equal(out, cur)
