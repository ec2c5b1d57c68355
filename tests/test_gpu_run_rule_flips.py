"""gol.Run with the flip streams of a Life-like rule on the fused turn + list
kernel: Run(..., rule="B36/S23", rule_flips=True), GOL_RULE_FLIPS=1 and
golrun -ruleFlips.  64 x 64 x 50 turns of HighLife from the golden 64 x 64
image with cell events on: the CellFlipped events of every turn and the final
board against golhip.life_like_np, the same events as without it.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import alive_cells_np, flips_np, pgm_bytes, unpack_bits

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

CLI = os.path.join(os.path.dirname(os.path.abspath(golhip.__file__)), "golrun")
N, T = 64, 50
RULE = "B36/S23"
_boards = {}


def boards(fixtures):
    """The model's HighLife boards of turns 0..T, computed once."""
    if not _boards:
        b = [unpack_bits(fixtures[f"image_{N}"], N)]
        masks = golhip.rule_parse(RULE)
        for _ in range(T):
            b.append(golhip.life_like_np(b[-1], *masks, 1))
        for x in b:
            x.setflags(write=False)
        _boards["b"] = b
    return _boards["b"]


@pytest.fixture()
def root(tmp_path, fixtures):
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / f"{N}x{N}.pgm").write_bytes(pgm_bytes(unpack_bits(fixtures[f"image_{N}"], N)))
    return tmp_path


def cells(events, turn):
    return sorted(tuple(e["Cell"]) for e in events if e["type"] == "CellFlipped" and e["CompletedTurns"] == turn)


def check_run(run, root, b):
    evs = [e for e in run if e["type"] != "AliveCellsCount"]
    assert run.wait() == ""
    run.close()
    by_turn = {t: [] for t in range(T + 1)}
    for e in evs:
        if e["type"] == "CellFlipped":
            by_turn[e["CompletedTurns"]].append(e)
    assert len(by_turn[0]) == len(alive_cells_np(b[0]))
    for t in range(1, T + 1):
        want = sorted(map(tuple, flips_np(b[t - 1], b[t]).tolist()))
        assert len(by_turn[t]) == len(want), t
        assert cells(by_turn[t], t) == want, t
    assert [e["CompletedTurns"] for e in evs if e["type"] == "TurnComplete"] == list(range(1, T + 1))
    final = [e for e in evs if e["type"] == "FinalTurnComplete"]
    assert len(final) == 1 and final[0]["CompletedTurns"] == T
    assert sorted(map(tuple, np.asarray(final[0]["Alive"]).reshape(-1, 2).tolist())) == \
        sorted(map(tuple, alive_cells_np(b[T]).tolist()))
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(b[T])


@pytest.mark.parametrize("strips", [1, 3])
def test_run_rule_flips(root, fixtures, monkeypatch, strips):
    monkeypatch.setenv("GOL_STRIPS", str(strips))
    monkeypatch.setenv("GOL_NGPU", "1")
    monkeypatch.delenv("GOL_RULE_FLIPS", raising=False)
    check_run(golhip.Run(T, 8, N, N, str(root), rule=RULE, rule_flips=True), root, boards(fixtures))


def test_run_rule_flips_from_the_environment(root, fixtures, monkeypatch):
    monkeypatch.setenv("GOL_RULE_FLIPS", "1")
    check_run(golhip.Run(T, 8, N, N, str(root), rule=RULE), root, boards(fixtures))


def test_cli_rule_flips(root, fixtures):
    b = boards(fixtures)
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), "-rule", RULE,
                          "-ruleFlips"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(b[T])
