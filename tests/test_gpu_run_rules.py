"""gol.Run on another Life-like rule than Conway's: Run(..., rule="B36/S23"),
golrun -rule.  64 x 64 x 50 turns of HighLife from the golden 64 x 64 image,
with cell events (the flip streams, one rule-kernel turn at a time) and
without, on one handle and on GOL_STRIPS=3; every event and the out PGM
against golhip.life_like_np.
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


def multiset(cells):
    return sorted(map(tuple, np.asarray(cells).reshape(-1, 2).tolist()))


@pytest.mark.parametrize("strips", [1, 3])
@pytest.mark.parametrize("cell_events", [True, False])
def test_run_highlife(root, fixtures, monkeypatch, strips, cell_events):
    monkeypatch.setenv("GOL_STRIPS", str(strips))
    monkeypatch.setenv("GOL_NGPU", "1")
    b = boards(fixtures)
    assert not np.array_equal(b[T], golhip.life_like_np(b[0], *golhip.CONWAY, T))  # the rule matters on this board
    run = golhip.Run(T, 8, N, N, str(root), rule=RULE, cell_events=cell_events)
    evs = [e for e in run if e["type"] != "AliveCellsCount"]
    assert run.wait() == ""
    run.close()
    flips = {t: 0 for t in range(T + 1)}
    for e in evs:
        if e["type"] == "CellFlipped":
            flips[e["CompletedTurns"]] += 1
    if cell_events:
        assert flips[0] == len(alive_cells_np(b[0]))
        assert [flips[t] for t in range(1, T + 1)] == [len(flips_np(b[t - 1], b[t])) for t in range(1, T + 1)]
    else:
        assert sum(flips.values()) == 0
    assert [e["CompletedTurns"] for e in evs if e["type"] == "TurnComplete"] == list(range(1, T + 1))
    final = [e for e in evs if e["type"] == "FinalTurnComplete"]
    assert len(final) == 1 and final[0]["CompletedTurns"] == T
    assert multiset(final[0]["Alive"]) == multiset(alive_cells_np(b[T]))
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(b[T])


def test_run_rule_as_masks_and_conway(root, fixtures):
    """(birth, survive) masks spell the rule too; Conway's is the plain run."""
    b = boards(fixtures)
    for rule, want in ((golhip.rule_parse(RULE), b[T]), ("B3/S23", golhip.life_like_np(b[0], *golhip.CONWAY, T))):
        run = golhip.Run(T, 8, N, N, str(root), rule=rule, cell_events=False, turn_events=False)
        for _ in run:
            pass
        assert run.wait() == ""
        run.close()
        assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(want)
    with pytest.raises(golhip.GolHipError, match="digit 9"):
        golhip.Run(T, 8, N, N, str(root), rule="B39/S23")


def test_run_patterns_follow_the_rule(root, fixtures):
    """-pattern files on a HighLife run: of that rule or of none; a B3/S23 file
    ends the run before any event, as a B36/S23 file ends a Conway run."""
    (root / "hl.rle").write_text("x = 3, y = 3, rule = B36/S23\nbob$2bo$3o!\n")
    (root / "plain.rle").write_text("x = 3, y = 3\nbob$2bo$3o!\n")
    (root / "conway.rle").write_text("x = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n")
    glider = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8) * np.uint8(255)
    start = golhip.stamp_np(np.zeros((N, N), np.uint8), glider, 5, 6, golhip.STAMP_OR)
    start = golhip.stamp_np(start, glider, 40, 41, golhip.STAMP_OR)
    run = golhip.Run(8, 8, N, N, str(root), rule=RULE, blank=True, cell_events=False,
                     patterns=[(str(root / "hl.rle"), 5, 6), (str(root / "plain.rle"), 40, 41)])
    for _ in run:
        pass
    assert run.wait() == ""
    run.close()
    want = golhip.life_like_np(start, *golhip.rule_parse(RULE), 8)
    assert (root / "out" / f"{N}x{N}x8.pgm").read_bytes() == pgm_bytes(want)
    os.remove(root / "out" / f"{N}x{N}x8.pgm")
    os.rmdir(root / "out")
    for rule, name, msg in ((RULE, "conway.rle", "rule B3/S23 is not the board's B36/S23"),
                            (None, "hl.rle", "rule B36/S23 is not Conway's B3/S23")):
        run = golhip.Run(8, 8, N, N, str(root), rule=rule, blank=True, patterns=[(str(root / name), 1, 1)])
        assert list(run) == []
        assert msg in run.wait()
        run.close()
        assert not os.path.exists(root / "out")


def test_cli_rule(root, fixtures):
    b = boards(fixtures)
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), "-rule", RULE],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(b[T])


@pytest.mark.parametrize("rule,msg", [("B39/S23", "digit 9"), ("B3/S23/C3", "Generations"), ("life", "no '/'")])
def test_cli_bad_rule(root, rule, msg):
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), f"-rule={rule}"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and msg in res.stderr, res.stderr
    assert "TurnComplete" not in res.stdout and not os.path.exists(root / "out")
