"""gol.Run on a bounded plane: Run(..., plane=True), golrun -plane and
golrun -rule B3/S23:P64,64.  64 x 64 x 20 turns of Conway's rule from a PGM
whose border ring is alive (on the torus the ring's sides touch across the
seams), on one handle and on GOL_STRIPS=2; every event and the out PGM against
golhip.life_like_plane_np.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import alive_cells_np, flips_np, pgm_bytes

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

CLI = os.path.join(os.path.dirname(os.path.abspath(golhip.__file__)), "golrun")
N, T = 64, 20
_boards = {}


def start():
    b = np.zeros((N, N), np.uint8)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = 255
    b[20:23, 30:33] = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8) * np.uint8(255)
    return b


def boards():
    """The plane model's boards of turns 0..T, computed once."""
    if not _boards:
        b = [start()]
        for _ in range(T):
            b.append(golhip.life_like_plane_np(b[-1], *golhip.CONWAY, 1))
        for x in b:
            x.setflags(write=False)
        _boards["b"] = b
    return _boards["b"]


@pytest.fixture()
def root(tmp_path):
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / f"{N}x{N}.pgm").write_bytes(pgm_bytes(start()))
    return tmp_path


def multiset(cells):
    return sorted(map(tuple, np.asarray(cells).reshape(-1, 2).tolist()))


def test_the_ring_tells_the_plane_from_the_torus():
    b = boards()
    for t in (1, T):
        assert not np.array_equal(b[t], golhip.life_like_np(b[0], *golhip.CONWAY, t))


@pytest.mark.parametrize("how", ["argument", "environment"])
@pytest.mark.parametrize("strips", [1, 2])
def test_run_plane(root, monkeypatch, strips, how):
    monkeypatch.setenv("GOL_STRIPS", str(strips))
    monkeypatch.setenv("GOL_NGPU", "1")
    if how == "environment":
        monkeypatch.setenv("GOL_PLANE", "1")
    else:
        monkeypatch.delenv("GOL_PLANE", raising=False)
    b = boards()
    run = golhip.Run(T, 8, N, N, str(root), plane=(how == "argument"), ticker_ms=1)
    evs = list(run)
    assert run.wait() == ""
    run.close()
    flips = {t: 0 for t in range(T + 1)}
    for e in evs:
        if e["type"] == "CellFlipped":
            flips[e["CompletedTurns"]] += 1
        if e["type"] == "AliveCellsCount":
            assert e["CellsCount"] == int((b[e["CompletedTurns"]] == 255).sum()), e
    assert flips[0] == len(alive_cells_np(b[0]))
    assert [flips[t] for t in range(1, T + 1)] == [len(flips_np(b[t - 1], b[t])) for t in range(1, T + 1)]
    assert [e["CompletedTurns"] for e in evs if e["type"] == "TurnComplete"] == list(range(1, T + 1))
    final = [e for e in evs if e["type"] == "FinalTurnComplete"]
    assert len(final) == 1 and final[0]["CompletedTurns"] == T
    assert multiset(final[0]["Alive"]) == multiset(alive_cells_np(b[T]))
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(b[T])


def test_run_without_plane_is_the_torus(root, monkeypatch):
    monkeypatch.delenv("GOL_PLANE", raising=False)
    run = golhip.Run(T, 8, N, N, str(root), cell_events=False, turn_events=False)
    for _ in run:
        pass
    assert run.wait() == ""
    run.close()
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(golhip.life_like_np(start(), *golhip.CONWAY, T))


def test_run_plane_saves_bounded_rle(root, monkeypatch):
    monkeypatch.delenv("GOL_PLANE", raising=False)
    run = golhip.Run(T, 8, N, N, str(root), plane=True, rule="B36/S23", save_rle=True, cell_events=False)
    for _ in run:
        pass
    assert run.wait() == ""
    run.close()
    want = golhip.life_like_plane_np(start(), *golhip.rule_parse("B36/S23"), T)
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(want)
    text = (root / "out" / f"{N}x{N}x{T}.rle").read_text()
    assert f", rule = B36/S23:P{N},{N}\n" in text


@pytest.mark.parametrize("args", [["-plane"], ["-rule", f"B3/S23:P{N},{N}"], [f"-rule=b3/s23:p{N},{N}"]])
def test_cli_plane(root, args, monkeypatch):
    monkeypatch.delenv("GOL_PLANE", raising=False)
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), *args],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(boards()[T])


def test_cli_torus_suffix_is_the_torus(root, monkeypatch):
    monkeypatch.delenv("GOL_PLANE", raising=False)
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root),
                          "-rule", f"B3/S23:T{N},{N}"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(golhip.life_like_np(start(), *golhip.CONWAY, T))


@pytest.mark.parametrize("args,plane", [
    (["-rule", f"B3/S23:P{N},{N}", "-rule", "B3/S23"], False),     # the last -rule counts, suffix included
    (["-rule", "B3/S23", "-rule", f"B3/S23:P{N},{N}"], True),
    (["-plane", "-rule", "B3/S23"], True),                           # -plane is not -rule's to undo
    (["-rule", f"B3/S23:P{N},{N}", "-plane=false"], False),          # and wins over a suffix
])
def test_cli_last_rule_decides(root, args, plane, monkeypatch):
    monkeypatch.delenv("GOL_PLANE", raising=False)
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), *args],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    want = boards()[T] if plane else golhip.life_like_np(start(), *golhip.CONWAY, T)
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(want)


@pytest.mark.parametrize("args,msg", [
    (["-w", "128", "-h", str(N), "-rule", f"B3/S23:P{N},{N}"], f"the bounds {N} x {N} are not the board's 128 x {N}"),
    (["-rule", f"B3/S23:P{N},{N}", "-w", "128", "-h", str(N)], f"the bounds {N} x {N} are not the board's 128 x {N}"),
    (["-w", str(N), "-h", str(N), "-rule", f"B3/S23:P0,{N}"], "bounded width 0"),
    (["-w", str(N), "-h", str(N), "-rule", f"B3/S23:P{N}"], "no ','"),
])
def test_cli_bad_bounds(root, args, msg):
    res = subprocess.run([CLI, "-noVis", "-turns", str(T), "-root", str(root), *args], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode != 0 and msg in res.stderr, res.stderr
    assert "TurnComplete" not in res.stdout and not os.path.exists(root / "out")
