"""gol.Run with patterns (RunOptions::blank, patterns; golrun_opts_t
reserved[2..3]; golrun -blank -pattern): pattern files
stamped after the initial board is there and before any event.  The initial
CellFlipped events are the alive cells of the board after the stamps, and the
turns, FinalTurnComplete and the final PGM are the oracle's from that board.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import alive_cells_np, flips_np, pgm_bytes, run_np, step_np, unpack_bits

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

CLI = os.path.join(os.path.dirname(os.path.abspath(golhip.__file__)), "golrun")
GLIDER = "#N Glider\nx = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n"
N, T = 64, 8


@pytest.fixture()
def root(tmp_path, fixtures):
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / f"{N}x{N}.pgm").write_bytes(pgm_bytes(unpack_bits(fixtures[f"image_{N}"], N)))
    (tmp_path / "glider.rle").write_text(GLIDER)
    return tmp_path


def multiset(cells):
    return sorted(map(tuple, np.asarray(cells).reshape(-1, 2).tolist()))


def check_run(run, start, turns, root):
    """Every event of `run` against the oracle from the board `start`."""
    evs = [e for e in run if e["type"] != "AliveCellsCount"]
    assert run.wait() == ""
    run.close()
    boards = [start]
    for _ in range(turns):
        boards.append(step_np(boards[-1]))
    flips = {t: [] for t in range(turns + 1)}
    for e in evs:
        if e["type"] == "CellFlipped":
            flips[e["CompletedTurns"]].append(e["Cell"])
    # the initial events: exactly the alive cells of the board after the stamps
    assert multiset(flips[0]) == multiset(alive_cells_np(start))
    for t in range(1, turns + 1):
        assert multiset(flips[t]) == multiset(flips_np(boards[t - 1], boards[t])), t
    assert [e["CompletedTurns"] for e in evs if e["type"] == "TurnComplete"] == list(range(1, turns + 1))
    final = [e for e in evs if e["type"] == "FinalTurnComplete"]
    assert len(final) == 1 and final[0]["CompletedTurns"] == turns
    assert multiset(final[0]["Alive"]) == multiset(alive_cells_np(boards[-1]))
    assert (root / "out" / f"{N}x{N}x{turns}.pgm").read_bytes() == pgm_bytes(boards[-1])


@pytest.mark.parametrize("strips", [1, 2])
def test_blank_run_with_a_glider(root, monkeypatch, strips):
    monkeypatch.setenv("GOL_STRIPS", str(strips))
    monkeypatch.setenv("GOL_NGPU", "1")
    start = golhip.stamp_np(np.zeros((N, N), dtype=np.uint8), golhip.rle_parse_np(GLIDER), 1, 1, golhip.STAMP_OR)
    assert int(np.count_nonzero(start)) == 5
    os.remove(root / "images" / f"{N}x{N}.pgm")  # a blank run reads no image
    check_run(golhip.Run(T, 8, N, N, str(root), blank=True, patterns=[(str(root / "glider.rle"), 1, 1)]), start, T, root)


@pytest.mark.parametrize("strips", [1, 2])
def test_image_plus_patterns(root, fixtures, monkeypatch, strips):
    """Stamped in order: a PGM block copied over the image, then the glider XORed across both seams."""
    monkeypatch.setenv("GOL_STRIPS", str(strips))
    monkeypatch.setenv("GOL_NGPU", "1")
    block = np.zeros((10, 12), dtype=np.uint8)
    block[2:4, 3:9] = 255
    (root / "block.pgm").write_bytes(pgm_bytes(block))
    start = unpack_bits(fixtures[f"image_{N}"], N)
    start = golhip.stamp_np(start, block, 28, 27, golhip.STAMP_COPY)
    start = golhip.stamp_np(start, golhip.rle_parse_np(GLIDER), 62, 63, golhip.STAMP_XOR)
    run = golhip.Run(T, 8, N, N, str(root), patterns=[(str(root / "block.pgm"), 28, 27, "copy"),
                                                      (str(root / "glider.rle"), 62, 63, golhip.STAMP_XOR)])
    check_run(run, start, T, root)


def refused(run, root):
    assert list(run) == []  # no event
    msg = run.wait()
    run.close()
    assert not os.path.exists(root / "out")
    return msg


def test_resume_refuses_patterns(root, fixtures):
    ck = str(root / "at5.ckpt")
    golhip.checkpoint_write_np(ck, fixtures[f"image_{N}"], N, N, 5)
    pat = [(str(root / "glider.rle"), 1, 1)]
    assert "must not stamp twice" in refused(golhip.Run(T, 8, N, N, str(root), resume=ck, patterns=pat), root)
    assert "must not stamp twice" in refused(golhip.Run(T, 8, N, N, str(root), resume=ck, blank=True), root)


def test_bad_patterns_end_the_run_before_any_event(root):
    glider = str(root / "glider.rle")
    (root / "bad.rle").write_text("x = 3, y = 3, rule = B36/S23\nbob$2bo$3o!\n")
    (root / "wide.rle").write_text(f"x = {N + 1}, y = 1\n{N + 1}o!\n")
    cases = [([(str(root / "none.rle"), 1, 1)], "no such file"),
             ([(glider, 1, 1), (str(root / "bad.rle"), 1, 1)], "not Conway's"),
             ([(str(root / "wide.rle"), 0, 0)], "does not fit"),
             ([(glider, N, 0)], "not on the")]
    for pats, msg in cases:
        assert msg in refused(golhip.Run(T, 8, N, N, str(root), blank=True, patterns=pats), root), msg
    with pytest.raises(golhip.GolHipError) as e:  # a spec that does not parse fails the start itself
        golhip.Run(T, 8, N, N, str(root), blank=True, patterns=[(glider, 1, 1, "and")])
    assert "unknown op" in str(e.value)


def test_cli_blank_and_pattern(root):
    start = golhip.stamp_np(np.zeros((N, N), dtype=np.uint8), golhip.rle_parse_np(GLIDER), 62, 1, golhip.STAMP_OR)
    start = golhip.stamp_np(start, golhip.rle_parse_np(GLIDER), 62, 1, golhip.STAMP_XOR)  # gone again
    start = golhip.stamp_np(start, golhip.rle_parse_np(GLIDER), 30, 62, golhip.STAMP_OR)
    glider = str(root / "glider.rle")
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), "-blank",
                          "-pattern", f"{glider}@62,1", "-pattern", f"{glider}@62,1,xor", f"-pattern={glider}@30,62,or"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert (root / "out" / f"{N}x{N}x{T}.pgm").read_bytes() == pgm_bytes(run_np(start, T))


@pytest.mark.parametrize("spec,msg", [("{g}@1", "bad position"), ("{g}@1,x", "bad position"), ("{g}", "no path@"),
                                      ("{g}@1,1,nand", "unknown op"), ("{r}/none.rle@1,1", "no such file")])
def test_cli_bad_spec(root, spec, msg):
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), "-blank",
                          "-pattern", spec.format(g=root / "glider.rle", r=root)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and msg in res.stderr, res.stderr
    assert not os.path.exists(root / "out")
