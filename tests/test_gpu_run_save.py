"""gol.Run with saved patterns (RunOptions::save_rle, GOLRUN_FLAG_SAVE_RLE,
golrun -saveRle, GOL_SAVE_RLE=1): beside the final image and
the images of `s` and `q` the run writes out/<W>x<H>x<turn>.rle, the alive box
of the board, complete before that image's ImageOutputComplete is sent.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.oracle import run_np

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "game-of-life-distributed_amd",
                   "golhip", "golrun")
N, T = 64, 8
GLIDER = "#N Glider\nx = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n"
AT = (61, 62)  # eight turns carry the glider two cells down and right: across both seams


@pytest.fixture()
def root(tmp_path):
    (tmp_path / "glider.rle").write_text(GLIDER)
    return tmp_path


def model(turns=T):
    start = golhip.stamp_np(np.zeros((N, N), dtype=np.uint8), golhip.rle_parse_np(GLIDER), *AT, golhip.STAMP_OR)
    return run_np(start, turns)


def check_file(path, board, turn):
    """The file is the model's alive box: Pos, Gen, size and cells."""
    text = open(path).read()
    box = golhip.alive_box_np(board)
    m = re.match(r"#CXRLE Pos=(\d+),(\d+) Gen=(\d+)\nx = (\d+), y = (\d+), rule = B3/S23\n", text)
    assert m and tuple(int(v) for v in m.groups()) == (box[0], box[1], turn, box[2], box[3]), text
    assert np.array_equal(golhip.rle_parse_np(text), golhip.extract_np(board, *box))
    assert np.array_equal(golhip.pattern_read(path), golhip.extract_np(board, *box))


@pytest.mark.parametrize("strips", [1, 2])
@pytest.mark.parametrize("how", ["argument", "environment"])
def test_final_rle(root, monkeypatch, strips, how):
    monkeypatch.setenv("GOL_STRIPS", str(strips))
    monkeypatch.setenv("GOL_NGPU", "1")
    if how == "environment":
        monkeypatch.setenv("GOL_SAVE_RLE", "1")
    rle = root / "out" / f"{N}x{N}x{T}.rle"
    r = golhip.Run(T, 8, N, N, str(root), blank=True, patterns=[(root / "glider.rle", *AT)],
                   save_rle=how == "argument")
    seen = []
    for ev in r:
        if ev["type"] == "ImageOutputComplete":
            # the file exists, whole, before the image's event arrives
            seen.append((ev["CompletedTurns"], rle.exists(), rle.read_text().endswith("!\n")))
    assert r.wait() == ""
    r.close()
    assert seen == [(T, True, True)]
    board = model()
    assert golhip.alive_box_np(board) == (63, 0, 3, 3)  # the glider lies across the x seam
    check_file(str(rle), board, T)
    assert sorted(os.listdir(root / "out")) == [f"{N}x{N}x{T}.pgm", f"{N}x{N}x{T}.rle"]


@pytest.mark.parametrize("quirks", [False, True])
def test_key_q_rle(root, quirks):
    """`q`: the .rle of the turn the run stops at, never transposed."""
    r = golhip.Run(100000000, 4, N, N, str(root), keys=True, cell_events=False, turn_events=False, quirks=quirks,
                   blank=True, patterns=[(root / "glider.rle", *AT)], save_rle=True)
    r.send_key("q")
    out = []
    for ev in r:
        if ev["type"] == "ImageOutputComplete":
            out.append((ev["CompletedTurns"], os.path.exists(root / "out" / f"{ev['Filename']}.rle")))
    assert r.wait() == ""
    r.close()
    assert len(out) == 1 and out[0][1]
    t = out[0][0]
    # (a glider's period is 4 turns and a lap of the diagonal 4 * 64: the model needs t mod 256 turns)
    board = model(t % 256)
    path = str(root / "out" / f"{N}x{N}x{t}.rle")
    text = open(path).read()
    box = golhip.alive_box_np(board)
    assert text.startswith(f"#CXRLE Pos={box[0]},{box[1]} Gen={t}\nx = 3, y = 3, rule = B3/S23\n")
    assert np.array_equal(golhip.pattern_read(path), golhip.extract_np(board, *box))


@pytest.mark.parametrize("stream", [False, True])
def test_key_s_rle(root, stream):
    """`s` behind TurnComplete{10}: the .rle of that image's turn is there before
    its ImageOutputComplete, with streamed images too; the final one follows."""
    turns = 3000
    r = golhip.Run(turns, 4, N, N, str(root), keys=True, blank=True, patterns=[(root / "glider.rle", *AT)],
                   save_rle=True, stream_images=stream)
    got, sent = [], False
    for ev in r:
        if ev["type"] == "TurnComplete" and ev["CompletedTurns"] == 10 and not sent:
            r.send_key("s")
            sent = True
        if ev["type"] == "ImageOutputComplete":
            got.append((ev["CompletedTurns"], os.path.exists(root / "out" / f"{ev['Filename']}.rle")))
    assert r.wait() == ""
    r.close()
    assert len(got) == 2 and got[1] == (turns, True) and got[0][1], got
    t = got[0][0]
    assert 10 <= t < turns
    for at in (t, turns):
        check_file(str(root / "out" / f"{N}x{N}x{at}.rle"), model(at % 256), at)
    assert not [p for p in os.listdir(root / "out") if p.endswith(".tmp")]


def test_cli_save_rle(root):
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), "-blank",
                          "-pattern", f"{root / 'glider.rle'}@{AT[0]},{AT[1]}", "-saveRle"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert f"File {N}x{N}x{T}.rle output done!" in res.stdout
    check_file(str(root / "out" / f"{N}x{N}x{T}.rle"), model(), T)


def test_no_switch_no_file(root):
    r = golhip.Run(T, 8, N, N, str(root), blank=True, patterns=[(root / "glider.rle", *AT)])
    list(r)
    assert r.wait() == ""
    r.close()
    assert sorted(os.listdir(root / "out")) == [f"{N}x{N}x{T}.pgm"]


def test_empty_board_writes_none(root):
    r = golhip.Run(T, 8, N, N, str(root), blank=True, save_rle=True)
    assert [e["CompletedTurns"] for e in r if e["type"] == "ImageOutputComplete"] == [T]
    assert r.wait() == ""
    r.close()
    assert sorted(os.listdir(root / "out")) == [f"{N}x{N}x{T}.pgm"]
    # the command line says so, once
    res = subprocess.run([CLI, "-noVis", "-w", str(N), "-h", str(N), "-turns", str(T), "-root", str(root), "-blank",
                          "-saveRle"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout.count(f"File {N}x{N}x{T}.rle not written: the board is empty") == 1
    assert sorted(os.listdir(root / "out")) == [f"{N}x{N}x{T}.pgm"]
