"""The live view behind gol.Run (golrun_start_view / golrun_view_frame, the
host mirror's RunOptions::view) and golrun's -viewScale: the reference's
TestSdl (sdl_test.go:93-128) with the window's pixels taken from the device
frame instead of a shadow board fed by CellFlipped."""
import os
import subprocess
import time

import numpy as np
import pytest

from oracle.oracle import pack_bits, pgm_bytes, run_np, unpack_bits

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "game-of-life-distributed_amd",
                   "golhip", "golrun")


@pytest.fixture()
def root(tmp_path, fixtures):
    img = tmp_path / "images"
    img.mkdir()
    for n in (64, 512):
        (img / f"{n}x{n}.pgm").write_bytes(pgm_bytes(unpack_bits(fixtures[f"image_{n}"], n)))
    return tmp_path


def test_sdl_from_the_view(root, fixtures):
    """512^2 x 100, no cell events, a frame every turn, unbuffered events: at
    TurnComplete{t} the fetched frame shows a turn ft >= t with alive_512[ft]
    white pixels; after FinalTurnComplete it is check/images/512x512x100."""
    alive = fixtures["alive_512"]
    r = golhip.Run(100, 8, 512, 512, str(root), cell_events=False, view=dict(scale=1, every=1))
    turns, final, first = 0, False, True
    for ev in r:
        if first:  # turn 0's frame is there before the first event
            frame, ft = r.view_frame()
            assert ft >= 0 and int((frame == 0xFFFFFFFF).sum()) == alive[ft]
            first = False
        if ev["type"] == "TurnComplete":
            turns += 1
            t = ev["CompletedTurns"]
            assert t == turns
            frame, ft = r.view_frame()
            assert t <= ft <= 100, (t, ft)
            assert int((frame == 0xFFFFFFFF).sum()) == alive[ft], (t, ft)
        elif ev["type"] == "FinalTurnComplete":
            final = True
            frame, ft = r.view_frame()
            assert ft == 100
            assert np.array_equal(frame, golhip.view_frame_np(fixtures["check_512x100"], 512, 512))
    assert r.wait() == "" and final and turns == 100
    frame, ft = r.view_frame()  # the last frame outlives the run
    assert ft == 100 and int((frame == 0xFFFFFFFF).sum()) == alive[100]
    r.close()


def test_view_with_cell_events(root, fixtures):
    """Cell events keep the flip stream; frames are rendered between its
    batches, which end on the frame turns (every = 3 of 10 turns, then the
    final board)."""
    board0 = unpack_bits(fixtures["image_64"], 64)
    r = golhip.Run(10, 4, 64, 64, str(root), view=dict(scale=2, every=3, fmt=golhip.VIEW_GRAY8))
    seen = {}
    for ev in r:
        if ev["type"] in ("TurnComplete", "FinalTurnComplete"):
            frame, ft = r.view_frame()
            # turn 10 is no frame turn: its TurnComplete still sees turn 9's frame
            assert ft >= min(ev["CompletedTurns"], 9) and (ft % 3 == 0 or ft == 10)
            assert ft == 10 or ev["type"] == "TurnComplete"
            seen[ft] = frame
    assert r.wait() == ""
    r.close()
    assert sorted(seen) == [3, 6, 9, 10]
    for t, frame in seen.items():
        assert np.array_equal(frame, golhip.view_frame_np(pack_bits(run_np(board0, t)), 64, 64, scale=2,
                                                          fmt=golhip.VIEW_GRAY8)), t


def test_pause_holds_the_frame(root):
    r = golhip.Run(100000000, 4, 64, 64, str(root), keys=True, cell_events=False, view=dict(scale=1))
    r.send_key("p")
    paused_at = None
    while True:  # up to the pause, then whatever the finished batch still sends
        ev = r.next(timeout_ms=2000 if paused_at is None else 300)
        assert ev is not None
        if ev == "timeout":
            assert paused_at is not None, "no Paused event"
            break
        if ev["type"] == "StateChange" and ev["NewState"] == golhip.PAUSED:
            paused_at = ev["CompletedTurns"]
    frame, ft = r.view_frame()
    assert ft == paused_at
    time.sleep(0.2)
    again, ft2 = r.view_frame()
    assert ft2 == paused_at and np.array_equal(again, frame)
    r.send_key("p")
    r.send_key("q")
    for _ in r:
        pass
    assert r.wait() == ""
    r.close()


def test_view_refuses_strips(root, monkeypatch):
    monkeypatch.setenv("GOL_STRIPS", "2")
    r = golhip.Run(10, 4, 64, 64, str(root), cell_events=False, view=dict(scale=1))
    assert list(r) == []
    msg = r.wait()
    assert "live view" in msg and "2 strips" in msg and "GOL_STRIPS" in msg
    with pytest.raises(golhip.GolHipError):
        r.view_frame()
    r.close()


def test_cli_view_frames(root, fixtures):
    """golrun -viewScale 4 -viewEvery 2 over 4 turns: P5 frames of turns 0, 2
    and 4 of the whole board; without -viewScale, no view directory."""
    board0 = unpack_bits(fixtures["image_512"], 512)
    cmd = [CLI, "-noVis", "-w", "512", "-h", "512", "-turns", "4", "-root", str(root)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert not (root / "out" / "view").exists()
    res = subprocess.run(cmd + ["-viewScale", "4", "-viewEvery", "2"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    files = sorted(p.name for p in (root / "out" / "view").iterdir())
    assert files == ["view_512x512x0.pgm", "view_512x512x2.pgm", "view_512x512x4.pgm"]
    for t in (0, 2, 4):
        want = golhip.view_frame_np(pack_bits(run_np(board0, t)), 512, 512, scale=4, fmt=golhip.VIEW_GRAY8)
        assert (root / "out" / "view" / f"view_512x512x{t}.pgm").read_bytes() == pgm_bytes(want), t
    # -viewDir
    res = subprocess.run(cmd + ["-viewScale", "4", "-viewEvery", "4", "-viewDir", str(root / "frames")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert sorted(p.name for p in (root / "frames").iterdir()) == ["view_512x512x0.pgm", "view_512x512x4.pgm"]
