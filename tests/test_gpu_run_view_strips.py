"""The live view behind gol.Run on row strips (GOL_STRIPS with the opt-in
switch: view=dict(strips=True), golrun -viewStrips / GOL_VIEW_STRIPS=1): the
frames are golhip_group_view_frame's and equal those of the run on one handle.
Without the switch such a run is still refused (test_gpu_run_view.py)."""
import os
import subprocess

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


def test_sdl_from_the_view_on_strips(root, fixtures, monkeypatch):
    """test_sdl_from_the_view on three strips (170 / 171 / 171 rows): at
    TurnComplete{t} the fetched frame shows a turn ft >= t with alive_512[ft]
    white pixels; after FinalTurnComplete it is check/images/512x512x100."""
    monkeypatch.setenv("GOL_STRIPS", "3")
    alive = fixtures["alive_512"]
    r = golhip.Run(100, 8, 512, 512, str(root), cell_events=False, view=dict(scale=1, every=1, strips=True))
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


def test_scale_5_over_three_strips(root, fixtures, monkeypatch):
    """64 x 64 as rows 21 / 21 / 22 at s = 5: pixel rows 4 and 8 straddle the
    strip boundaries.  Every frame seen is the oracle's of its turn, the last
    one turn 10's."""
    monkeypatch.setenv("GOL_STRIPS", "3")
    board0 = unpack_bits(fixtures["image_64"], 64)
    r = golhip.Run(10, 4, 64, 64, str(root), cell_events=False,
                   view=dict(scale=5, every=1, fmt=golhip.VIEW_GRAY8, strips=True))
    seen = {}
    for ev in r:
        if ev["type"] in ("TurnComplete", "FinalTurnComplete"):
            frame, ft = r.view_frame()
            assert ft >= ev["CompletedTurns"]
            seen[ft] = frame
    assert r.wait() == ""
    frame, ft = r.view_frame()
    r.close()
    assert ft == 10 and 10 in seen and frame.shape == (12, 12)
    seen[ft] = frame
    for t, f in seen.items():
        assert np.array_equal(f, golhip.view_frame_np(pack_bits(run_np(board0, t)), 64, 64, scale=5,
                                                      fmt=golhip.VIEW_GRAY8)), t


@pytest.mark.parametrize("switch", ["flag", "env"])
def test_cli_view_frames_on_strips(root, fixtures, switch):
    """golrun -viewScale 5 over 10 turns of 64 x 64: the PGM frames under
    GOL_STRIPS=3 with the switch are byte-equal to those of the same command
    without GOL_STRIPS (and are the oracle's)."""
    board0 = unpack_bits(fixtures["image_64"], 64)
    cmd = [CLI, "-noVis", "-w", "64", "-h", "64", "-turns", "10", "-root", str(root), "-viewScale", "5"]
    env = {k: v for k, v in os.environ.items() if k not in ("GOL_STRIPS", "GOL_NGPU", "GOL_VIEW_STRIPS")}
    res = subprocess.run(cmd + ["-viewDir", str(root / "one")], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stderr
    env["GOL_STRIPS"] = "3"
    if switch == "env":
        env["GOL_VIEW_STRIPS"] = "1"
    res = subprocess.run(cmd + ["-viewDir", str(root / "strips")] + (["-viewStrips"] if switch == "flag" else []),
                         capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0, res.stderr
    names = sorted(p.name for p in (root / "one").iterdir())
    assert names == sorted(f"view_64x64x{t}.pgm" for t in range(11))
    assert sorted(p.name for p in (root / "strips").iterdir()) == names
    for name in names:
        assert (root / "strips" / name).read_bytes() == (root / "one" / name).read_bytes(), name
    want = golhip.view_frame_np(pack_bits(run_np(board0, 10)), 64, 64, scale=5, fmt=golhip.VIEW_GRAY8)
    assert (root / "strips" / "view_64x64x10.pgm").read_bytes() == pgm_bytes(want)
