"""gol.Run with checkpoints and resume (RunOptions::checkpoint_path,
checkpoint_every, resume_path; golrun_start_opts): a run that writes
checkpoints sends the same events and the same final PGM as one that does
not, and a run resumed from a checkpoint continues as the uninterrupted run
does from that turn: initial CellFlipped of the checkpoint's board at its
turn, TurnComplete from T + 1, the same FinalTurnComplete and final PGM.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.oracle import alive_cells_np, pack_bits, pgm_bytes, read_pgm, run_np, unpack_bits

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

CLI = os.path.join(os.path.dirname(os.path.abspath(golhip.__file__)), "golrun")
T = 100


@pytest.fixture()
def root(tmp_path, fixtures):
    img = tmp_path / "images"
    img.mkdir()
    for n in (16, 64):
        (img / f"{n}x{n}.pgm").write_bytes(pgm_bytes(unpack_bits(fixtures[f"image_{n}"], n)))
    return tmp_path


def events_of(run):
    evs = [e for e in run if e["type"] != "AliveCellsCount"]
    assert run.wait() == ""
    run.close()
    return evs


def plain(e):
    d = dict(e)
    if "Alive" in d:
        d["Alive"] = sorted(map(tuple, d["Alive"].tolist()))
    return d


def multiset(cells):
    return sorted(map(tuple, np.asarray(cells).reshape(-1, 2).tolist()))


@pytest.mark.parametrize("n", [64, 16])
@pytest.mark.parametrize("cell_events", [True, False])
def test_periodic_then_resume(root, fixtures, monkeypatch, n, cell_events):
    start = unpack_bits(fixtures[f"image_{n}"], n)
    at80 = run_np(start, 80)
    base = events_of(golhip.Run(T, 8, n, n, str(root), cell_events=cell_events))
    final_pgm = (root / "out" / f"{n}x{n}x{T}.pgm").read_bytes()
    os.remove(root / "out" / f"{n}x{n}x{T}.pgm")

    # periodic: same events, same PGM; the file left is the board of turn 80
    ck = str(root / "run.ckpt")
    got = events_of(golhip.Run(T, 8, n, n, str(root), cell_events=cell_events, checkpoint=dict(path=ck, every=40)))
    assert list(map(plain, got)) == list(map(plain, base))
    assert (root / "out" / f"{n}x{n}x{T}.pgm").read_bytes() == final_pgm
    info, words = golhip.checkpoint_read_np(ck)
    assert info["turn"] == 80 and np.array_equal(unpack_bits(words, n), at80)
    assert not os.path.exists(ck + ".tmp")
    os.remove(root / "out" / f"{n}x{n}x{T}.pgm")

    # resume, on one strip and on three
    for strips in (None, "3"):
        if strips:
            monkeypatch.setenv("GOL_STRIPS", strips)
            monkeypatch.setenv("GOL_NGPU", "1")
        evs = events_of(golhip.Run(T, 8, n, n, str(root), cell_events=cell_events, resume=ck))
        first_tc = next(i for i, e in enumerate(evs) if e["type"] == "TurnComplete")
        assert evs[first_tc]["CompletedTurns"] == 81
        if cell_events:
            init = evs[:first_tc]
            flips80 = [e for e in init if e["type"] == "CellFlipped" and e["CompletedTurns"] == 80]
            assert multiset([e["Cell"] for e in flips80]) == multiset(alive_cells_np(at80))
            assert len(flips80) == int((at80 == 255).sum())
            assert not any(e["CompletedTurns"] < 80 for e in evs)
        else:
            assert first_tc == 0
        # from the first TurnComplete-81 batch on, the events are the uninterrupted run's
        i0 = next(i for i, e in enumerate(base) if e["CompletedTurns"] == 81)
        j0 = next(i for i, e in enumerate(evs) if e["CompletedTurns"] == 81)
        assert list(map(plain, evs[j0:])) == list(map(plain, base[i0:]))
        fin = [e for e in evs if e["type"] == "FinalTurnComplete"][0]
        assert fin["CompletedTurns"] == T
        assert multiset(fin["Alive"]) == multiset(alive_cells_np(unpack_bits(fixtures[f"check_{n}x{T}"], n)))
        assert (root / "out" / f"{n}x{n}x{T}.pgm").read_bytes() == final_pgm
        os.remove(root / "out" / f"{n}x{n}x{T}.pgm")


@pytest.mark.parametrize("resume", [False, True])
def test_view_stream_frames_stay_on_their_turns(root, fixtures, resume):
    """A view stream (cell events off, a frame behind every 7th turn) whose
    engine calls are cut at the checkpoint turns 40 and 80, or that starts at
    turn 80 from a checkpoint: every frame still shows a multiple of 7 (or the
    final board) and equals the oracle's board of that turn."""
    n = 64
    board0 = unpack_bits(fixtures[f"image_{n}"], n)
    ck = str(root / "view.ckpt")
    kw = dict(checkpoint=dict(path=ck, every=40))
    if resume:
        golhip.checkpoint_write_np(ck, pack_bits(run_np(board0, 80)), n, n, 80)
        kw = dict(resume=ck)
    r = golhip.Run(T, 8, n, n, str(root), cell_events=False, view=dict(scale=1, every=7, fmt=golhip.VIEW_GRAY8), **kw)
    seen = {}
    for ev in r:
        if ev["type"] in ("TurnComplete", "FinalTurnComplete"):
            frame, ft = r.view_frame()
            t = ev["CompletedTurns"]
            assert ft >= (t if t == T and ev["type"] == "FinalTurnComplete" else t // 7 * 7), (t, ft)
            seen[ft] = frame
    assert r.wait() == ""
    r.close()
    # (turn 80's frame is published at the start of the resumed run and may be
    # replaced by turn 84's before the first TurnComplete is received)
    assert sorted(set(seen) - {80}) == list(range(84 if resume else 0, T, 7)) + [T]
    for t, frame in seen.items():
        assert np.array_equal(frame, golhip.view_frame_np(pack_bits(run_np(board0, t)), n, n, fmt=golhip.VIEW_GRAY8)), t
    if not resume:
        assert golhip.checkpoint_info(ck)["turn"] == 80


def test_resume_at_the_last_turn(root, fixtures):
    n = 64
    want = unpack_bits(fixtures[f"check_{n}x{T}"], n)
    ck = str(root / "end.ckpt")
    golhip.checkpoint_write_np(ck, pack_bits(want), n, n, T)
    evs = events_of(golhip.Run(T, 8, n, n, str(root), cell_events=False, resume=ck))
    assert [e["type"] for e in evs] == ["ImageOutputComplete", "FinalTurnComplete", "StateChange"]
    assert evs[1]["CompletedTurns"] == T and multiset(evs[1]["Alive"]) == multiset(alive_cells_np(want))
    assert np.array_equal(read_pgm(str(root / "out" / f"{n}x{n}x{T}.pgm"), n, n), want)


def test_take_over_after_q(root, fixtures):
    n = 64
    ck = str(root / "q.ckpt")
    r = golhip.Run(1000000, 8, n, n, str(root), keys=True, cell_events=False, turn_events=False, ticker_ms=20,
                   checkpoint=dict(path=ck, every=0))
    ev = r.next(timeout_ms=10000)  # the run is under way
    assert ev not in (None, "timeout")
    r.send_key("q")
    rest = [ev] + list(r)
    assert r.wait() == ""
    r.close()
    out = [e for e in rest if e["type"] == "ImageOutputComplete"]
    assert len(out) == 1 and rest[-1]["type"] == "StateChange" and rest[-1]["NewState"] == golhip.QUITTING
    t = out[0]["CompletedTurns"]
    info, words = golhip.checkpoint_read_np(ck)  # complete before Quitting was sent
    assert info["turn"] == t
    at_t = read_pgm(str(root / "out" / f"{n}x{n}x{t}.pgm"), n, n)
    assert np.array_equal(unpack_bits(words, n), at_t)
    # a new controller takes over
    evs = events_of(golhip.Run(t + 25, 8, n, n, str(root), cell_events=False, resume=ck))
    tcs = [e["CompletedTurns"] for e in evs if e["type"] == "TurnComplete"]
    assert tcs == list(range(t + 1, t + 26))
    want = run_np(at_t, 25)
    fin = [e for e in evs if e["type"] == "FinalTurnComplete"][0]
    assert multiset(fin["Alive"]) == multiset(alive_cells_np(want))
    assert np.array_equal(read_pgm(str(root / "out" / f"{n}x{n}x{t + 25}.pgm"), n, n), want)


@pytest.mark.parametrize("case", ["size", "turn"])
def test_resume_refused(root, fixtures, case):
    n = 64
    ck = str(root / "bad.ckpt")
    if case == "size":
        golhip.checkpoint_write_np(ck, fixtures["image_16"], 16, 16, 5)
    else:
        golhip.checkpoint_write_np(ck, fixtures[f"image_{n}"], n, n, T + 1)
    r = golhip.Run(T, 8, n, n, str(root), resume=ck)
    assert list(r) == []
    msg = r.wait()
    r.close()
    assert ("Incorrect width" in msg) if case == "size" else (f"turn {T + 1}" in msg)
    assert not os.path.exists(root / "out")


def test_cli(root):
    n = 64
    ck = str(root / "cli.ckpt")
    common = [CLI, "-noVis", "-t", "4", "-w", str(n), "-h", str(n), "-turns", str(T), "-root", str(root)]
    assert subprocess.run(common, capture_output=True, text=True, timeout=120).returncode == 0
    pgm = root / "out" / f"{n}x{n}x{T}.pgm"
    want = pgm.read_bytes()
    os.remove(pgm)
    res = subprocess.run(common + ["-checkpoint", ck, "-checkpointEvery", "40"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    assert pgm.read_bytes() == want and golhip.checkpoint_info(ck)["turn"] == 80
    os.remove(pgm)
    res = subprocess.run(common + ["-resume", ck], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert pgm.read_bytes() == want
