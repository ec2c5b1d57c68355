"""The live view on the GPU (golhip_view_frame / golhip_view_stream, K7 in
gol_view.hip) against its numpy restatement golhip.view_frame_np, bit-exact.

Each layout case fills a board, steps 3 turns (so the stepping layout and the
other ping-pong buffer are in play) and takes the expectation from the
snapshot path; the 512^2 fixture pins the stream against the reference's own
numbers (TestSdl, sdl_test.go:107-116: white pixels per turn == alive cells)
without going through a snapshot."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import fill_random_np, pack_bits, run_np, unpack_bits

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

SEED = 0x51EED
FORMATS = [golhip.VIEW_ARGB, golhip.VIEW_GRAY8]
SCALES = [1, 2, 3, 5, 32, 33, 64]

# board, option wpl (None: leave), perf words_per_lane that proves the layout
LAYOUTS = [
    pytest.param(16, 16, None, 0, id="generic-16x16"),
    pytest.param(48, 40, None, 0, id="generic-48x40"),
    pytest.param(96, 64, None, 1, id="canonical-96x64"),
    pytest.param(192, 96, 2, 2, id="pairs-192x96"),
    pytest.param(256, 128, 4, 4, id="quads-256x128"),
]


def viewports(W, H, s):
    """The full frame at the origin and a smaller one across both seams."""
    ow, oh = W // s, H // s
    yield 0, 0, ow, oh
    yield W - 7, H - 3, max(ow - 1, 1), max(oh - 1, 1)


@pytest.mark.parametrize("W,H,wpl,want_wpl", LAYOUTS)
def test_view_frame_every_layout(W, H, wpl, want_wpl):
    board0 = fill_random_np(W, H, SEED)
    with golhip.Board(W, H, timing=True) as b:
        if wpl is not None:
            b.set_option("wpl", wpl)
        b.fill_random(SEED)
        b.step(3)
        assert b.perf()["words_per_lane"] == want_wpl
        words = b.snapshot_bits()
        assert np.array_equal(unpack_bits(words, W), run_np(board0, 3))
        digest = b.board_hash()
        pinned = golhip.host_array((H, W), np.uint32)
        frames = 0
        for s in [s for s in SCALES if s <= min(W, H)]:
            for x0, y0, ow, oh in viewports(W, H, s):
                for fmt in FORMATS:
                    want = golhip.view_frame_np(words, W, H, x0, y0, s, ow, oh, fmt)
                    got, turn = b.view_frame(x0, y0, s, ow, oh, fmt)
                    assert turn == 3
                    assert got.dtype == want.dtype and np.array_equal(got, want), (s, x0, y0, fmt)
                    # the same frame written by the kernel itself into page-locked memory
                    out = pinned.reshape(-1).view(want.dtype)[: ow * oh]
                    out[:] = 0x5A
                    got, turn = b.view_frame(x0, y0, s, ow, oh, fmt, out=out)
                    assert turn == 3 and np.array_equal(got, want), ("pinned", s, x0, y0, fmt)
                    frames += 2
        p = b.perf()
        assert p["view_frames"] == frames and p["view_kernel_ms"] > 0
        # the view disturbed neither the layout nor the buffers
        assert b.board_hash() == digest and b.turn() == 3
        b.step(5)
        assert np.array_equal(b.snapshot_bytes(), run_np(board0, 8))


def test_view_stream_is_the_window_of_testsdl(fixtures):
    """512^2 fixture, a frame every turn at s = 1: the white pixels of frame t
    are alive_512[t] (the reference's CountPixels per TurnComplete) and the
    last frame is check/images/512x512x100."""
    alive = fixtures["alive_512"]
    out = golhip.host_array((100, 512, 512), np.uint32)
    with golhip.Board(512, 512) as b:
        b.load_bytes(unpack_bits(fixtures["image_512"], 512))
        frames, done = b.view_stream(100, 1, out=out)
        assert done == 100 and b.turn() == 100 and frames.shape == (100, 512, 512)
    white = (frames == 0xFFFFFFFF).sum(axis=(1, 2))
    assert np.array_equal(white, alive[1:101])
    assert np.array_equal((frames != 0) & (frames != 0xFFFFFFFF), np.zeros_like(frames, dtype=bool))
    assert np.array_equal(frames[-1], golhip.view_frame_np(fixtures["check_512x100"], 512, 512))


def test_view_stream_frames_and_remainder():
    """14 turns, a frame every 4: frames of turns 4, 8, 12, two more turns
    stepped; too few frames is ERANGE with nothing advanced; pageable and
    page-locked `out` hold the same bytes."""
    W, H, s, x0, y0 = 256, 128, 3, 256 - 7, 128 - 3
    ow, oh = W // s, H // s
    board0 = fill_random_np(W, H, SEED)
    want = np.stack([golhip.view_frame_np(pack_bits(run_np(board0, t)), W, H, x0, y0, s, ow, oh) for t in (4, 8, 12)])
    with golhip.Board(W, H) as b:
        b.fill_random(SEED)
        with pytest.raises(golhip.GolHipError) as e:
            b.view_stream(14, 4, x0, y0, s, ow, oh, cap_frames=2)
        assert e.value.code == golhip.GOLHIP_ERANGE and "holds 2 frames" in str(e.value) and "need 3" in str(e.value)
        assert b.turn() == 0
        pageable, done = b.view_stream(14, 4, x0, y0, s, ow, oh)
        assert done == 14 and b.turn() == 14
        assert np.array_equal(b.snapshot_bytes(), run_np(board0, 14))
        b.fill_random(SEED)
        out = golhip.host_array((3, oh, ow), np.uint32)
        pinned, done = b.view_stream(14, 4, x0, y0, s, ow, oh, out=out)
        assert done == 14 and b.turn() == 14
    assert pageable.shape == (3, oh, ow) and np.array_equal(pageable, want)
    assert np.array_equal(pinned, want)


def test_view_on_strips():
    """A 128^2 board as two 64-row strips: their frames at s = 4, stacked, are
    the whole board's; y counts torus rows and may not leave the strip."""
    W = H = 128
    with golhip.Board(W, H) as one:
        one.fill_random(SEED)
        one.step(6)
        whole, _ = one.view_frame(W - 7, 0, 4, fmt=golhip.VIEW_GRAY8)
    strips = [golhip.Board(W, H, row0=r, rows=64) for r in (0, 64)]
    try:
        for st in strips:
            st.fill_random(SEED)
        golhip.group_step(strips, 6)
        parts = [st.view_frame(W - 7, st.row0, 4, 32, 16, golhip.VIEW_GRAY8) for st in strips]
        assert [t for _, t in parts] == [6, 6]
        assert np.array_equal(np.concatenate([f for f, _ in parts]), whole)
        for st, y0, oh in ((strips[1], 60, 16), (strips[1], 64, 17), (strips[0], 64, 1)):
            with pytest.raises(golhip.GolHipError) as e:
                st.view_frame(0, y0, 4, 32, oh)
            assert e.value.code == -1 and "leave the strip" in str(e.value)
    finally:
        for st in strips:
            st.close()


def test_view_5120_into_1024_gray():
    """BASELINE's 5120^2 board as a 1024^2 GRAY8 frame (s = 5)."""
    N = 5120
    with golhip.Board(N, N) as b:
        b.fill_random(SEED)
        b.step(3)
        got, turn = b.view_frame(scale=5, fmt=golhip.VIEW_GRAY8)
        words = b.snapshot_bits()
    assert turn == 3 and got.shape == (1024, 1024)
    assert np.array_equal(got, golhip.view_frame_np(words, N, N, scale=5, fmt=golhip.VIEW_GRAY8))


def test_view_quads_scale_64_from_the_last_cell():
    """8192 x 4096 on quads, s = 64, a full lap from the board's last cell:
    every pixel row and column straddles a seam, mid-quad."""
    W, H = 8192, 4096
    with golhip.Board(W, H) as b:
        b.set_option("wpl", 4)
        b.fill_random(SEED)
        b.step(3)
        assert b.perf()["words_per_lane"] == 4
        got, turn = b.view_frame(W - 1, H - 1, 64)
        words = b.snapshot_bits()
    assert turn == 3 and got.shape == (64, 128)
    assert np.array_equal(got, golhip.view_frame_np(words, W, H, W - 1, H - 1, 64))


def test_view_arguments():
    lib = golhip.load()
    buf = np.zeros(64 * 64, dtype=np.uint32)

    def call(b, v, out=buf, cap=None):
        t = ctypes.c_int64(-7)
        rc = lib.golhip_view_frame(b.handle, ctypes.byref(v) if v is not None else None,
                                   ctypes.c_void_p(out.ctypes.data) if out is not None else None,
                                   buf.nbytes if cap is None else cap, ctypes.byref(t))
        return rc, lib.golhip_last_error().decode(), t.value

    with golhip.Board(64, 64) as b:
        ok = golhip.View(0, 0, 1, 64, 64, golhip.VIEW_ARGB)
        rc, msg, _ = call(b, ok)
        assert rc == -1 and msg == "no board loaded"
        b.fill_random(SEED)
        b.step(2)
        digest = b.board_hash()
        for v, text in ((golhip.View(0, 0, 0, 64, 64, 0), "view scale 0 not in [1, 1024]"),
                        (golhip.View(0, 0, 1025, 1, 1, 0), "view scale 1025 not in [1, 1024]"),
                        (golhip.View(0, 0, 2, 33, 32, 0), "more than one lap"),
                        (golhip.View(0, 0, 2, 32, 33, 0), "more than one lap"),
                        (golhip.View(64, 0, 1, 1, 1, 0), "outside the 64 x 64 board"),
                        (golhip.View(0, -1, 1, 1, 1, 0), "outside the 64 x 64 board"),
                        (golhip.View(0, 0, 1, 0, 1, 0), "view frame 0 x 1"),
                        (golhip.View(0, 0, 1, 1, 1, 2), "view format 2")):
            rc, msg, _ = call(b, v)
            assert rc == -1 and text in msg, (rc, msg)
        rc, msg, _ = call(b, ok, out=None)
        assert rc == -1 and msg == "out is null"
        rc, msg, _ = call(b, None)
        assert rc == -1 and msg == "view is null"
        rc, msg, _ = call(b, ok, cap=64 * 64 * 4 - 1)
        assert rc == golhip.GOLHIP_ERANGE and msg == "buffer holds 16383 bytes, the frame needs 16384"
        rc, msg, turn = call(b, ok)
        assert rc == 0 and turn == 2
        # stream arguments: every < 1, and nothing of the above moved the board
        with pytest.raises(golhip.GolHipError) as e:
            b.view_stream(4, 0)
        assert e.value.code == -1 and "every 0" in str(e.value)
        assert b.board_hash() == digest and b.turn() == 2
