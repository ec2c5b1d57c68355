"""The live view of a board held as row strips (golhip_group_view_frame /
golhip_group_view_stream) against golhip.view_frame_np of the whole board,
bit-exact.  The whole board is the oracle's (fill_random_np, run_np,
pack_bits), never a snapshot of the strips.

The strip boundaries lie off every pixel grid that the scales form, so pixel
rows straddle strips (the counts + resolve path of gol_view.hip), lie wholly in
one strip (the kernels of the single-handle view, on the strip) or both, in the
same frame."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import fill_random_np, pack_bits, run_np

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

SEED = 0x51EED
FORMATS = [golhip.VIEW_ARGB, golhip.VIEW_GRAY8]
SCALES = [1, 3, 5, 32, 33, 64]

# board, option wpl (None: leave), perf words_per_lane that proves the layout, first rows of strips 1..
LAYOUTS = [
    pytest.param(96, 64, None, 1, (21,), id="canonical-96x64"),
    pytest.param(48, 40, None, 0, (13, 14), id="generic-48x40-one-row-strip"),
    pytest.param(192, 96, 2, 2, (40,), id="pairs-192x96"),
    pytest.param(256, 128, 4, 4, (50,), id="quads-256x128"),
]


def make_strips(W, H, cuts, wpl=None, timing=False, fill=True):
    """Strips of a W x H board that begin at rows 0, *cuts."""
    r0 = [0, *cuts]
    strips = []
    try:
        for a, b in zip(r0, [*cuts, H]):
            st = golhip.Board(W, H, row0=a, rows=b - a, timing=timing)
            strips.append(st)
            if wpl is not None:
                st.set_option("wpl", wpl)
            if fill:
                st.fill_random(SEED)
    except Exception:
        close_all(strips)
        raise
    return strips


def close_all(strips):
    for st in strips:
        st.close()


def gather(strips):
    return np.concatenate([st.snapshot_bytes() for st in strips])


def viewports(W, H, s):
    """The two of test_gpu_view.py: the full frame at the origin and a smaller
    one across both seams, from the last strip into the first."""
    ow, oh = W // s, H // s
    yield 0, 0, ow, oh
    yield W - 7, H - 3, max(ow - 1, 1), max(oh - 1, 1)


def strips_touched(cuts, H, y0, rows):
    """Indices of the strips that hold a row of [y0, y0 + rows) mod H."""
    r0 = [0, *cuts, H]
    ys = (y0 + np.arange(rows)) % H
    return {i for i in range(len(r0) - 1) if ((ys >= r0[i]) & (ys < r0[i + 1])).any()}


def test_cuts_are_the_issue_s_strip_rows():
    """(21, 43), (13, 1, 26), (40, 56), (50, 78) rows."""
    rows = {p.id: np.diff([0, *p.values[4], p.values[1]]).tolist() for p in LAYOUTS}
    assert rows == {"canonical-96x64": [21, 43], "generic-48x40-one-row-strip": [13, 1, 26],
                    "pairs-192x96": [40, 56], "quads-256x128": [50, 78]}


@pytest.mark.parametrize("W,H,wpl,want_wpl,cuts", LAYOUTS)
def test_group_view_frame_every_layout(W, H, wpl, want_wpl, cuts):
    board0 = fill_random_np(W, H, SEED)
    words = pack_bits(run_np(board0, 3))
    strips = make_strips(W, H, cuts, wpl, timing=True)
    try:
        golhip.group_step(strips, 3)
        assert all(st.perf()["words_per_lane"] == want_wpl for st in strips)
        digests = [st.board_hash() for st in strips]
        pinned = golhip.host_array((H, W), np.uint32)
        frames = [0] * len(strips)
        for s in [s for s in SCALES if s <= min(W, H)]:
            for x0, y0, ow, oh in viewports(W, H, s):
                for fmt in FORMATS:
                    want = golhip.view_frame_np(words, W, H, x0, y0, s, ow, oh, fmt)
                    got, turn = golhip.group_view_frame(strips, x0, y0, s, ow, oh, fmt)
                    assert turn == 3
                    assert got.dtype == want.dtype and np.array_equal(got, want), (s, x0, y0, fmt)
                    # the same frame written by the kernels themselves into page-locked memory
                    out = pinned.reshape(-1).view(want.dtype)[: ow * oh]
                    out[:] = 0x5A
                    got, turn = golhip.group_view_frame(strips, x0, y0, s, ow, oh, fmt, out=out)
                    assert turn == 3 and np.array_equal(got, want), ("pinned", s, x0, y0, fmt)
                    for i in strips_touched(cuts, H, y0, oh * s):
                        frames[i] += 2
        for st, n in zip(strips, frames):
            p = st.perf()
            assert n > 0 and p["view_frames"] == n and p["view_kernel_ms"] > 0
        # the view disturbed neither the layout nor the buffers
        assert [st.board_hash() for st in strips] == digests and all(st.turn() == 3 for st in strips)
        golhip.group_step(strips, 5)
        assert np.array_equal(gather(strips), run_np(board0, 8))
    finally:
        close_all(strips)


@pytest.mark.parametrize("W,H,cuts,s,x0,y0,ow", [
    pytest.param(96, 64, (21,), 64, 0, 20, 1, id="96x64-s64-strip0-twice"),
    pytest.param(96, 64, (21,), 64, 90, 20, 1, id="96x64-s64-x-seam"),
    pytest.param(48, 40, (13, 14), 32, 0, 5, 1, id="48x40-s32-three-strips"),
])
def test_one_pixel_row_over_the_lap(W, H, cuts, s, x0, y0, ow):
    """One pixel row that takes rows from every strip; at s = H = 64 from
    y0 = 20 strip 0 gives two pieces, rows [20, 21) and [0, 20)."""
    words = pack_bits(run_np(fill_random_np(W, H, SEED), 3))
    strips = make_strips(W, H, cuts)
    try:
        golhip.group_step(strips, 3)
        for fmt in FORMATS:
            want = golhip.view_frame_np(words, W, H, x0, y0, s, ow, 1, fmt)
            got, turn = golhip.group_view_frame(strips, x0, y0, s, ow, 1, fmt)
            assert turn == 3 and np.array_equal(got, want), (fmt, got, want)
    finally:
        close_all(strips)


def test_group_view_stream_frames_and_remainder():
    """256 x 128 as (50, 78) rows, 14 turns, a frame every 4 at s = 3 from
    (249, 125): frames of turns 4, 8, 12, every strip at turn 14 with the
    oracle's rows; too few frames is ERANGE with nothing advanced; pageable and
    page-locked `out` hold the same bytes."""
    W, H, s, x0, y0 = 256, 128, 3, 256 - 7, 128 - 3
    ow, oh = W // s, H // s
    board0 = fill_random_np(W, H, SEED)
    want = np.stack([golhip.view_frame_np(pack_bits(run_np(board0, t)), W, H, x0, y0, s, ow, oh) for t in (4, 8, 12)])
    strips = make_strips(W, H, (50,))
    try:
        with pytest.raises(golhip.GolHipError) as e:
            golhip.group_view_stream(strips, 14, 4, x0, y0, s, ow, oh, cap_frames=2)
        assert e.value.code == golhip.GOLHIP_ERANGE and "holds 2 frames" in str(e.value) and "need 3" in str(e.value)
        assert all(st.turn() == 0 for st in strips)
        pageable, done = golhip.group_view_stream(strips, 14, 4, x0, y0, s, ow, oh)
        assert done == 14 and all(st.turn() == 14 for st in strips)
        assert np.array_equal(gather(strips), run_np(board0, 14))
        for st in strips:
            st.fill_random(SEED)
        out = golhip.host_array((3, oh, ow), np.uint32)
        pinned, done = golhip.group_view_stream(strips, 14, 4, x0, y0, s, ow, oh, out=out)
        assert done == 14 and all(st.turn() == 14 for st in strips)
        assert np.array_equal(gather(strips), run_np(board0, 14))
    finally:
        close_all(strips)
    assert pageable.shape == (3, oh, ow) and np.array_equal(pageable, want)
    assert np.array_equal(pinned, want)


def test_group_view_arguments():
    lib = golhip.load()
    buf = np.zeros(64 * 64, dtype=np.uint32)
    ok = golhip.View(0, 0, 1, 64, 64, golhip.VIEW_ARGB)

    def call(boards, v, out=buf, cap=None):
        arr = (ctypes.c_void_p * len(boards))(*[b.handle for b in boards])
        t = ctypes.c_int64(-7)
        rc = lib.golhip_group_view_frame(arr, len(boards), ctypes.byref(v) if v is not None else None,
                                         ctypes.c_void_p(out.ctypes.data) if out is not None else None,
                                         buf.nbytes if cap is None else cap, ctypes.byref(t))
        return rc, lib.golhip_last_error().decode(), t.value

    strips = make_strips(64, 64, (21,), fill=False)
    try:
        # fresh strips of which only one is loaded
        strips[0].fill_random(SEED)
        rc, msg, _ = call(strips, ok)
        assert rc == -1 and msg == "strip 1 has no board"
        strips[1].fill_random(SEED)
        # strips that do not cover the board, or do not start it
        rc, msg, _ = call(strips[:1], ok)
        assert rc == -1 and msg == "strips do not cover the board"
        rc, msg, _ = call(strips[1:], ok)
        assert rc == -1 and msg == "strip 0 starts at 21, expected 0"
        # strips at different turns: one of them reloaded after a step of both
        golhip.group_step(strips, 2)
        strips[1].fill_random(SEED)
        rc, msg, _ = call(strips, ok)
        assert rc == -1 and msg == "strip 1 is at turn 0, strip 0 at turn 2"
        with pytest.raises(golhip.GolHipError) as e:
            golhip.group_view_stream(strips, 4, 1)
        assert e.value.code == -1 and "strip 1 is at turn 0" in str(e.value)
        strips[0].fill_random(SEED)
        golhip.group_step(strips, 2)
        digests = [st.board_hash() for st in strips]
        # the view is checked against the whole torus
        for v, text in ((golhip.View(0, 0, 0, 64, 64, 0), "view scale 0 not in [1, 1024]"),
                        (golhip.View(0, 0, 2, 32, 33, 0), "more than one lap"),
                        (golhip.View(0, 64, 1, 1, 1, 0), "outside the 64 x 64 board"),
                        (golhip.View(0, 0, 1, 0, 1, 0), "view frame 0 x 1"),
                        (golhip.View(0, 0, 1, 1, 1, 2), "view format 2")):
            rc, msg, _ = call(strips, v)
            assert rc == -1 and text in msg, (rc, msg)
        rc, msg, _ = call(strips, ok, out=None)
        assert rc == -1 and msg == "out is null"
        rc, msg, _ = call(strips, None)
        assert rc == -1 and msg == "view is null"
        rc, msg, _ = call(strips, ok, cap=64 * 64 * 4 - 1)
        assert rc == golhip.GOLHIP_ERANGE and msg == "buffer holds 16383 bytes, the frame needs 16384"
        rc, msg, turn = call(strips, ok)
        assert rc == 0 and turn == 2
        want = golhip.view_frame_np(pack_bits(run_np(fill_random_np(64, 64, SEED), 2)), 64, 64)
        assert np.array_equal(buf.reshape(64, 64), want)
        with pytest.raises(golhip.GolHipError) as e:
            golhip.group_view_stream(strips, 4, 0)
        assert e.value.code == -1 and "every 0" in str(e.value)
        assert [st.board_hash() for st in strips] == digests and all(st.turn() == 2 for st in strips)
    finally:
        close_all(strips)


def test_group_of_one_whole_board_is_the_board_s_view():
    with golhip.Board(96, 64) as b:
        b.fill_random(SEED)
        b.step(3)
        for fmt in FORMATS:
            want, _ = b.view_frame(90, 61, 5, 18, 11, fmt)
            got, turn = golhip.group_view_frame([b], 90, 61, 5, 18, 11, fmt)
            assert turn == 3 and np.array_equal(got, want)
        frames, done = golhip.group_view_stream([b], 5, 2, scale=3)
        assert done == 5 and b.turn() == 8 and frames.shape == (2, 21, 32)
        assert np.array_equal(frames[1], golhip.view_frame_np(pack_bits(run_np(fill_random_np(96, 64, SEED), 7)),
                                                              96, 64, scale=3))
