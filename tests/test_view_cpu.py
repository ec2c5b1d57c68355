"""Live view without a GPU: the numpy restatement of the pixel definition
(golhip.view_frame_np, what the GPU tests compare against) against a plain
triple loop, the s = 1 frame against the reference's window contents
(sdl/window.go: FF FF FF FF or zeros; CountPixels, sdl_test.go:107-116), and
the new symbols of both libraries."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import fill_random_np, pack_bits, unpack_bits

golhip = pytest.importorskip("golhip")


def loop_frame(board, x0, y0, s, out_w, out_h, fmt):
    """The pixel definition of include/golhip.h, cell by cell."""
    H, W = board.shape
    out = np.zeros((out_h, out_w), dtype=np.uint8 if fmt == golhip.VIEW_GRAY8 else np.uint32)
    for py in range(out_h):
        for px in range(out_w):
            n = 0
            for dy in range(s):
                row = board[(y0 + py * s + dy) % H]
                for dx in range(s):
                    n += 1 if row[(x0 + px * s + dx) % W] == 255 else 0
            g = (255 * n + s * s - 1) // (s * s)
            out[py, px] = g if fmt == golhip.VIEW_GRAY8 else g * 0x01010101
    return out


@pytest.mark.parametrize("fmt", [golhip.VIEW_ARGB, golhip.VIEW_GRAY8])
@pytest.mark.parametrize("W,H,scale", [(W, H, s) for W, H in [(16, 16), (48, 40), (128, 64)]
                                       for s in (1, 3, 5, 32) if s <= min(W, H)])
def test_view_frame_np_matches_triple_loop(W, H, scale, fmt):
    board = fill_random_np(W, H, 7)
    words = pack_bits(board)
    x0, y0 = W - 7, H - 3  # both seams are crossed
    out_w, out_h = W // scale, H // scale
    got = golhip.view_frame_np(words, W, H, x0, y0, scale, out_w, out_h, fmt)
    assert got.dtype == (np.uint8 if fmt == golhip.VIEW_GRAY8 else np.uint32)
    assert np.array_equal(got, loop_frame(board, x0, y0, scale, out_w, out_h, fmt))
    # a smaller viewport from the same corner is the same picture's corner
    part = golhip.view_frame_np(words, W, H, x0, y0, scale, max(out_w - 1, 1), max(out_h - 1, 1), fmt)
    assert np.array_equal(part, got[: part.shape[0], : part.shape[1]])


def test_view_frame_np_extremes():
    """g rounds up: 0 only for an empty block, 255 for a full one (and for one
    within s^2 / 255 cells of full: ceil(255 * 1023 / 1024) = 255)."""
    W = H = 64
    board = np.zeros((H, W), dtype=np.uint8)
    board[0, 0] = 255            # one cell in block (0, 0)
    board[32:64, 32:64] = 255    # block (1, 1) full
    board[40:45, 40] = 0         # ... but for five cells: ceil(255 * 1019 / 1024) = 254
    g = golhip.view_frame_np(pack_bits(board), W, H, 0, 0, 32, 2, 2, golhip.VIEW_GRAY8)
    assert g.tolist() == [[1, 0], [0, 254]]
    board[41:45, 40] = 255       # one cell short of full still rounds up to 255
    g = golhip.view_frame_np(pack_bits(board), W, H, 0, 0, 32, 2, 2, golhip.VIEW_GRAY8)
    assert g.tolist() == [[1, 0], [0, 255]]
    board[40, 40] = 255
    g = golhip.view_frame_np(pack_bits(board), W, H, 0, 0, 32, 2, 2, golhip.VIEW_ARGB)
    assert g.tolist() == [[0x01010101, 0], [0, 0xFFFFFFFF]]


def test_view_frame_np_refuses_more_than_a_lap():
    words = np.zeros((16, 1), dtype=np.uint32)
    for kw in (dict(scale=0), dict(scale=3, out_w=6), dict(x0=16), dict(y0=-1), dict(out_h=0)):
        with pytest.raises(ValueError):
            golhip.view_frame_np(words, 16, 16, **kw)


def test_scale_one_is_the_reference_window(fixtures):
    """At s = 1 the ARGB frame is the window's pixel buffer after every flip
    of 100 turns, and its white pixels are CountPixels()."""
    words = fixtures["check_512x100"]
    frame = golhip.view_frame_np(words, 512, 512)
    assert frame.shape == (512, 512) and frame.dtype == np.uint32
    cells = (unpack_bits(words, 512) == 255).astype(np.uint32)
    assert np.array_equal(frame, cells * np.uint32(0x01010101) * np.uint32(255))
    assert int((frame == 0xFFFFFFFF).sum()) == int(fixtures["alive_512"][100])
    assert set(np.unique(frame).tolist()) <= {0, 0xFFFFFFFF}


def test_libraries_export_the_view():
    lib = golhip.load()
    for name in ("golhip_view_frame", "golhip_view_stream"):
        assert name in golhip.header_symbols()
        assert hasattr(lib, name), name
    host = golhip.load_host()
    for name in ("golrun_start_view", "golrun_view_frame"):
        assert hasattr(host, name), name


def test_perf_ends_with_the_view_counters():
    names = [k for k, _ in golhip.Perf._fields_]
    assert names[-2:] == ["view_frames", "view_kernel_ms"]
    assert golhip.Perf._fields_[-2][1] is ctypes.c_int64 and golhip.Perf._fields_[-1][1] is ctypes.c_double
    assert ctypes.sizeof(golhip.Perf) == 8 * len(names) - 4 * 6  # six int32 fields among the 8-byte ones


def test_view_struct_is_six_int32():
    assert ctypes.sizeof(golhip.View) == 24
    assert [k for k, _ in golhip.View._fields_] == ["x0", "y0", "scale", "out_w", "out_h", "format"]
