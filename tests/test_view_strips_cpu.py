"""The view across row strips, as far as it shows without a GPU: the exported
symbols, the opt-in switch of gol.Run in all its spellings, and the argument
checks that come before any device call."""
import ctypes
import os
import re

import pytest

golhip = pytest.importorskip("golhip")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_group_view_symbols_and_wrappers():
    lib = golhip.load()
    header = read("include", "golhip.h")
    for name in ("golhip_group_view_frame", "golhip_group_view_stream"):
        assert re.search(rf"\bint {name}\(golhip_t \*hs, int32_t n,", header), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert callable(golhip.group_view_frame) and callable(golhip.group_view_stream)


def test_group_view_refuses_a_bad_group_before_any_device_call():
    lib = golhip.load()
    v = golhip.View(0, 0, 1, 1, 1, golhip.VIEW_ARGB)
    buf = (ctypes.c_uint32 * 1)()
    nf, done = ctypes.c_uint64(7), ctypes.c_int64(7)
    assert lib.golhip_group_view_frame(None, 2, ctypes.byref(v), buf, 4, None) == -1
    assert lib.golhip_last_error().decode() == "bad group"
    arr = (ctypes.c_void_p * 2)(None, None)
    assert lib.golhip_group_view_frame(arr, 2, ctypes.byref(v), buf, 4, None) == -1
    assert lib.golhip_last_error().decode() == "null handle"
    assert lib.golhip_group_view_frame(arr, 0, ctypes.byref(v), buf, 4, None) == -1
    assert lib.golhip_group_view_stream(arr, 2, 4, 1, ctypes.byref(v), buf, 4, ctypes.byref(nf),
                                        ctypes.byref(done)) == -1
    assert (nf.value, done.value) == (0, 0)


def test_run_switch_is_spelled_the_same_everywhere():
    """GOLRUN_FLAG_VIEW_STRIPS is the next free flag bit, the Python constant
    is that bit, and the mirror, the CLI and the Go binding know the switch."""
    header = read("include", "golrun.h")
    flags = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (GOLRUN_FLAG_\w+) (0x[0-9a-f]+)u", header)}
    assert flags["GOLRUN_FLAG_VIEW_STRIPS"] == golhip.FLAG_VIEW_STRIPS == 0x10
    assert sorted(flags.values()) == [0x1, 0x2, 0x4, 0x8, 0x10]
    host = read("game-of-life-distributed_amd", "csrc", "gol_host.cpp")
    assert '"GOL_VIEW_STRIPS"' in host and "GOLRUN_FLAG_VIEW_STRIPS" in host
    assert "int view_strips = -1;" in read("game-of-life-distributed_amd", "csrc", "gol_host.h")
    assert '"-viewStrips"' in read("game-of-life-distributed_amd", "csrc", "golrun_main.cpp")
    go = read("integration", "gol", "golhip.go")
    assert "golhip_group_view_frame(hs, n, v, out, cap, turn)" in go
    assert "golhip_group_view_stream(hs, n, t, every, v, out, cap, frames, done)" in go
