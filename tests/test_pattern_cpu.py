"""Pattern files without a GPU: golhip_pattern_info and
golhip_pattern_read (csrc/gol_pattern_file.h behind them) against the numpy
restatements rle_parse_np / rle_format_np, which share no code with them.

* RLE: a glider, the Gosper glider gun, and a pattern with every liberty the
  format allows; every accepted spelling of the rule; every refusal with its
  message; a header of 2e9 x 2e9 cells whose body is parsed without an
  allocation of that size;
* PGM patterns, told from RLE by their first bytes;
* stamp_np, the statement the GPU tests check the kernel against, on cases
  small enough to write out by hand.
"""
import ctypes
import os

import numpy as np
import pytest

golhip = pytest.importorskip("golhip")

NEW_SYMBOLS = ["golhip_clear", "golhip_stamp_bits", "golhip_group_stamp_bits", "golhip_pattern_info",
               "golhip_pattern_read", "golhip_stamp_file"]

GLIDER = "#N Glider\nx = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n"
GLIDER_CELLS = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=bool)
GUN = ("#N Gosper glider gun\n#C the first gun: a glider every 30 turns\nx = 36, y = 9, rule = B3/S23\n"
       "24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4b\nobo$10bo5bo7bo$11bo3bo$12b2o!\n")
# 3$, a row of only dead cells (5b), trailing b runs and the last row left out,
# a run count wrapped over a line break (1 / 0bo = 10bo), #C / #N lines, no rule
TRICKY = "#N tricky\n#C a comment\n\nx = 12, y = 7\n2o$1\n0bo3$5b$o!\nanything behind the ! is ignored\n"
TRICKY_CELLS = np.zeros((7, 12), dtype=bool)
TRICKY_CELLS[0, 0:2] = True
TRICKY_CELLS[1, 10] = True
TRICKY_CELLS[5, 0] = True


def _put(tmp_path, name, blob):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(blob if isinstance(blob, bytes) else blob.encode())
    return p


def test_new_symbols_in_header_and_library():
    syms = golhip.header_symbols()
    lib = golhip.load()
    for s in NEW_SYMBOLS:
        assert s in syms and hasattr(lib, s), s


@pytest.mark.parametrize("name,text,cells", [("glider", GLIDER, GLIDER_CELLS), ("tricky", TRICKY, TRICKY_CELLS),
                                             ("gun", GUN, None)])
def test_known_patterns(tmp_path, name, text, cells):
    p = _put(tmp_path, name + ".rle", text)
    want = golhip.rle_parse_np(text)
    if cells is not None:
        assert np.array_equal(want, cells)
    info = golhip.pattern_info(p)
    assert info == {"width": want.shape[1], "height": want.shape[0], "alive": int(want.sum()), "format": "rle"}
    got = golhip.pattern_read(p)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    if name == "glider":
        assert (info["width"], info["height"], info["alive"]) == (3, 3, 5)
    if name == "gun":
        assert (info["width"], info["height"], info["alive"]) == (36, 9, 36)


@pytest.mark.parametrize("w,h", [(1, 1), (70, 1), (1, 70), (33, 9), (100, 40)])
def test_round_trip(tmp_path, w, h):
    rng = np.random.default_rng(0x51A + 131 * w + h)
    for k, density in enumerate((0.5, 0.05, 0.0, 1.0)):
        c = rng.random((h, w)) < density
        text = golhip.rle_format_np(c)
        assert max(len(line) for line in text.split("\n")) <= 70
        assert np.array_equal(golhip.rle_parse_np(text), c)
        p = _put(tmp_path, f"r{k}.rle", text)
        assert np.array_equal(golhip.pattern_read(p), c)
        assert golhip.pattern_info(p) == {"width": w, "height": h, "alive": int(c.sum()), "format": "rle"}


@pytest.mark.parametrize("rule", [", rule = B3/S23", ", rule = b3/s23", ", rule = 23/3", ",rule=B3/S23", ""])
def test_rule_spellings(tmp_path, rule):
    p = _put(tmp_path, "g.rle", f"x = 3, y = 3{rule}\nbob$2bo$3o!\n")
    assert np.array_equal(golhip.pattern_read(p), GLIDER_CELLS)


REFUSALS = [
    ("rule", "x = 3, y = 3, rule = B36/S23\nbob$2bo$3o!\n", "rule B36/S23 is not Conway's B3/S23"),
    ("no_header", "bob$2bo$3o!\n", "no header line"),
    ("header_junk", "#C only comments\n", "no header line"),
    ("empty", "", "no header line"),
    ("width_0", "x = 0, y = 3\n!\n", "outside 1 .. 2^31 - 1"),
    ("height_neg", "x = 3, y = -1\n!\n", "outside 1 .. 2^31 - 1"),
    ("width_2_31", "x = 2147483648, y = 3\n!\n", "outside 1 .. 2^31 - 1"),
    ("run_x", "x = 3, y = 3\n4o!\n", "a run leaves the 3 x 3 box"),
    ("run_x_dead", "x = 3, y = 3\n2o2b!\n", "a run leaves the 3 x 3 box"),
    ("run_y", "x = 3, y = 1\no$o!\n", "a run leaves the 3 x 1 box"),
    ("run_count", "x = 3, y = 3\n99999999999o!\n", "a run leaves the 3 x 3 box"),
    ("unknown", "x = 3, y = 3\nbzb$2bo$3o!\n", "unknown character 'z'"),
    ("no_bang", "x = 3, y = 3\nbob$2bo$3o\n", "no '!' before the end of the file"),
]


@pytest.mark.parametrize("name,text,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(tmp_path, name, text, msg):
    p = _put(tmp_path, name + ".rle", text)
    for fn in (golhip.pattern_info, golhip.pattern_read):
        with pytest.raises(golhip.GolHipError) as e:
            fn(p)
        assert e.value.code == golhip.GOLHIP_EINVAL and msg in str(e.value), (name, str(e.value))
    with pytest.raises(ValueError):
        golhip.rle_parse_np(text)


def test_missing_file(tmp_path):
    with pytest.raises(golhip.GolHipError) as e:
        golhip.pattern_info(str(tmp_path / "none.rle"))
    assert e.value.code == golhip.GOLHIP_EINVAL and "no such file" in str(e.value)


def test_huge_header_allocates_nothing(tmp_path):
    """4e18 cells declared, none alive: the body is parsed in one pass."""
    p = _put(tmp_path, "huge.rle", "x = 2000000000, y = 2000000000\n!\n")
    assert golhip.pattern_info(p) == {"width": 2000000000, "height": 2000000000, "alive": 0, "format": "rle"}
    p = _put(tmp_path, "huge2.rle", "x = 2000000000, y = 2000000000\n1999999999bo1999999999$2000000000o!\n")
    assert golhip.pattern_info(p)["alive"] == 2000000001


def test_read_reports_the_size_it_needs(tmp_path):
    p = _put(tmp_path, "gun.rle", GUN)
    info = golhip.PatternInfo()
    words = np.full(18, 0xFFFFFFFF, dtype=np.uint32)
    lib = golhip.load()
    rc = lib.golhip_pattern_read(os.fsencode(p), ctypes.c_void_p(words.ctypes.data), 17, ctypes.byref(info))
    assert rc == golhip.GOLHIP_ERANGE and (info.width, info.height) == (36, 9)
    assert (words == 0xFFFFFFFF).all()  # nothing written
    rc = lib.golhip_pattern_read(os.fsencode(p), ctypes.c_void_p(words.ctypes.data), 18, ctypes.byref(info))
    assert rc == 0 and info.alive == 36 and int(np.unpackbits(words.view(np.uint8)).sum()) == 36


def test_pgm_patterns(tmp_path):
    rng = np.random.default_rng(7)
    raster = rng.choice(np.array([0, 255, 7, 254], dtype=np.uint8), size=(9, 37))
    p = _put(tmp_path, "p.pgm", golhip.image_header_np(37, 9) + raster.tobytes())
    want = raster == 255
    assert golhip.pattern_info(p) == {"width": 37, "height": 9, "alive": int(want.sum()), "format": "pgm"}
    assert np.array_equal(golhip.pattern_read(p), want)
    # the format goes by the first bytes, not the name
    q = _put(tmp_path, "named.rle", golhip.image_header_np(37, 9) + raster.tobytes())
    assert golhip.pattern_info(q)["format"] == "pgm"
    r = _put(tmp_path, "named.pgm", GLIDER)
    assert golhip.pattern_info(r) == {"width": 3, "height": 3, "alive": 5, "format": "rle"}
    short = _put(tmp_path, "short.pgm", golhip.image_header_np(37, 9) + raster.tobytes()[:-1])
    for fn in (golhip.pattern_info, golhip.pattern_read):
        with pytest.raises(golhip.GolHipError) as e:
            fn(short)
        assert e.value.code == golhip.GOLHIP_EINVAL and "short raster" in str(e.value)
    bad = _put(tmp_path, "maxval.pgm", b"P5\n3 3\n15\n" + bytes(9))
    with pytest.raises(golhip.GolHipError) as e:
        golhip.pattern_info(bad)
    assert "Incorrect maxval/bit depth" in str(e.value)


def test_pattern_words_np():
    c = np.zeros((2, 33), dtype=bool)
    c[0, 0] = c[0, 31] = c[1, 32] = True
    assert golhip.pattern_words_np(c).tolist() == [[0x80000001, 0], [0, 1]]
    assert golhip.pattern_words_np(np.where(c, 255, 7).astype(np.uint8)).tolist() == [[0x80000001, 0], [0, 1]]


def test_stamp_np_by_hand():
    board = np.zeros((4, 5), dtype=bool)
    board[:, 0] = True
    pat = np.array([[1, 0], [1, 1]], dtype=bool)
    # across both seams: pattern (r, c) -> board ((3 + r) % 4, (4 + c) % 5)
    got = golhip.stamp_np(board, pat, 4, 3, golhip.STAMP_COPY)
    want = board.copy()
    want[3, 4], want[3, 0], want[0, 4], want[0, 0] = True, False, True, True
    assert np.array_equal(got, want)
    assert np.array_equal(golhip.stamp_np(board, pat, 4, 3, golhip.STAMP_OR), board | np.array(
        [[0, 0, 0, 0, 1], [0] * 5, [0] * 5, [0, 0, 0, 0, 1]], dtype=bool))
    x = golhip.stamp_np(board, pat, 4, 3, golhip.STAMP_XOR)
    assert not x[0, 0] and x[0, 4] and x[3, 4] and x[3, 0] and x[1, 0]
    c = golhip.stamp_np(board, pat, 4, 3, golhip.STAMP_CLEAR)
    assert not c[0, 0] and c[3, 0] and c[1, 0] and not c[:, 4].any()
    # bytes in, bytes out
    b8 = np.where(board, 255, 0).astype(np.uint8)
    assert np.array_equal(golhip.stamp_np(b8, pat, 4, 3, golhip.STAMP_COPY), np.where(want, 255, 0))
    assert np.array_equal(board[:, 0], np.ones(4, dtype=bool))  # the input is not written
