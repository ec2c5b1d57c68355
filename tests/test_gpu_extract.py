"""Saving patterns on the GPU (K12 and K13, csrc/gol_extract.hip; DESIGN.md
5.22): golhip_extract_bits, golhip_group_extract_bits, golhip_alive_box and
golhip_save_rle.

Every answer is compared with golhip.extract_np / golhip.alive_box_np on the
numpy model of the same board (oracle.run_np, golhip.life_like_np,
golhip.stamp_np), after at least one step, so the board lies in the layout it
is stepped in.  Equality is exact.  The shapes are the smallest at which the
kernels can go wrong: every shift and edge mask, both seams, the pair and quad
layouts, widths that are no multiple of 32 (the x seam inside a source word),
the rule kernel's canonical words, row strips, and one rectangle of more output
words than the extract's grid holds in a lap.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle.oracle import fill_random_np, run_np

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

EINVAL, ERANGE = golhip.GOLHIP_EINVAL, golhip.GOLHIP_ERANGE
HIGHLIFE = (0x048, 0x00C)
# gol_extract.hip: the grid is capped at 4096 blocks of 256 lanes, one output word a lane and lap
EXTRACT_GRID_CAP_WORDS = 4096 * 256
GLIDER = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], dtype=bool)

# (W, H, wpl option (0: the plan's), rule)
BOARDS = [(64, 37, 1, None), (64, 37, 2, None), (128, 37, 1, None), (128, 37, 2, None), (256, 37, 4, None),
          (33, 7, 0, None), (1000, 37, 0, None), (64, 37, 0, HIGHLIFE)]


def alive(cells):
    return np.asarray(cells) == 255


def stepped(b, W, H, wpl, rule, seed, turns=2):
    """Loads a random board and steps it; returns the model's board (0 / 255 bytes)."""
    want = fill_random_np(W, H, seed)
    if wpl:
        b.set_option("wpl", wpl)
    if rule:
        b.set_rule(rule)
    b.load_bytes(want)
    b.step(turns)
    want = golhip.life_like_np(want, *rule, turns) if rule else run_np(want, turns)
    p = b.perf()
    if wpl:
        assert p["words_per_lane"] == wpl, p
    if rule:
        assert p["kernel_variant"] == 5, p
    return want


def rectangles(W, H):
    """(x0, y0, pw, ph) on a W x H board."""
    base = 32 if W > 64 else 0
    out = [(5 % W, 3, 1, 1), (W - 1, H - 1, 1, 1),
           (3, 2, min(20, W), 4),           # inside one word
           (25, 1, min(20, W), 5),          # across a word boundary
           (W - 5, 4, min(11, W), 3),       # across the x seam
           (7, H - 2, min(9, W), 5),        # across the y seam
           (W - 3, H - 2, min(8, W), 6),    # across both
           (5 % W, 3, W, H),                # the whole board from another corner
           (W - 1, H - 1, W, H)]
    for xm in (0, 1, 31):
        for pw in (1, 31, 32, 33, W):
            out.append(((base + xm) % W, 2, min(pw, W), 3))
    return out


@pytest.mark.parametrize("W,H,wpl,rule", BOARDS)
def test_extract_against_the_model(W, H, wpl, rule):
    with golhip.Board(W, H) as b:
        want = stepped(b, W, H, wpl, rule, 0x5EEDE000 + W + wpl)
        for x0, y0, pw, ph in rectangles(W, H):
            got = b.extract(x0, y0, pw, ph)
            assert got.shape == (ph, pw)
            assert np.array_equal(got, golhip.extract_np(want, x0, y0, pw, ph)), (x0, y0, pw, ph)
        assert b.alive_box() == golhip.alive_box_np(want)


@pytest.mark.parametrize("W,H,wpl", [(33, 7, 0), (1000, 37, 0), (128, 37, 2), (256, 37, 4)])
def test_padding_bits_come_back_zero(W, H, wpl):
    """The raw words: bits of columns >= pw are zero, also where the x seam lies inside a source word."""
    with golhip.Board(W, H) as b:
        want = stepped(b, W, H, wpl, None, 0x5EEDE100 + W)
        lib = golhip.load()
        for x0, y0, pw, ph in rectangles(W, H):
            ww = (pw + 31) // 32
            words = np.full((ph, ww), 0xFFFFFFFF, dtype=np.uint32)  # whatever was there is overwritten
            assert lib.golhip_extract_bits(b.handle, x0, y0, pw, ph, words.ctypes.data, words.size) == 0
            assert np.array_equal(words, golhip.pattern_words_np(golhip.extract_np(want, x0, y0, pw, ph))), (x0, y0, pw, ph)


def test_second_lap_of_the_grid():
    """One rectangle of more output words than the grid holds in a lap, on a
    board just large enough for it: canonical words (W % 64 != 0)."""
    W, H = 8160, 4200
    x0, y0 = 37, 11
    # the first column segment of the first row interval alone: output words 0 .. 253 of H - y0 rows
    assert ((W - x0 + 31) // 32) * (H - y0) > EXTRACT_GRID_CAP_WORDS
    with golhip.Board(W, H) as b:
        want = stepped(b, W, H, 0, None, 0x5EEDE200, turns=1)
        assert b.perf()["words_per_lane"] == 1
        assert np.array_equal(b.extract(x0, y0, W, H), golhip.extract_np(want, x0, y0, W, H))
        assert b.alive_box() == (0, 0, W, H)


# ---------------------------------------------------------------- observers
@pytest.mark.parametrize("W,wpl", [(128, 2), (100, 0)])
def test_observer_contract(W, wpl):
    H = 37
    with golhip.Board(W, H) as b:
        if wpl:
            b.set_option("wpl", wpl)
        want = fill_random_np(W, H, 0x5EEDE300 + W)
        b.load_bytes(want)
        b.step(3, want_flips=True)
        old, want = run_np(want, 2), run_np(want, 3)
        ys, xs = np.nonzero(old != want)
        flips = np.stack([xs, ys], axis=1)
        before = (b.turn(), b.alive_count(), b.board_hash())
        assert before[:2] == (3, (int(np.count_nonzero(want == 255)), 3))
        assert np.array_equal(b.flips(), flips)
        for call in (lambda: b.extract(W - 7, H - 3, 40, 9), b.alive_box, lambda: b.extract(0, 0, W, H)):
            call()
            assert (b.turn(), b.alive_count(), b.board_hash()) == before
            assert np.array_equal(b.flips(), flips)
        bits = b.snapshot_bits()
        b.extract(3, 3, 70, 20)
        b.alive_box()
        assert np.array_equal(b.snapshot_bits(), bits)
        b.step(2)
        assert np.array_equal(b.extract(0, 0, W, H), alive(run_np(want, 2)))


# ---------------------------------------------------------------- row strips
def make_strips(W, H, cuts):
    return [golhip.Board(W, H, row0=cuts[i], rows=cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]


def put_group(strips, cells):
    """The whole board replaced in the layout the strips are stepped in."""
    golhip.group_stamp(strips, np.asarray(cells, dtype=bool), 0, 0, golhip.STAMP_COPY)


@pytest.mark.parametrize("W", [64, 1000])
def test_strips(W, tmp_path):
    H, cuts = 37, [0, 7, 20, 37]
    strips = make_strips(W, H, cuts)
    try:
        for s in strips:
            s.fill_random(0x5EEDE400 + W)
        golhip.group_step(strips, 2)
        want = run_np(fill_random_np(W, H, 0x5EEDE400 + W), 2)
        rects = [(W - 9, 5, 30, 20),     # across both inner strip boundaries and the x seam
                 (3, 30, 33, 15),        # across the y seam: rows 30 .. 36 and 0 .. 7
                 (W - 1, H - 1, W, H),   # everything, both seams
                 (11, 8, 1, 1), (0, 0, W, 7), (0, 7, W, 13)]
        for x0, y0, pw, ph in rects:
            assert np.array_equal(golhip.group_extract(strips, x0, y0, pw, ph),
                                  golhip.extract_np(want, x0, y0, pw, ph)), (x0, y0, pw, ph)
            # one strip alone: the rows it does not own come back zero
            for s, (r0, r1) in zip(strips, zip(cuts, cuts[1:])):
                own = np.zeros_like(want)
                own[r0:r1] = want[r0:r1]
                assert np.array_equal(s.extract(x0, y0, pw, ph), golhip.extract_np(own, x0, y0, pw, ph)), (x0, y0, r0)
        assert np.array_equal(strips[1].extract(0, 25, W, 5), np.zeros((5, W), dtype=bool))  # it owns none of these
        assert golhip.group_alive_box(strips) == golhip.alive_box_np(want)
        hashes = [s.board_hash() for s in strips]
        # alive cells in one strip only
        cells = np.zeros((H, W), dtype=bool)
        cells[9:12, W - 2:] = True
        cells[10, 0] = True
        put_group(strips, cells)
        assert golhip.group_alive_box(strips) == golhip.alive_box_np(cells) == (W - 2, 9, 3, 3)
        # on both sides of the y seam (and of the x seam)
        cells = np.zeros((H, W), dtype=bool)
        cells[H - 2, 5] = cells[1, W - 1] = cells[0, 2] = True
        put_group(strips, cells)
        assert golhip.group_alive_box(strips) == golhip.alive_box_np(cells) == (W - 1, H - 2, 7, 4)
        info = golhip.save_rle(strips, str(tmp_path / "s.rle"), chunk_rows=3)
        assert (info["width"], info["height"], info["alive"]) == (7, 4, 3)
        assert np.array_equal(golhip.pattern_read(str(tmp_path / "s.rle")), golhip.extract_np(cells, W - 1, H - 2, 7, 4))
        put_group(strips, np.zeros((H, W), dtype=bool))
        assert golhip.group_alive_box(strips) == (0, 0, 0, 0)
        put_group(strips, alive(want))
        assert [s.board_hash() for s in strips] == hashes
    finally:
        for s in strips:
            s.close()


# ---------------------------------------------------------------- the alive box
def put(b, cells):
    """The whole board replaced in the layout the handle is stepped in."""
    b.stamp(np.asarray(cells, dtype=bool), 0, 0, golhip.STAMP_COPY)


@pytest.mark.parametrize("W,H,wpl", [(64, 37, 1), (128, 37, 2), (256, 37, 4), (33, 7, 0), (1000, 37, 0)])
def test_alive_box(W, H, wpl):
    with golhip.Board(W, H) as b:
        stepped(b, W, H, wpl, None, 0x5EEDE500 + W)
        z = np.zeros((H, W), dtype=bool)
        put(b, z)
        assert b.alive_box() == (0, 0, 0, 0)
        put(b, ~z)
        assert b.alive_box() == (0, 0, W, H)
        for x, y in ((0, 0), (W - 1, H - 1), (31 % W, 3), (32 % W, 4)):
            one = z.copy()
            one[y, x] = True
            put(b, one)
            assert b.alive_box() == (x, y, 1, 1)
        # a glider whose corner is the board's last cell: a 3 x 3 box there, not the whole board
        g = golhip.stamp_np(z, GLIDER, W - 1, H - 1, golhip.STAMP_OR)
        put(b, g)
        assert b.alive_box() == golhip.alive_box_np(g) == (W - 1, H - 1, 3, 3)
        if W % 2 == 0:
            # two cells half a lap apart in x: two gaps tie, the smaller start wins
            tie = z.copy()
            tie[5, 3] = tie[6, 3 + W // 2] = True
            put(b, tie)
            assert b.alive_box() == golhip.alive_box_np(tie) == (3, 5, W // 2 + 1, 2)
        # two cells a third of H apart in y on a 37-row board: no tie, the box wraps
        far = z.copy()
        far[1, 7 % W] = far[H - 2, 7 % W] = True
        put(b, far)
        assert b.alive_box() == golhip.alive_box_np(far) == (7 % W, H - 2, 1, 4)
        # the last column only (at width 33 it is bit 0 of the row's last word)
        col = z.copy()
        col[:, W - 1] = True
        put(b, col)
        assert b.alive_box() == golhip.alive_box_np(col) == (W - 1, 0, 1, H)
        row = z.copy()
        row[H - 1, :] = True
        put(b, row)
        assert b.alive_box() == (0, H - 1, W, 1)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_board_unchanged(tmp_path):
    W, H = 100, 17
    lib = golhip.load()
    with golhip.Board(W, H) as b:
        want = stepped(b, W, H, 0, None, 0x5EEDE600)
        before = (b.turn(), b.alive_count(), b.board_hash())
        cases = {
            "pw > W": lambda: b.extract(0, 0, W + 1, 1),
            "ph > H": lambda: b.extract(0, 0, 1, H + 1),
            "pw = 0": lambda: b.extract(0, 0, 0, 1),
            "ph = 0": lambda: b.extract(0, 0, 1, 0),
            "x0 = W": lambda: b.extract(W, 0, 1, 1),
            "x0 = -1": lambda: b.extract(-1, 0, 1, 1),
            "y0 = H": lambda: b.extract(0, H, 1, 1),
            "y0 = -1": lambda: b.extract(0, -1, 1, 1),
            "save: pw > W": lambda: golhip.save_rle(b, str(tmp_path / "a.rle"), (0, 0, W + 1, 1)),
            "save: y0 = H": lambda: golhip.save_rle(b, str(tmp_path / "a.rle"), (0, H, 1, 1)),
            "save: ph = 0": lambda: golhip.save_rle(b, str(tmp_path / "a.rle"), (0, 0, 5, 0)),
            "save: chunk < 0": lambda: golhip.save_rle(b, str(tmp_path / "a.rle"), (0, 0, 5, 5), -1),
            "save: no directory": lambda: golhip.save_rle(b, str(tmp_path / "none" / "a.rle"), (0, 0, 5, 5)),
        }
        for name, call in cases.items():
            with pytest.raises(golhip.GolHipError) as e:
                call()
            assert e.value.code == EINVAL, (name, str(e.value))
        words = np.zeros((5, 2), dtype=np.uint32)
        assert lib.golhip_extract_bits(b.handle, 0, 0, 33, 5, None, 10) == EINVAL
        assert lib.golhip_extract_bits(b.handle, 0, 0, 33, 5, words.ctypes.data, 9) == ERANGE
        assert not words.any()
        assert lib.golhip_extract_bits(b.handle, 0, 0, 33, 5, words.ctypes.data, 10) == 0
        arr = (ctypes.c_void_p * 1)(b.handle)
        assert lib.golhip_group_extract_bits(arr, 1, 0, 0, 33, 5, words.ctypes.data, 9) == ERANGE
        assert lib.golhip_alive_box(arr, 1, None, None, None, None) == EINVAL
        assert os.listdir(tmp_path) == []
        assert (b.turn(), b.alive_count(), b.board_hash()) == before
        assert np.array_equal(b.extract(0, 0, W, H), alive(want))
    with golhip.Board(W, H) as b:  # never loaded
        with pytest.raises(golhip.GolHipError) as e:
            b.extract(0, 0, 1, 1)
        assert e.value.code == EINVAL and "no board" in str(e.value)
        with pytest.raises(golhip.GolHipError) as e:
            b.alive_box()
        assert e.value.code == EINVAL
    strips = make_strips(W, H, [0, 5, H])
    try:
        strips[0].clear()  # the second strip has no board
        for call in (lambda: golhip.group_extract(strips, 0, 0, 1, 1), lambda: golhip.group_alive_box(strips),
                     lambda: golhip.save_rle(strips, str(tmp_path / "a.rle"))):
            with pytest.raises(golhip.GolHipError) as e:
                call()
            assert e.value.code == EINVAL
        with pytest.raises(golhip.GolHipError) as e:  # a strip alone is no group
            golhip.group_alive_box([strips[0]])
        assert e.value.code == EINVAL
    finally:
        for s in strips:
            s.close()
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------- save_rle
def cxrle(path):
    m = re.match(r"#CXRLE Pos=(-?\d+),(-?\d+) Gen=(-?\d+)\n", open(path).read())
    return tuple(int(v) for v in m.groups())


@pytest.mark.parametrize("W,wpl", [(128, 2), (100, 0)])
def test_save_rle(tmp_path, W, wpl):
    H = 37
    with golhip.Board(W, H) as b:
        want = stepped(b, W, H, wpl, None, 0x5EEDE700 + W, turns=3)
        box = (W - 10, H - 3, 40, 13)  # both seams; 13 rows: no multiple of 2 or 5
        cells = golhip.extract_np(want, *box)
        texts = []
        for chunk in (0, 1, 2, 5):
            path = str(tmp_path / f"c{chunk}.rle")
            info = golhip.save_rle(b, path, box, chunk)
            assert info == {"width": 40, "height": 13, "alive": int(cells.sum()), "format": "rle"}
            assert np.array_equal(golhip.pattern_read(path), cells)
            assert np.array_equal(golhip.pattern_read(path), b.extract(*box))
            assert cxrle(path) == (W - 10, H - 3, 3)
            texts.append(open(path).read())
        assert len(set(texts)) == 1 and "rule = B3/S23\n" in texts[0]
        assert all(len(line) <= 70 for line in texts[0].split("\n"))
        # the alive box by default, and the way back
        z = np.zeros((H, W), dtype=bool)
        few = golhip.stamp_np(z, cells, W - 10, H - 3, golhip.STAMP_OR)
        put(b, few)
        digest = b.board_hash()
        path = str(tmp_path / "box.rle")
        info = golhip.save_rle(b, path)
        abox = golhip.alive_box_np(few)
        assert b.alive_box() == abox and (info["width"], info["height"]) == abox[2:]
        assert info["alive"] == int(few.sum())
        assert np.array_equal(golhip.pattern_read(path), golhip.extract_np(few, *abox))
        x0, y0, gen = cxrle(path)
        assert (x0, y0, gen) == (abox[0], abox[1], 3)
        b.clear()
        golhip.stamp_file(b, path, x0, y0)
        assert b.board_hash() == digest
        # an empty board
        b.clear()
        with pytest.raises(golhip.GolHipError) as e:
            golhip.save_rle(b, str(tmp_path / "empty.rle"))
        assert e.value.code == EINVAL and str(e.value).endswith("board is empty")
        assert sorted(os.listdir(tmp_path)) == ["box.rle", "c0.rle", "c1.rle", "c2.rle", "c5.rle"]


def test_save_rle_highlife(tmp_path):
    W, H = 64, 37
    with golhip.Board(W, H) as b:
        want = stepped(b, W, H, 0, HIGHLIFE, 0x5EEDE800)
        path = str(tmp_path / "hl.rle")
        golhip.save_rle(b, path, chunk_rows=5)
        text = open(path).read()
        abox = golhip.alive_box_np(want)
        assert f"x = {abox[2]}, y = {abox[3]}, rule = B36/S23\n" in text
        assert golhip.pattern_rule(path) == HIGHLIFE
        # (rle_parse_np reads Conway's rule alone)
        assert np.array_equal(golhip.rle_parse_np(text.replace("rule = B36/S23", "rule = B3/S23")),
                              golhip.extract_np(want, *abox))
        digest = b.board_hash()
        x0, y0, gen = cxrle(path)
        assert gen == 2
        b.clear()
        golhip.stamp_file(b, path, x0, y0)  # a HighLife handle takes a HighLife file
        assert b.board_hash() == digest
