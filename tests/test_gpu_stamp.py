"""The stamp kernel on the GPU (K10, csrc/gol_stamp.hip):
golhip_clear, golhip_stamp_bits, golhip_group_stamp_bits and golhip_stamp_file.

Expected boards come from golhip.stamp_np on oracle.fill_random_np, then
oracle.run_np.  Equality is exact on four things: snapshot_bits, alive_count,
board_hash against board_hash_np (it catches set padding bits) and view_frame
at scale 1.  The shapes are the smallest at which the kernel can go wrong:
every shift and edge mask, a full-width pattern off a word boundary (both
column segments touch one word), the x and y seams, the pair and quad layouts,
the padded torus, a board on the resident kernels, row strips, and one pattern
of more encode units than the grid cap.
"""
import numpy as np
import pytest

from oracle.oracle import fill_random_np, pack_bits, run_np

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

OPS = [golhip.STAMP_COPY, golhip.STAMP_OR, golhip.STAMP_XOR, golhip.STAMP_CLEAR]
H17 = 17
# gol_stamp.hip: the grid is capped at 4096 blocks of 256 lanes, one encode unit a lane and lap
STAMP_GRID_CAP_UNITS = 4096 * 256

GLIDER = "#N Glider\nx = 3, y = 3, rule = B3/S23\nbob$2bo$3o!\n"


def pattern(rng, pw, ph, p=0.5):
    return rng.random((ph, pw)) < p


def check(b, want, turn, what=None):
    """The four equalities, on one whole-torus handle."""
    bits = pack_bits(want)
    assert np.array_equal(b.snapshot_bits(), bits), what
    assert b.alive_count() == (int(np.count_nonzero(want == 255)), turn), what
    assert b.turn() == turn, what
    assert b.board_hash() == golhip.board_hash_np(bits), what
    frame, at = b.view_frame(0, 0, 1, fmt=golhip.VIEW_GRAY8)
    assert at == turn and np.array_equal(frame, want), what


def check_group(boards, want, turn, what=None):
    """The same on a group of strips: the strips' rows, counts and digests add up."""
    bits = pack_bits(want)
    assert np.array_equal(np.concatenate([s.snapshot_bits() for s in boards]), bits), what
    counts = [s.alive_count() for s in boards]
    assert sum(c for c, _ in counts) == int(np.count_nonzero(want == 255)) and all(t == turn for _, t in counts), what
    assert sum(s.board_hash() for s in boards) % 2 ** 64 == golhip.board_hash_np(bits), what
    frame, at = golhip.group_view_frame(boards, 0, 0, 1, fmt=golhip.VIEW_GRAY8)
    assert at == turn and np.array_equal(frame, want), what


def make_strips(W, H, cuts):
    return [golhip.Board(W, H, row0=cuts[i], rows=cuts[i + 1] - cuts[i]) for i in range(len(cuts) - 1)]


# ---------------------------------------------------------------- canonical words: shifts, masks, seams
@pytest.mark.parametrize("op", OPS)
def test_shift_and_edge_masks(op):
    """W = 128 on canonical words: x0 % 32 in {0, 1, 31} and widths around one and
    two words, each stamp on top of the last (a random pattern on a random board)."""
    W, H = 128, H17
    rng = np.random.default_rng(0x57A + op)
    want = fill_random_np(W, H, 0x5EED1000 + op)
    with golhip.Board(W, H) as b:
        b.set_option("wpl", 1)
        b.load_bytes(want)
        for xm in (0, 1, 31):
            for pw in (1, 31, 32, 33, 64, 65):
                cells = pattern(rng, pw, 5)
                b.stamp(cells, 32 + xm, 3, op)
                want = golhip.stamp_np(want, cells, 32 + xm, 3, op)
                check(b, want, 0, (op, xm, pw))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("W,x0,pw", [
    (64, 5, 64), (100, 37, 100),                            # full width off a word boundary: both segments in one word
    (128, 120, 20), (100, 90, 30), (33, 32, 33), (5, 3, 5),  # the x seam
])
def test_x_seam_and_full_width(W, x0, pw, op):
    H = H17
    rng = np.random.default_rng(1000 * W + x0 + op)
    want = fill_random_np(W, H, 0x5EED2000 + W)
    cells = pattern(rng, pw, 6)
    with golhip.Board(W, H) as b:
        b.load_bytes(want)
        b.stamp(cells, x0, 4, op)
        check(b, golhip.stamp_np(want, cells, x0, 4, op), 0, (W, x0, pw, op))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("W,x0,pw", [(128, 17, 40), (100, 90, 30)])
@pytest.mark.parametrize("ph", [5, H17])
def test_y_seam(W, x0, pw, ph, op):
    H = H17
    rng = np.random.default_rng(77 * W + ph + op)
    want = fill_random_np(W, H, 0x5EED3000 + W)
    cells = pattern(rng, pw, ph)
    with golhip.Board(W, H) as b:
        b.load_bytes(want)
        b.stamp(cells, x0, 15, op)
        check(b, golhip.stamp_np(want, cells, x0, 15, op), 0, (W, x0, pw, ph, op))


# ---------------------------------------------------------------- pairs and quads
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("W,wpl", [(128, 2), (256, 4)])
def test_interleaved_layouts(W, wpl, op):
    """Stepped first, so the board lies in pairs / quads: odd corners, patterns
    across a 64-cell and a 128-cell group boundary and across both seams, then
    three more turns."""
    H = H17
    rng = np.random.default_rng(31 * W + op)
    want = fill_random_np(W, H, 0x5EED4000 + W)
    with golhip.Board(W, H) as b:
        b.set_option("wpl", wpl)
        b.load_bytes(want)
        b.step(3)
        want = run_np(want, 3)
        assert b.perf()["words_per_lane"] == wpl
        for x0, y0, pw, ph in ((61, 2, 9, 4), (125, 7, 9, 4), (W - 3, 15, 71, 5), (1, 0, W - 1, 2)):
            cells = pattern(rng, pw, ph)
            b.stamp(cells, x0, y0, op)
            want = golhip.stamp_np(want, cells, x0, y0, op)
            check(b, want, 3, (W, wpl, op, x0))
        b.step(3)
        check(b, run_np(want, 3), 6, (W, wpl, op))


# ---------------------------------------------------------------- the padded torus
@pytest.mark.parametrize("W", [33, 100, 1000])
def test_padded_torus(W):
    H = H17
    rng = np.random.default_rng(W)
    want = fill_random_np(W, H, 0x5EED5000 + W)
    cells = pattern(rng, 20, 6)
    with golhip.Board(W, H) as b:
        b.set_pad_step(1)
        b.load_bytes(want)
        b.step(3)
        want = golhip.stamp_np(run_np(want, 3), cells, W - 10, 14, golhip.STAMP_XOR)
        b.stamp(cells, W - 10, 14, golhip.STAMP_XOR)
        check(b, want, 3, W)
        b.step(3)
        assert b.perf()["pad_launches"] > 0
        check(b, run_np(want, 3), 6, W)


# ---------------------------------------------------------------- the resident kernels
def test_board_on_the_resident_kernels():
    """5120 x 1280 takes K1r by the default plan (tests/test_gpu_lds.py): the
    board changes buffer and lies in pairs when the stamp meets it."""
    W, H = 5120, 1280
    rng = np.random.default_rng(5120)
    want = fill_random_np(W, H, 0x5EED6000)
    cells = pattern(rng, 200, 60)
    with golhip.Board(W, H) as b:
        b.load_bytes(want)
        b.step(3)
        p = b.perf()
        assert p["persist_launches"] == 1 and p["lds_launches"] == 1, p
        want = golhip.stamp_np(run_np(want, 3), cells, W - 77, H - 13, golhip.STAMP_COPY)
        b.stamp(cells, W - 77, H - 13, golhip.STAMP_COPY)
        b.step(3)
        assert b.perf()["lds_launches"] == 2
        check(b, run_np(want, 3), 6)


# ---------------------------------------------------------------- row strips
@pytest.mark.parametrize("W,pad", [(128, False), (100, True)])
def test_strips(W, pad):
    H, cuts = 50, [0, 7, 17, 50]
    rng = np.random.default_rng(50 + W)
    want = fill_random_np(W, H, 0x5EED7000 + W)
    strips = make_strips(W, H, cuts)
    try:
        if pad:
            golhip.group_set_pad_step(strips, 1)
        for s in strips:
            s.fill_random(0x5EED7000 + W)
        # across the y seam (rows 45 .. 49 of the last strip, 0 .. 6 of the first), the x seam too
        cells = pattern(rng, 40, 12)
        golhip.group_stamp(strips, cells, W - 9, 45, golhip.STAMP_XOR)
        want = golhip.stamp_np(want, cells, W - 9, 45, golhip.STAMP_XOR)
        # across both inner strip boundaries (rows 5 .. 19)
        cells = pattern(rng, 33, 15)
        golhip.group_stamp(strips, cells, 31, 5, golhip.STAMP_COPY)
        want = golhip.stamp_np(want, cells, 31, 5, golhip.STAMP_COPY)
        check_group(strips, want, 0, W)
        golhip.group_step(strips, 3)
        want = run_np(want, 3)
        check_group(strips, want, 3, W)
        if pad:
            assert strips[0].perf()["pad_launches"] > 0
        # mid-run, and one strip alone: only that strip's rows take the pattern
        cells = pattern(rng, 50, 30)
        strips[1].stamp(cells, 90, 40, golhip.STAMP_OR)  # torus rows 40 .. 49, 0 .. 19: the strip owns 7 .. 16
        full = golhip.stamp_np(want, cells, 90, 40, golhip.STAMP_OR)
        want = want.copy()
        want[7:17] = full[7:17]
        check_group(strips, want, 3, W)
        golhip.group_step(strips, 3)
        check_group(strips, run_np(want, 3), 6, W)
    finally:
        for s in strips:
            s.close()


# ---------------------------------------------------------------- what a stamp keeps and drops
def test_state_after_a_stamp():
    W, H = 128, H17
    rng = np.random.default_rng(9)
    want = fill_random_np(W, H, 0x5EED8000)
    cells = pattern(rng, 30, 5)
    with golhip.Board(W, H) as b:
        b.load_bytes(want)
        with pytest.raises(golhip.GolHipError) as e0:  # flips() of a freshly loaded board: what a stamp goes back to
            b.flips()
        b.step(5, want_flips=True)
        want = run_np(want, 5)
        assert len(b.flips()) > 0
        assert b.alive_count() == (int(np.count_nonzero(want == 255)), 5)  # the cached count of turn 5
        b.stamp(cells, 100, 14, golhip.STAMP_COPY)
        want = golhip.stamp_np(want, cells, 100, 14, golhip.STAMP_COPY)
        assert b.turn() == 5
        assert b.alive_count() == (int(np.count_nonzero(want == 255)), 5)  # recounted
        with pytest.raises(golhip.GolHipError) as e1:
            b.flips()
        assert e1.value.code == e0.value.code == golhip.GOLHIP_EINVAL and str(e1.value) == str(e0.value)
        check(b, want, 5)
        b.step(1, want_flips=True)
        old, want = want, run_np(want, 1)
        ys, xs = np.nonzero(old != want)
        assert np.array_equal(b.flips(), np.stack([xs, ys], axis=1))
        check(b, want, 6)


# ---------------------------------------------------------------- the grid-stride loop
def test_second_lap_of_the_grid():
    """One pattern of more encode units than the grid holds in a lap, on a board
    just large enough for it: canonical words (W % 64 != 0), so a unit is a word."""
    W, H = 8160, 4200
    rng = np.random.default_rng(8160)
    cells = rng.integers(0, 256, size=(H, W), dtype=np.uint8) < 77
    x0, y0 = 37, 11
    # the first column segment of the first row interval alone: words 1 .. 254 of H - y0 rows
    assert (W // 32 - 1) * (H - y0) > STAMP_GRID_CAP_UNITS
    with golhip.Board(W, H) as b:
        b.clear()
        assert b.perf()["words_per_lane"] == 1
        b.stamp(cells, x0, y0, golhip.STAMP_OR)
        want = np.where(np.roll(np.roll(cells, y0, axis=0), x0, axis=1), 255, 0).astype(np.uint8)
        assert np.array_equal(want, golhip.stamp_np(np.zeros((H, W), dtype=np.uint8), cells, x0, y0, golhip.STAMP_OR))
        check(b, want, 0)


# ---------------------------------------------------------------- clear and files
def test_clear():
    W, H = 100, H17
    rng = np.random.default_rng(100)
    zeros = np.zeros((H, W), dtype=np.uint8)
    cells = pattern(rng, 37, 9)
    with golhip.Board(W, H) as b:
        b.fill_random(1)
        b.step(4)
        b.clear()
        check(b, zeros, 0)
        b.stamp(cells, 80, 12, golhip.STAMP_OR)
        check(b, golhip.stamp_np(zeros, cells, 80, 12, golhip.STAMP_OR), 0)
    with golhip.Board(W, H) as b:  # a handle never loaded: clear gives it its board
        b.clear()
        check(b, zeros, 0)


@pytest.mark.parametrize("cuts", [None, [0, 30, 64]])
def test_stamp_file_glider_across_both_seams(tmp_path, cuts):
    W = H = 64
    path = tmp_path / "glider.rle"
    path.write_text(GLIDER)
    glider = golhip.rle_parse_np(GLIDER)
    zeros = np.zeros((H, W), dtype=np.uint8)
    boards = [golhip.Board(W, H)] if cuts is None else make_strips(W, H, cuts)
    try:
        for b in boards:
            b.clear()
        info = golhip.stamp_file(boards if cuts else boards[0], str(path), 62, 62, golhip.STAMP_OR)
        assert info == {"width": 3, "height": 3, "alive": 5, "format": "rle"}
        want = golhip.stamp_np(zeros, glider, 62, 62, golhip.STAMP_OR)
        check_group(boards, want, 0)
        golhip.group_step(boards, 4) if cuts else boards[0].step(4)
        want = run_np(want, 4)
        # four turns move a glider one cell down and right
        assert np.array_equal(want, golhip.stamp_np(zeros, glider, 63, 63, golhip.STAMP_OR))
        check_group(boards, want, 4)
        # a pattern larger than the board is refused before its cells are read
        big = tmp_path / "big.rle"
        big.write_text("x = 65, y = 1\n65o!\n")
        with pytest.raises(golhip.GolHipError) as e:
            golhip.stamp_file(boards, str(big), 0, 0)
        assert e.value.code == golhip.GOLHIP_EINVAL and "does not fit" in str(e.value)
        check_group(boards, want, 4)
    finally:
        for b in boards:
            b.close()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_board_unchanged():
    W, H = 100, H17
    want = fill_random_np(W, H, 0x5EED9000)
    one = np.ones((1, 1), dtype=bool)
    with golhip.Board(W, H) as b:
        b.load_bytes(want)
        b.step(2)
        want = run_np(want, 2)
        cases = {
            "pw > W": lambda: b.stamp(np.ones((1, W + 1), dtype=bool), 0, 0),
            "ph > H": lambda: b.stamp(np.ones((H + 1, 1), dtype=bool), 0, 0),
            "x0 = W": lambda: b.stamp(one, W, 0),
            "y0 = -1": lambda: b.stamp(one, 0, -1),
            "x0 = -1": lambda: b.stamp(one, -1, 0),
            "y0 = H": lambda: b.stamp(one, 0, H),
            "op = 4": lambda: b.stamp(one, 0, 0, 4),
            "op = -1": lambda: b.stamp(one, 0, 0, -1),
            "pw = 0": lambda: b.stamp_bits(np.zeros(0, dtype=np.uint32), 0, 1, 0, 0),
            "null words": lambda: b.stamp_bits(None, 1, 1, 0, 0),
        }
        for name, call in cases.items():
            with pytest.raises(golhip.GolHipError) as e:
                call()
            assert e.value.code == golhip.GOLHIP_EINVAL, (name, str(e.value))
        check(b, want, 2)
    with golhip.Board(W, H) as b:  # never loaded
        with pytest.raises(golhip.GolHipError) as e:
            b.stamp(one, 0, 0)
        assert e.value.code == golhip.GOLHIP_EINVAL and "no board" in str(e.value)
    strips = make_strips(W, H, [0, 5, H])
    try:
        strips[0].clear()  # the second strip has no board
        with pytest.raises(golhip.GolHipError) as e:
            golhip.group_stamp(strips, one, 0, 0)
        assert e.value.code == golhip.GOLHIP_EINVAL
    finally:
        for s in strips:
            s.close()
