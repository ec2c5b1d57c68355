"""The checkpoint kernels (K8, csrc/gol_ckpt.hip, with csrc/golhip_ckpt.cpp;
DESIGN.md §5.16) at their block, chunk, tail and padding edges.

tests/test_gpu_ckpt.py pins what a checkpoint is; its largest board is 128
16-byte groups, one workgroup, one chunk.  Here the sizes and states at which
the kernels and the host path take another branch are the subject:
  A  more than one block, more than one lap of the grid-stride loop, more than
     one automatic chunk in the drain and in the load;
  B  every tail (0..3 words), row widths of 1..7 words, and the padding mask of
     the load kernel at every lane position k = 0..3 and in the scalar tail;
  C  the layout a handle holds at checkpoint time (h->il) where it is not the
     layout it would step in next (want_il);
  D  strips of padded widths, with tails, of one row;
  E  what a handle forgets and keeps across a load, and ringed handles.
Bar: exact equality with numpy (golhip.checkpoint_*_np, board_hash_np,
view_frame_np) and the oracle.  Every test asserts the arithmetic its premise
rests on before it touches the device: a retuned kernel fails it loudly.
"""
import functools
import os
import tempfile

import numpy as np
import pytest

from oracle.oracle import fill_random_np, flips_np, pack_bits, run_np, step_np, unpack_bits

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

LANES = 256              # ckpt_blocks(), gol_ckpt.hip: blocks of 256 lanes (__launch_bounds__(256))
MAX_BLOCKS = 4096        # ckpt_blocks(), gol_ckpt.hip: the grid's cap; past it the loop strides
GROUP_WORDS = 4          # gol_ckpt_kernel / gol_ckpt_load_kernel: a lane owns one 16-byte group
CHUNK_BYTES = 16 << 20   # kChunkBytes, golhip_ckpt.cpp: the automatic chunk is the rows that fit
HEADER_BYTES = 64        # golckpt::kHeaderBytes, gol_ckpt_file.h (golhip.CKPT_HEADER_BYTES)

SEED = 0xC0FFEE


def geometry(W, H):
    """What ckpt_blocks(), the kernels' loops and chunk_rows_for() make of a whole W x H board."""
    Ww = (W + 31) // 32
    nwords = Ww * H
    groups = nwords // GROUP_WORDS
    blocks = max(1, min(-(-groups // LANES), MAX_BLOCKS))
    chunk = max(1, CHUNK_BYTES // (4 * Ww))
    return {"Ww": Ww, "nwords": nwords, "groups": groups, "tail": nwords % GROUP_WORDS, "blocks": blocks,
            "laps": max(1, -(-groups // (blocks * LANES))), "chunk": chunk, "nchunks": -(-H // chunk)}


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum(dtype=np.int64))


def assert_words(got, want, W, H, what):
    """Equality of two boards of canonical words; a mismatch names where the
    kernel and the host path were: word, group, grid lap, row and chunk."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    g = geometry(W, H)
    i = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
    row = i // g["Ww"]
    where = "the scalar tail" if i >= GROUP_WORDS * g["groups"] else \
        f"group {i // GROUP_WORDS} (k = {i % GROUP_WORDS}), grid lap {i // GROUP_WORDS // (MAX_BLOCKS * LANES)}"
    pytest.fail(f"{what}: {int(np.count_nonzero(got != want))} words differ, the first is word {i} in {where}, "
                f"row {row}, chunk {row // g['chunk']} of {g['nchunks']}: "
                f"{int(got.reshape(-1)[i]):#010x}, expected {int(want.reshape(-1)[i]):#010x}")


def board(W, H, wpl=0, **kw):
    b = golhip.Board(W, H, **kw)
    if wpl:
        b.set_option("wpl", wpl)
    return b


def strips(W, H, cuts, wpl=0):
    return [board(W, H, wpl, row0=a, rows=e - a) for a, e in zip(cuts[:-1], cuts[1:])]


def close_all(bs):
    for b in bs:
        b.close()


@functools.lru_cache(maxsize=None)
def ref(W, H, turns, seed=SEED):
    """fill_random(seed) after `turns` turns (0/255 bytes); computed once, shared read-only."""
    b = fill_random_np(W, H, seed) if turns == 0 else step_np(ref(W, H, turns - 1, seed))
    b.setflags(write=False)
    return b


def ref_words(W, H, turns, seed=SEED):
    return pack_bits(ref(W, H, turns, seed))


def np_file(W, H, turns, seed=SEED):
    """The bytes golhip.checkpoint_write_np writes for ref(W, H, turns)."""
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "np.ckpt")
        golhip.checkpoint_write_np(p, ref_words(W, H, turns, seed), W, H, turns)
        with open(p, "rb") as f:
            return f.read()


def read(path):
    with open(path, "rb") as f:
        return f.read()


def write_as_it_stands(path, words, W, H, turn):
    """A file whose header is sound and matches the payload as it stands,
    padding bits included (so only the load kernel's own mask can refuse it)."""
    with open(path, "wb") as f:
        f.write(golhip.checkpoint_header_np(W, H, turn, popcount(words), golhip.board_hash_np(words)))
        f.write(np.ascontiguousarray(words, dtype="<u4").tobytes())
    assert golhip.checkpoint_info(path)["alive"] == popcount(words)


def assert_corrupt(boards, path):
    with pytest.raises(golhip.GolHipError) as e:
        golhip.checkpoint_load(boards, path)
    assert e.value.code == golhip.GOLHIP_ECORRUPT, str(e.value)


# ---------------------------------------------------------------- A: past one block, one lap, one chunk
# (W, H, wpl of the checkpointed board, wpl of the board the file is loaded into, premise)
BIG = [(8192, 16385, 1, 2, "lap"), (8192, 16385, 2, 4, "lap"), (8192, 16385, 4, 1, "lap"), (8200, 16385, 0, 0, "lap-tail"),
       (1024, 33, 0, 4, "blocks"), (1024, 2049, 1, 4, "blocks"), (1024, 2049, 2, 1, "blocks"), (1024, 2049, 4, 2, "blocks"),
       (1024, 8193, 1, 2, "blocks")]


@functools.lru_cache(maxsize=2)
def big_case(W, H):
    """Random words with the padding of each row's last word cleared, their
    count and digest, and the file numpy writes for them at turn 0."""
    Ww = (W + 31) // 32
    words = np.random.default_rng(W * 7 + H).integers(0, 1 << 32, (H, Ww), dtype=np.uint32)
    if W % 32:
        words[:, -1] &= np.uint32((1 << (W % 32)) - 1)
    words.setflags(write=False)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "np.ckpt")
        golhip.checkpoint_write_np(p, words, W, H, 0)
        data = read(p)
    return words, popcount(words), golhip.board_hash_np(words), data


@functools.lru_cache(maxsize=1)
def big_after_3(W, H):
    got = pack_bits(run_np(unpack_bits(big_case(W, H)[0], W), 3))
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("W,H,wpl,wpl2,premise", BIG)
def test_past_one_block_lap_and_chunk(tmp_path, W, H, wpl, wpl2, premise):
    """A checkpoint at turn 0 of random words, default chunk_rows, and its
    load into a board of another layout.
    8192 x 16385 (canonical, pairs, quads): 4,194,560 words, 1,048,640 groups,
    64 of them in the second lap of the 4096 x 256 grid, all in the last row;
    the automatic chunk is 16384 rows: two chunks, the second of one row.
    8200 x 16385 (generic, Ww 257, padding): 4,210,945 words, two laps and a
    tail of one word; chunks of 16320 and 65 rows.
    1024 x 33: 264 groups, two blocks, the second with 8 lanes at work.
    1024 x 2049: 16,392 groups, 65 blocks, the last with 8 lanes at work.
    1024 x 8193: 65,544 groups, 257 blocks."""
    g = geometry(W, H)
    if premise == "blocks":
        assert g["blocks"] >= 2 and g["laps"] == 1 and g["groups"] % LANES != 0, g
        assert g["blocks"] == {33: 2, 2049: 65, 8193: 257}[H], g
    else:
        assert g["groups"] > MAX_BLOCKS * LANES and g["blocks"] == MAX_BLOCKS and g["laps"] == 2, g
        assert H > g["chunk"] and g["nchunks"] == 2, g
        if premise == "lap":
            second_lap = g["groups"] - MAX_BLOCKS * LANES
            assert second_lap == 64 and GROUP_WORDS * MAX_BLOCKS * LANES >= (H - 1) * g["Ww"] and g["tail"] == 0, g
            assert g["chunk"] == 16384 and H - g["chunk"] == 1, g
        else:
            assert g["tail"] == 1 and g["Ww"] == 257 and W % 32 != 0, g
            assert g["chunk"] == 16320 and H - g["chunk"] == 65, g
    words, alive, digest, np_bytes = big_case(W, H)
    assert len(np_bytes) == HEADER_BYTES + 4 * g["nwords"]
    path = str(tmp_path / "a.ckpt")
    with board(W, H, wpl) as b, board(W, H, wpl2) as c:
        b.load_bits(words)
        info = golhip.checkpoint_begin(b, path).wait()
        assert not os.path.exists(path + ".tmp")
        finfo, got = golhip.checkpoint_read_np(path, verify=False)
        assert_words(got, words, W, H, "the file")
        assert (finfo["turn"], finfo["alive"], finfo["hash"]) == (0, alive, digest)
        assert {k: info[k] for k in finfo} == finfo
        assert b.board_hash() == digest and b.alive_count() == (alive, 0)
        assert read(path) == np_bytes
        assert golhip.checkpoint_load(c, path) == finfo
        assert_words(c.snapshot_bits(), words, W, H, "the loaded board")
        assert c.board_hash() == digest and c.alive_count() == (alive, 0) and c.turn() == 0
        if premise == "blocks":
            want = big_after_3(W, H)
            for x in (b, c):
                x.step(3)
                assert_words(x.snapshot_bits(), want, W, H, "three turns on")
        else:  # (the same engine twice: the loaded layout is the one its step kernel expects)
            b.step(1)
            c.step(1)
            assert b.board_hash() == c.board_hash() and b.alive_count() == c.alive_count()
        if W % 64 == 0:
            assert c.perf()["words_per_lane"] == wpl2
            assert b.perf()["words_per_lane"] == (wpl or b.perf()["words_per_lane"]) != wpl2


# ---------------------------------------------------------------- B: tails, row widths, the padding mask
# (W, H, words a row, words, tail)
SMALL = [(17, 9, 1, 9, 1), (33, 7, 2, 14, 2), (70, 5, 3, 15, 3), (100, 7, 4, 28, 0), (150, 5, 5, 25, 1), (200, 9, 7, 63, 3),
         (32, 5, 1, 5, 1), (96, 7, 3, 21, 1)]
PADDED = [s for s in SMALL if s[0] % 32]


def last_word_class(W, H, row):
    """Where the load kernel meets the last word of `row`: the lane position
    k = 0..3 of its 16-byte group, or "tail" behind the last whole group."""
    g = geometry(W, H)
    i = row * g["Ww"] + g["Ww"] - 1
    return "tail" if i >= GROUP_WORDS * (g["nwords"] // GROUP_WORDS) else i % GROUP_WORDS


@pytest.mark.parametrize("turns", [(0,), (7,), (7, 1)], ids=["0", "7", "7+1"])
@pytest.mark.parametrize("W,H,Ww,nwords,tail", SMALL)
def test_small_round_trip(tmp_path, W, H, Ww, nwords, tail, turns):
    """Turn 0 (no step at all), turn 7, and turn 8 as 7 + 1 (the board in the
    other buffer than after 7): the file is numpy's, and a load steps on."""
    g = geometry(W, H)
    assert (g["Ww"], g["nwords"], g["tail"], g["blocks"]) == (Ww, nwords, tail, 1)
    t = sum(turns)
    path = str(tmp_path / "a.ckpt")
    with board(W, H) as b:
        b.fill_random(SEED)
        for n in turns:
            if n:
                b.step(n)
        info = golhip.checkpoint_begin(b, path).wait()
        assert b.turn() == t and b.board_hash() == info["hash"] and b.alive_count() == (info["alive"], t)
    finfo, words = golhip.checkpoint_read_np(path)
    assert_words(words, ref_words(W, H, t), W, H, "the file")
    assert finfo["turn"] == t
    assert read(path) == np_file(W, H, t)
    with board(W, H) as c:
        assert golhip.checkpoint_load(c, path) == finfo
        assert c.turn() == t and c.board_hash() == finfo["hash"] and c.alive_count() == (finfo["alive"], t)
        assert_words(c.snapshot_bits(), ref_words(W, H, t), W, H, "the loaded board")
        c.step(5)
        assert c.turn() == t + 5
        assert np.array_equal(c.snapshot_bytes(), ref(W, H, t + 5))


def test_padding_shapes_reach_every_position():
    """Over the rows of the padded shapes the last word of a row falls on
    k = 0, 1, 2 and 3 of a group and in the scalar tail; 17 wide has one word a
    row (every word a last word), 33 wide two (the column wraps inside a group)."""
    seen = {last_word_class(W, H, r) for W, H, *_ in PADDED for r in range(H)}
    assert seen == {0, 1, 2, 3, "tail"}
    assert {s[2] for s in PADDED} == {1, 2, 3, 4, 5, 7}
    assert {last_word_class(100, 7, r) for r in range(7)} == {3}
    assert {last_word_class(17, 9, r) for r in range(9)} == {0, 1, 2, 3, "tail"}


@pytest.mark.parametrize("W,H,Ww,nwords,tail", PADDED)
def test_one_padding_bit_in_one_row_is_refused(tmp_path, W, H, Ww, nwords, tail):
    """A file whose only defect is one bit of a column >= width in one row's
    last word, its header made to match: GOLHIP_ECORRUPT for every row, for the
    first padding bit and for bit 31.  One position at a time: the check is an
    inequality of sums, so only a single dirty word proves that its position
    (k of the group, or the scalar tail) is masked.  The clean file loads in
    between, so nothing passes merely because everything is refused."""
    assert geometry(W, H)["Ww"] == Ww and W % 32
    clean = ref_words(W, H, 7)
    good, bad = str(tmp_path / "good.ckpt"), str(tmp_path / "bad.ckpt")
    golhip.checkpoint_write_np(good, clean, W, H, 7)
    ginfo = golhip.checkpoint_info(good)
    tried = set()
    with board(W, H) as c:
        for row in range(H):
            for bit in sorted({W % 32, (W % 32 + 31) // 2, 31}):
                words = clean.copy()
                words[row, -1] |= np.uint32(1 << bit)
                assert popcount(words) == ginfo["alive"] + 1
                write_as_it_stands(bad, words, W, H, 7)
                with pytest.raises(golhip.GolHipError) as e:
                    golhip.checkpoint_load(c, bad)
                assert e.value.code == golhip.GOLHIP_ECORRUPT, (row, bit, last_word_class(W, H, row), str(e.value))
                tried.add(last_word_class(W, H, row))
            assert golhip.checkpoint_load(c, good) == ginfo
            assert c.board_hash() == ginfo["hash"] and c.alive_count() == (ginfo["alive"], 7)
    assert tried == {last_word_class(W, H, r) for r in range(H)}


# ---------------------------------------------------------------- C: the layout held at checkpoint time
LAYOUT_SHAPES = [(256, 9), (128, 6)]


def load_everywhere_and_step(path, W, H, t):
    """The file into a board of each layout; five turns on it is the oracle's board."""
    finfo = golhip.checkpoint_info(path)
    for wpl in (1, 2, 4):
        with board(W, H, wpl) as c:
            assert golhip.checkpoint_load(c, path) == finfo
            assert c.turn() == t and c.board_hash() == finfo["hash"]
            c.step(5)
            assert c.perf()["words_per_lane"] == wpl
            assert np.array_equal(c.snapshot_bytes(), ref(W, H, t + 5)), wpl


@pytest.mark.parametrize("how", ["load_bytes", "load_bits", "fill_random"])
@pytest.mark.parametrize("wpl", [2, 4])
@pytest.mark.parametrize("W,H", LAYOUT_SHAPES)
def test_layout_at_turn_0(tmp_path, W, H, wpl, how):
    """No step before the checkpoint: the layout is what the load left (pairs
    or quads, converted in place), and after set_option("wpl", 1) it still is,
    while the layout the handle would step in (want_il) is canonical."""
    assert W % 128 == 0  # (both layouts exist at this width: wpl_for(), golhip_plan.cpp)
    path, path2 = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    with board(W, H, wpl) as b:
        if how == "fill_random":
            b.fill_random(SEED)
        elif how == "load_bits":
            b.load_bits(ref_words(W, H, 0))
        else:
            b.load_bytes(ref(W, H, 0))
        assert golhip.checkpoint_begin(b, path).wait()["turn"] == 0
        b.set_option("wpl", 1)
        assert golhip.checkpoint_begin(b, path2).wait()["turn"] == 0
        b.step(5)
        assert b.perf()["words_per_lane"] == 1 and np.array_equal(b.snapshot_bytes(), ref(W, H, 5))
    assert read(path) == np_file(W, H, 0)
    assert read(path2) == np_file(W, H, 0)
    load_everywhere_and_step(path, W, H, 0)


@pytest.mark.parametrize("wpl,other", [(1, 2), (2, 1), (2, 4), (4, 2), (1, 4), (4, 1)])
@pytest.mark.parametrize("W,H", LAYOUT_SHAPES)
def test_layout_option_changed_after_stepping(tmp_path, W, H, wpl, other):
    """Seven turns in one layout, then the option names another, then the
    checkpoint before any further step: the rows still lie in the first."""
    path = str(tmp_path / "a.ckpt")
    with board(W, H, wpl) as b:
        b.fill_random(SEED)
        b.step(7)
        assert b.perf()["words_per_lane"] == wpl
        b.set_option("wpl", other)
        assert golhip.checkpoint_begin(b, path).wait()["turn"] == 7
        b.step(5)  # the board was not disturbed, and converts for its next launch as before
        assert b.perf()["words_per_lane"] == other and np.array_equal(b.snapshot_bytes(), ref(W, H, 12))
    assert read(path) == np_file(W, H, 7)
    load_everywhere_and_step(path, W, H, 7)


# ---------------------------------------------------------------- D: strips with padding, tails, one row
# (W, H, wpl, the cuts checkpointed, the cuts loaded into, their wpl)
STRIPS = [(70, 11, 0, (0, 1, 4, 11), [(0, 11), (0, 10, 11), (0, 5, 6, 11)], 0),
          (200, 9, 0, (0, 2, 9), [(0, 9), (0, 8, 9), (0, 1, 5, 9)], 0),
          (256, 10, 4, (0, 1, 10), [(0, 10), (0, 9, 10), (0, 3, 4, 10)], 2)]


@pytest.mark.parametrize("W,H,wpl,cuts,load_cuts,load_wpl", STRIPS)
def test_strips_with_padding_tails_and_one_row(tmp_path, W, H, wpl, cuts, load_cuts, load_wpl):
    """70 x 11 as strips of 1, 3 and 7 rows: 3, 9 and 21 words, a tail behind
    every strip's groups, the first strip without one whole group.  200 x 9:
    Ww 7.  256 x 10 in quads with a one-row strip.  group_step plans one-row
    strips at padded widths (depth 1, one halo row an exchange), so none of the
    strips here needs a second row."""
    Ww = geometry(W, H)["Ww"]
    per_strip = [(e - a) * Ww for a, e in zip(cuts[:-1], cuts[1:])]
    assert (1 in [e - a for a, e in zip(cuts[:-1], cuts[1:])]) == (cuts[1] == 1)  # (200 x 9 is cut 2 + 7)
    if W == 70:
        assert per_strip == [3, 9, 21] and all(n % GROUP_WORDS for n in per_strip)
    assert all(len(c) - 1 == n for c, n in zip(load_cuts, (1, 2, 3))) and cuts not in load_cuts
    assert all(1 in [e - a for a, e in zip(c[:-1], c[1:])] for c in load_cuts[1:])
    whole = np_file(W, H, 7)
    bs = strips(W, H, cuts, wpl)
    try:
        for b in bs:
            b.fill_random(SEED)
        golhip.group_step(bs, 7)
        for name, chunk in (("one.ckpt", 1), ("auto.ckpt", 0)):
            info = golhip.checkpoint_begin(bs, str(tmp_path / name), chunk_rows=chunk).wait()
            assert info["turn"] == 7
            assert read(str(tmp_path / name)) == whole, name
    finally:
        close_all(bs)
    path = str(tmp_path / "one.ckpt")
    finfo = golhip.checkpoint_info(path)
    for lc in load_cuts:
        cs = strips(W, H, lc, load_wpl)
        try:
            assert golhip.checkpoint_load(cs, path) == finfo
            assert [c.turn() for c in cs] == [7] * len(cs)
            assert sum(c.board_hash() for c in cs) % (1 << 64) == finfo["hash"]
            assert_words(np.concatenate([c.snapshot_bits() for c in cs]), ref_words(W, H, 7), W, H, f"strips {lc}")
            golhip.group_step(cs, 9)
            got = np.concatenate([c.snapshot_bits() for c in cs])
            assert_words(got, ref_words(W, H, 16), W, H, f"strips {lc}, nine turns on")
        finally:
            close_all(cs)


@pytest.mark.parametrize("W,H,wpl,cuts,load_cuts,load_wpl", [s for s in STRIPS if s[0] % 32])
def test_strips_refuse_dirty_padding_in_any_one_strip(tmp_path, W, H, wpl, cuts, load_cuts, load_wpl):
    """Every padding bit set in the rows of one strip, the other strips clean,
    the header matching the payload: each strip's own kernel launch masks."""
    clean = ref_words(W, H, 7)
    pad = np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
    good, bad = str(tmp_path / "good.ckpt"), str(tmp_path / "bad.ckpt")
    golhip.checkpoint_write_np(good, clean, W, H, 7)
    for lc in load_cuts:
        cs = strips(W, H, lc)
        try:
            for a, e in zip(lc[:-1], lc[1:]):
                words = clean.copy()
                words[a:e, -1] |= pad
                write_as_it_stands(bad, words, W, H, 7)
                assert_corrupt(cs, bad)
                assert golhip.checkpoint_load(cs, good)["turn"] == 7
            golhip.group_step(cs, 9)
            got = np.concatenate([c.snapshot_bits() for c in cs])
            assert_words(got, ref_words(W, H, 16), W, H, f"strips {lc}, nine turns on")
        finally:
            close_all(cs)


# ---------------------------------------------------------------- E: what the handle forgets and keeps
HANDLE_SHAPES = [(64, 16, 1), (256, 9, 2)]
OTHER_SEED = 0xBADC0DE


def assert_no_flip_list(b):
    with pytest.raises(golhip.GolHipError) as e:
        b.flips()
    assert e.value.code == golhip.GOLHIP_EINVAL


@pytest.mark.parametrize("before", [3, 7])
@pytest.mark.parametrize("W,H,wpl", HANDLE_SHAPES)
def test_handle_state_across_a_load(tmp_path, W, H, wpl, before):
    """The target board holds a flip list and a cached count of another board
    (at turn 3, and at the file's own turn 7, where only flips_valid tells the
    stale list from a fresh one).  The load stages the file in the other board
    buffer, the one a flip list is computed against: flips() must be refused as
    after load_bits, never answered from it."""
    p7, p12 = str(tmp_path / "7.ckpt"), str(tmp_path / "12.ckpt")
    golhip.checkpoint_write_np(p7, ref_words(W, H, 7), W, H, 7)
    golhip.checkpoint_write_np(p12, ref_words(W, H, 12, OTHER_SEED), W, H, 12)
    alive7 = int(np.count_nonzero(ref(W, H, 7)))
    with board(W, H, wpl) as b:
        b.fill_random(OTHER_SEED)
        b.step(before, want_flips=True)
        assert np.array_equal(b.flips(), flips_np(ref(W, H, before - 1, OTHER_SEED), ref(W, H, before, OTHER_SEED)))
        assert b.alive_count() == (int(np.count_nonzero(ref(W, H, before, OTHER_SEED))), before)
        info = golhip.checkpoint_load(b, p7)
        assert (info["turn"], info["alive"]) == (7, alive7)
        assert_no_flip_list(b)
        assert b.alive_count() == (alive7, 7) and b.turn() == 7
        for fmt in (golhip.VIEW_ARGB, golhip.VIEW_GRAY8):
            frame, turn = b.view_frame(W - 7, H - 3, 3, fmt=fmt)
            assert turn == 7
            assert np.array_equal(frame, golhip.view_frame_np(ref_words(W, H, 7), W, H, W - 7, H - 3, 3, fmt=fmt))
        assert_no_flip_list(b)
        # the four turns behind the file's: the oracle's lists 7 -> 8 ... 10 -> 11
        xy, counts, done = b.flip_stream(4, cap=4 * W * H)
        lists = [flips_np(ref(W, H, t), ref(W, H, t + 1)) for t in range(7, 11)]
        assert done == 4 and [int(c) for c in counts] == [len(x) for x in lists]
        assert np.array_equal(xy, np.concatenate(lists))
        assert b.turn() == 11 and np.array_equal(b.snapshot_bytes(), ref(W, H, 11))
        # a second file over the first
        b.step(1, want_flips=True)
        assert len(b.flips()) == len(flips_np(ref(W, H, 11), ref(W, H, 12)))
        info = golhip.checkpoint_load(b, p12)  # (the board is at turn 12 itself: again only flips_valid tells)
        assert info["turn"] == 12 and b.turn() == 12
        assert_no_flip_list(b)
        assert b.alive_count() == (int(np.count_nonzero(ref(W, H, 12, OTHER_SEED))), 12)
        assert_words(b.snapshot_bits(), ref_words(W, H, 12, OTHER_SEED), W, H, "the second file's board")
        b.step(3, want_flips=True)
        assert np.array_equal(b.flips(), flips_np(ref(W, H, 14, OTHER_SEED), ref(W, H, 15, OTHER_SEED)))
        assert np.array_equal(b.snapshot_bytes(), ref(W, H, 15, OTHER_SEED))


@pytest.mark.parametrize("force_halo", [0, 1])
@pytest.mark.parametrize("W,H,wpl", HANDLE_SHAPES)
def test_ringed_handle(tmp_path, W, H, wpl, force_halo):
    """A handle made a one-rank ring: checkpoint_begin refuses it
    (GOLHIP_EINVAL, the message names the ring) and leaves no file;
    checkpoint_load takes it as the whole torus it is (golhip.h), and it steps
    on from the file's turn, through the halo path too."""
    d = tmp_path / "out"
    d.mkdir()
    src = str(tmp_path / "7.ckpt")
    golhip.checkpoint_write_np(src, ref_words(W, H, 7), W, H, 7)
    with board(W, H, wpl) as b:
        b.comm_init(golhip.unique_id(), 1, 0)
        b.set_option("force_halo", force_halo)
        b.fill_random(OTHER_SEED)
        b.step(2)
        with pytest.raises(golhip.GolHipError) as e:
            golhip.checkpoint_begin(b, str(d / "no.ckpt"))
        assert e.value.code == golhip.GOLHIP_EINVAL and "ring" in str(e.value)
        assert os.listdir(d) == []
        assert np.array_equal(b.snapshot_bytes(), ref(W, H, 2, OTHER_SEED))  # the refusal left the board alone
        info = golhip.checkpoint_load(b, src)
        assert info == golhip.checkpoint_info(src)
        assert b.turn() == 7 and b.alive_count() == (info["alive"], 7) and b.board_hash() == info["hash"]
        b.step(5)
        assert b.turn() == 12 and np.array_equal(b.snapshot_bytes(), ref(W, H, 12))
