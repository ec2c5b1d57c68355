"""The CellFlipped stream of boards whose width is no multiple of 32 on the
fused turn + list kernels (K5 per turn, K5r resident): the
kernel closes the row seam in the row's first and last word
(csrc/gol_flip_seam.h), so golhip_flip_stream, golhip_step_flips and
golhip_group_flip_stream run such boards exactly as they run the others --
no any-width kernel, no three-pass compaction, no padded torus.

Every list is compared with the oracle's turn by turn (initializeAliveCells,
gol/distributor.go:212-220: one CellFlipped per changed cell, row-major), and
perf()["flip_launches"] shows that the fused kernel did the work.
"""
import functools

import numpy as np
import pytest

from oracle.oracle import COracle, flips_np, pack_bits, pgm_bytes, step_np

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

BATCHES = (1, 5, 17, 3)
TURNS = sum(BATCHES)

SHAPES = [
    (16, 16),                   # Ww = 1: both seam fixes on one word
    (1, 5), (2, 4), (3, 7),     # coinciding neighbours
    (33, 9), (63, 4),           # r = 1 and r = 31, strided branch
    (48, 48),                   # the reference-sized generic case
    (100, 37), (127, 3),        # Ww = 4: the CONTIG branch, r = 4 and r = 31
    (97, 1),                    # one row
    (2081, 3),                  # Ww = 66: a strided row longer than a wave
    (8191, 2),                  # Ww = 256: a CONTIG row is exactly one wave (lane 63 is wave edge and row edge)
    (1000, 40),                 # 1280 words: two blocks, CONTIG
    (4100, 9),                  # Ww = 129, 1161 words: a row straddles the block boundary, strided branch
]


@functools.lru_cache(maxsize=None)
def oracle():
    return COracle()


def soup(W, H, seed, p=0.35):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((H, W)) < p, 255, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def truth(W, H, seed, turns):
    """(boards 0..turns, lists of turns 1..turns) of the soup, computed once and never written."""
    boards, lists = [soup(W, H, seed)], []
    for _ in range(turns):
        nxt = step_np(boards[-1])
        lists.append(flips_np(boards[-1], nxt))
        boards.append(nxt)
    for a in boards + lists:
        a.setflags(write=False)
    return boards, lists


def seed_of(W, H):
    return 7000 * W + H


def idx_to_xy(idx, W):
    idx = idx.astype(np.int64)
    return np.stack([idx % W, idx // W], axis=1).astype(np.int32)


def alive(board):
    return int(np.count_nonzero(board == 255))


def split(ent, counts, fmt, W):
    """The per-turn lists of a call as (x, y) pairs."""
    xy = ent if fmt == 0 else idx_to_xy(ent, W)
    out, off = [], 0
    for c in counts:
        out.append(xy[off:off + int(c)].copy())
        off += int(c)
    assert off == len(xy)
    return out


def check_board(b, want, turns, what):
    """The board, its count, its bit words (padding zero) and its hash against a fresh handle's."""
    H, W = want.shape
    assert np.array_equal(b.snapshot_bytes(), want), what
    assert b.alive_count() == (alive(want), turns), what
    bits = b.snapshot_bits()
    pad = np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
    assert not (bits[:, -1] & pad).any(), what
    assert np.array_equal(bits, pack_bits(want)), what
    with golhip.Board(W, H) as ref:
        ref.load_bytes(want)
        assert b.board_hash() == ref.board_hash() == golhip.board_hash_np(pack_bits(want)), what


# ---------------------------------------------------------------- one handle
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("W,H", SHAPES)
def test_flip_stream_matches_oracle(W, H, fmt):
    boards, lists = truth(W, H, seed_of(W, H), TURNS)
    with golhip.Board(W, H) as b:
        b.load_bytes(boards[0])
        t = 0
        for k in BATCHES:
            ent, counts, done = b.flip_stream(k, cap=k * W * H, fmt=fmt)
            assert done == k and len(counts) == k and int(counts.sum()) == len(ent)
            for got in split(ent, counts, fmt, W):
                assert np.array_equal(got, lists[t]), (W, H, t)
                t += 1
        p = b.perf()
        assert p["flip_launches"] == TURNS and p["pad_launches"] == 0, p
        assert p["flip_entries"] == sum(len(x) for x in lists), p
        check_board(b, boards[TURNS], TURNS, (W, H, fmt))
        b.step(7)  # the per-launch kernels continue from the stream's board
        assert np.array_equal(b.snapshot_bytes(), oracle().run(boards[TURNS], 7))


@pytest.mark.parametrize("W,H,fmt", [(100, 37, 0), (1000, 40, 1)])
def test_flip_stream_stops_without_loss(W, H, fmt):
    """A small buffer: each call runs the turns that fit, the rest follow in
    the next calls; the concatenation equals the oracle's stream."""
    boards, lists = truth(W, H, seed_of(W, H), 40)
    cap = max(len(w) for w in lists) * 3
    got, turns, calls = [], 0, 0
    with golhip.Board(W, H) as b:
        b.load_bytes(boards[0])
        while turns < 40:
            ent, counts, done = b.flip_stream(40 - turns, cap=cap, fmt=fmt)
            assert 1 <= done <= 40 - turns and len(ent) <= cap
            got += split(ent, counts, fmt, W)
            turns += done
            calls += 1
            assert b.alive_count() == (alive(boards[turns]), turns)
            assert np.array_equal(b.snapshot_bytes(), boards[turns])
        assert calls > 5
        assert b.perf()["pad_launches"] == 0
    assert len(got) == 40
    for t in range(40):
        assert np.array_equal(got[t], lists[t]), t


@pytest.mark.parametrize("fmt,overlap,shift", [(0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 3), (0, 1, 1), (0, 3, 0),
                                               (1, 3, 0), (0, 3, 1), (1, 3, 3)])
def test_flip_stream_into_pinned_host_buffer(fmt, overlap, shift):
    """out inside a golhip_host_alloc buffer at every flip_overlap mode (0: the
    turn's blocks store there; 1: copy blocks of the next launch; 3: K5r, one
    resident launch a batch), `shift` entries into the buffer."""
    W, H = 1000, 40
    boards, lists = truth(W, H, seed_of(W, H), 40)
    cap = max(len(w) for w in lists[:30]) * 4
    buf = golhip.host_array((cap + shift, 2) if fmt == 0 else (cap + shift,), np.int32 if fmt == 0 else np.uint32)
    out = buf[shift:]
    got = []
    with golhip.Board(W, H) as b:
        b.set_option("flip_overlap", overlap)
        b.load_bytes(boards[0])
        while len(got) < 30:
            ent, counts, done = b.flip_stream(30 - len(got), cap=cap, fmt=fmt, out=out)
            assert done >= 1
            got += split(ent, counts, fmt, W)
        p = b.perf()
        assert (p["flip_resident_launches"] >= 1) == (overlap == 3), p
        assert p["pad_launches"] == 0 and p["flip_fallbacks"] == 0, p
        check_board(b, boards[30], 30, (fmt, overlap, shift))
    for t in range(30):
        assert np.array_equal(got[t], lists[t]), t
    del out, buf


@pytest.mark.parametrize("fmt", [0, 1])
def test_resident_batch_overflows_in_mid_batch(fmt):
    """K5r with a buffer that holds two turns and a half: the first call has no
    estimate yet and launches all 10 turns, the third overflows, so the board
    the call leaves is K5r's rollback board (turn 2), and the stream goes on
    from it without a lost or repeated entry."""
    W, H = 1000, 40
    boards, lists = truth(W, H, seed_of(W, H), 40)
    cap = len(lists[0]) + len(lists[1]) + len(lists[2]) // 2
    big = max(len(w) for w in lists[:10]) * 8
    buf = golhip.host_array((big, 2) if fmt == 0 else (big,), np.int32 if fmt == 0 else np.uint32)
    with golhip.Board(W, H) as b:
        b.set_option("flip_overlap", 3)
        b.load_bytes(boards[0])
        ent, counts, done = b.flip_stream(10, cap=cap, fmt=fmt, out=buf)
        assert done == 2 and b.perf()["flip_resident_launches"] == 1
        got = split(ent, counts, fmt, W)
        check_board(b, boards[2], 2, "rolled back")
        while len(got) < 10:
            ent, counts, done = b.flip_stream(10 - len(got), cap=big, fmt=fmt, out=buf)
            got += split(ent, counts, fmt, W)
        check_board(b, boards[10], 10, "resumed")
        assert b.perf()["flip_fallbacks"] == 0
    for t in range(10):
        assert np.array_equal(got[t], lists[t]), t
    del buf


def test_step_flips_one_rank_ring():
    """golhip_step_flips through the halo path (one halo row exchanged a turn)."""
    W, H = 100, 37
    boards, lists = truth(W, H, seed_of(W, H), TURNS)
    with golhip.Board(W, H) as b:
        b.comm_init(golhip.unique_id(), 1, 0)
        b.set_option("force_halo", 1)
        b.load_bytes(boards[0])
        xy, counts = b.step_flips(9, cap=9 * W * H)
        assert len(counts) == 9
        for t, got in enumerate(split(xy, counts, 0, W)):
            assert np.array_equal(got, lists[t]), t
        p = b.perf()
        assert p["flip_launches"] == 9 and p["halo_exchanges"] >= 9 and p["pad_launches"] == 0, p
        assert np.array_equal(b.snapshot_bytes(), boards[9])
        assert b.alive_count() == (alive(boards[9]), 9)


# ---------------------------------------------------------------- row strips
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("W,H,n", [(1000, 40, 3), (48, 48, 3), (16, 16, 2), (100, 5, 5), (129, 9, 2)])
def test_group_flip_stream_matches_oracle(W, H, n, fmt):
    """The board on n row strips of one device ((100, 5, 5): one-row strips,
    every input row a halo): K5 per strip and turn, one gather a strip."""
    boards, lists = truth(W, H, seed_of(W, H), TURNS)
    cuts = [H * i // n for i in range(n + 1)]
    bs = []
    try:
        for a, e in zip(cuts[:-1], cuts[1:]):
            st = golhip.Board(W, H, row0=a, rows=e - a)
            bs.append(st)
            st.load_bytes(boards[0][a:e])
        t, total = 0, 0
        for k in BATCHES:
            ent, counts, done = golhip.group_flip_stream(bs, k, cap=k * W * H, fmt=fmt)
            assert done == k and len(counts) == k and int(counts.sum()) == len(ent)
            for got in split(ent, counts, fmt, W):
                assert np.array_equal(got, lists[t]), (W, H, n, t)
                t += 1
            total += len(ent)
        want = boards[TURNS]
        for st, a, e in zip(bs, cuts[:-1], cuts[1:]):
            assert np.array_equal(st.snapshot_bytes(), want[a:e]), (a, e)
            assert np.array_equal(st.snapshot_bits(), pack_bits(want[a:e])), (a, e)  # (padding bits zero)
        counts_at = [st.alive_count() for st in bs]
        assert sum(c for c, _ in counts_at) == alive(want) and all(at == TURNS for _, at in counts_at)
        perf = [st.perf() for st in bs]
        assert all(p["flip_launches"] == TURNS and p["pad_launches"] == 0 for p in perf), perf
        assert sum(p["flip_entries"] for p in perf) == total
        golhip.group_step(bs, 7)
        after = oracle().run(want, 7)
        for st, a, e in zip(bs, cuts[:-1], cuts[1:]):
            assert np.array_equal(st.snapshot_bytes(), after[a:e]), (a, e)
    finally:
        for st in bs:
            st.close()


# ---------------------------------------------------------------- gol.Run
def test_run_events_100x60x30(tmp_path):
    """gol.Run with every CellFlipped of a 100 x 60 board: the events replayed
    onto a shadow board give the oracle's board at every TurnComplete
    (sdl_test.go:93-128)."""
    W, H, turns = 100, 60, 30
    boards, _ = truth(W, H, seed_of(W, H), turns)
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / f"{W}x{H}.pgm").write_bytes(pgm_bytes(boards[0]))
    shadow = np.zeros((H, W), dtype=np.uint8)
    r = golhip.Run(turns, 8, W, H, str(tmp_path))
    seen, final = 0, False
    for ev in r:
        if ev["type"] == "CellFlipped":
            x, y = ev["Cell"]
            shadow[y, x] ^= 255
        elif ev["type"] == "TurnComplete":  # (the initial board's CellFlipped events came before the first turn's)
            seen += 1
            assert ev["CompletedTurns"] == seen
            assert np.array_equal(shadow, boards[seen]), seen
        elif ev["type"] == "FinalTurnComplete":
            final = True
    assert r.wait() == "" and final and seen == turns
    r.close()
