"""The batched CellFlipped stream of a board held as row strips
(golhip_group_flip_stream: K5 per strip and turn, one gather launch a strip),
against the oracle.

Reference: initializeAliveCells (gol/distributor.go:212-220) sends one
CellFlipped per changed cell, row-major over the whole board, every turn.  The
group's stream must give exactly the oracle's per-turn diff lists in global
coordinates, in turn order, never dropping an entry: a batch that would
overflow the caller's buffer stops at the last turn that fits and leaves
every strip there.
"""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest

from oracle.oracle import COracle, flips_np, step_np, unpack_bits

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")


@pytest.fixture(scope="module")
def coracle():
    return COracle()


def idx_to_xy(idx, W):
    idx = idx.astype(np.int64)
    return np.stack([idx % W, idx // W], axis=1).astype(np.int32)


def board_for(fixtures, coracle, W, H, seed):
    if W == H and f"image_{W}" in fixtures:
        return unpack_bits(fixtures[f"image_{W}"], W)
    return coracle.fill_random(W, H, seed)


def cuts_for(H, n):
    """Row 0 of each of n strips and H: the mirror's split (H i / n)."""
    return [H * i // n for i in range(n + 1)]


@contextmanager
def strips_of(board, n, cuts=None):
    """The board on n row strips of device 0."""
    H, W = board.shape
    r = cuts or cuts_for(H, n)
    bs = []
    try:
        for a, b in zip(r[:-1], r[1:]):
            st = golhip.Board(W, H, row0=a, rows=b - a)
            bs.append(st)
            st.load_bytes(board[a:b])
        yield bs, r
    finally:
        for st in bs:
            st.close()


def assert_board(bs, r, want):
    for st, a, b in zip(bs, r[:-1], r[1:]):
        assert np.array_equal(st.snapshot_bytes(), want[a:b]), (a, b)


def oracle_lists(board, turns):
    want, cur = [], board
    for _ in range(turns):
        nxt = step_np(cur)
        want.append(flips_np(cur, nxt))
        cur = nxt
    return want, cur


@pytest.fixture(scope="module")
def oracle_512(fixtures):
    """40 turns of the 512 x 512 fixture: per-turn lists and every board."""
    board = unpack_bits(fixtures["image_512"], 512)
    lists, boards, cur = [], [board], board
    for _ in range(40):
        nxt = step_np(cur)
        lists.append(flips_np(cur, nxt))
        boards.append(nxt)
        cur = nxt
    return lists, boards


@pytest.mark.parametrize("W,H,n", [(512, 512, 3), (64, 64, 2), (1024, 300, 4), (2048, 5, 5), (160, 33, 2),
                                   (48, 48, 3), (16, 16, 2), (512, 512, 1)])
@pytest.mark.parametrize("fmt", [0, 1])
def test_group_flip_stream_matches_oracle(fixtures, coracle, W, H, n, fmt):
    """Every turn's list in uneven batches, both formats: unequal strips
    (170/171/171), one-row strips (every input row a halo), Ww % 4 != 0,
    generic widths (48, 16), and one whole-torus handle (= Board.flip_stream)."""
    board = board_for(fixtures, coracle, W, H, 0x5EED0090 + W)
    cur, t, total = board, 0, 0
    with strips_of(board, n) as (bs, r):
        if (W, H, n) == (512, 512, 3):
            assert [b - a for a, b in zip(r[:-1], r[1:])] == [170, 171, 171]
        single = golhip.Board(W, H) if n == 1 else None
        if single:
            single.load_bytes(board)
        for k in (1, 5, 17, 3):
            ent, counts, done = golhip.group_flip_stream(bs, k, cap=k * W * H, fmt=fmt)
            assert done == k and len(counts) == k and int(counts.sum()) == len(ent)
            if single:
                ent1, counts1, done1 = single.flip_stream(k, cap=k * W * H, fmt=fmt)
                assert done1 == done and np.array_equal(counts1, counts) and np.array_equal(ent1, ent)
            xy = ent if fmt == 0 else idx_to_xy(ent, W)
            off = 0
            for c in counts:
                nxt = step_np(cur)
                assert np.array_equal(xy[off:off + int(c)], flips_np(cur, nxt)), t
                cur, off, t = nxt, off + int(c), t + 1
            total += len(ent)
        if single:
            single.close()
        assert_board(bs, r, cur)
        got = [st.alive_count() for st in bs]
        assert sum(c for c, _ in got) == int((cur == 255).sum()) and all(at == t for _, at in got)
        if W % 32 == 0:
            perf = [st.perf() for st in bs]
            assert all(p["flip_launches"] == t for p in perf), perf
            assert sum(p["flip_entries"] for p in perf) == total
        golhip.group_step(bs, 7)  # the per-launch kernels continue from the stream's boards
        assert_board(bs, r, coracle.run(cur, 7))


def test_group_flip_stream_sparse_strips():
    """One glider in the top strip of 4 on an empty 512 x 512 board: most
    (turn, strip) segments are empty, and the glider crosses into the second
    strip within 40 turns."""
    W = H = 512
    board = np.zeros((H, W), dtype=np.uint8)
    for x, y in ((1, 0), (2, 1), (0, 2), (1, 2), (2, 2)):  # heads down and right, one row in 4 turns
        board[117 + y, 200 + x] = 255
    want, last = oracle_lists(board, 40)
    assert (last[:128] == 255).any() and (last[128:256] == 255).any()  # it straddles the boundary now
    with strips_of(board, 4) as (bs, r):
        ent, counts, done = golhip.group_flip_stream(bs, 40, cap=40 * 64, fmt=golhip.FLIPS_XY)
        assert done == 40
        off = 0
        for t, c in enumerate(counts):
            assert np.array_equal(ent[off:off + int(c)], want[t]), t
            off += int(c)
        assert_board(bs, r, last)
        perf = [st.perf() for st in bs]
        assert perf[2]["flip_entries"] == perf[3]["flip_entries"] == 0 and perf[1]["flip_entries"] > 0


@pytest.mark.parametrize("W,H,fmt", [(512, 512, 0), (48, 48, 1)])
def test_group_flip_stream_stops_without_loss(fixtures, coracle, W, H, fmt):
    """A small buffer: each call runs the turns that fit, the rest follow in
    the next calls; the concatenation equals the oracle's stream and after
    every call all three strips stand at the same turn of the oracle's board."""
    board = board_for(fixtures, coracle, W, H, 0x5EED0091)
    want, _ = oracle_lists(board, 40)
    cap = max(len(w) for w in want) * 3  # about three turns per call
    got, turns, calls = [], 0, 0
    with strips_of(board, 3) as (bs, r):
        while turns < 40:
            ent, counts, done = golhip.group_flip_stream(bs, 40 - turns, cap=cap, fmt=fmt)
            assert 1 <= done <= 40 - turns and len(ent) <= cap
            xy = ent if fmt == 0 else idx_to_xy(ent, W)
            off = 0
            for c in counts:
                got.append(xy[off:off + int(c)].copy())
                off += int(c)
            turns += done
            calls += 1
            assert [st.turn() for st in bs] == [turns] * 3
            assert_board(bs, r, coracle.run(board, turns))
        assert calls > 5
    assert len(got) == 40
    for t in range(40):
        assert np.array_equal(got[t], want[t]), t


@pytest.mark.parametrize("shift", [0, 1, 3, 33])
@pytest.mark.parametrize("fmt", [0, 1])
def test_group_flip_stream_into_pinned_buffer(oracle_512, fmt, shift):
    """out inside a golhip_host_alloc buffer: the gather kernels write the
    entries over the host link themselves.  `shift` entries into the buffer
    the INDEX destination is not 16-byte aligned (1, 3), and the segment
    boundaries inside the batch are misaligned in any case."""
    W = H = 512
    want, boards = oracle_512
    cap = max(len(w) for w in want[:30]) * 4
    buf = golhip.host_array((cap + shift, 2) if fmt == 0 else (cap + shift,), np.int32 if fmt == 0 else np.uint32)
    out = buf[shift:]
    got = []
    with strips_of(boards[0], 3) as (bs, r):
        while len(got) < 30:
            ent, counts, done = golhip.group_flip_stream(bs, 30 - len(got), cap=cap, fmt=fmt, out=out)
            assert done >= 1
            xy = ent if fmt == 0 else idx_to_xy(ent, W)
            off = 0
            for c in counts:
                got.append(xy[off:off + int(c)].copy())
                off += int(c)
        assert_board(bs, r, boards[30])
    for t in range(30):
        assert np.array_equal(got[t], want[t]), t
    del out, buf


@pytest.mark.parametrize("W,H", [(512, 512), (48, 48)])
def test_group_flip_stream_first_turn_too_big(fixtures, coracle, W, H):
    """cap 1: ERANGE, *n_entries = what the first turn needs, no strip advanced."""
    board = board_for(fixtures, coracle, W, H, 0x5EED0092)
    need = len(flips_np(board, step_np(board)))
    with strips_of(board, 3) as (bs, r):
        arr = (ctypes.c_void_p * 3)(*[st.handle for st in bs])
        out = np.zeros(2, dtype=np.int32)
        counts = np.zeros(4, dtype=np.uint64)
        done, n = ctypes.c_int64(-1), ctypes.c_uint64(0)
        rc = golhip.load().golhip_group_flip_stream(arr, 3, 4, golhip.FLIPS_XY, out.ctypes.data_as(ctypes.c_void_p), 1,
                                                    counts.ctypes.data_as(ctypes.c_void_p), ctypes.byref(done),
                                                    ctypes.byref(n))
        assert rc == golhip.GOLHIP_ERANGE and done.value == 0 and n.value == need
        assert [st.turn() for st in bs] == [0, 0, 0]
        assert_board(bs, r, board)
        ent, counts, done = golhip.group_flip_stream(bs, 1, cap=need)
        assert done == 1 and len(ent) == need
        assert_board(bs, r, step_np(board))


def test_group_flip_stream_refusals(coracle):
    """EINVAL: strips at different turns, a gap in the group, a bad format."""
    W, H = 64, 64
    board = coracle.fill_random(W, H, 0x5EED0093)
    with strips_of(board, 2) as (bs, r):
        for fmt in (2, -1):
            with pytest.raises(golhip.GolHipError) as e:
                golhip.group_flip_stream(bs, 1, cap=W * H, fmt=fmt, out=np.empty(W * H, dtype=np.uint32))
            assert e.value.code == golhip.GOLHIP_EINVAL
        assert [st.turn() for st in bs] == [0, 0]
    with strips_of(board, 3, cuts=[0, 20, 40, 64]) as (bs, r):
        with pytest.raises(golhip.GolHipError) as e:
            golhip.group_flip_stream([bs[0], bs[2]], 1, cap=W * H)  # rows 20..39 missing
        assert e.value.code == golhip.GOLHIP_EINVAL
    with strips_of(board, 2) as (bs, r):
        golhip.group_step(bs, 1)
        # strip 0 back at turn 0, strip 1 at turn 1
        with golhip.Board(W, H, row0=0, rows=r[1]) as fresh:
            fresh.load_bytes(board[:r[1]])
            with pytest.raises(golhip.GolHipError) as e:
                golhip.group_flip_stream([fresh, bs[1]], 1, cap=W * H)
            assert e.value.code == golhip.GOLHIP_EINVAL
            assert fresh.turn() == 0 and bs[1].turn() == 1
