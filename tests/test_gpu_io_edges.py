"""GPU side channels at their size edges: libgolhip.so against numpy and the C oracle.

Every other GPU test measures through load_bytes / load_bits / snapshot_* /
alive_cells / flips at whatever size its step test happens to use.  Here the
side channels themselves are the subject, at the sizes where their code takes
another branch:
  A  K3 compaction past 1024 blocks (compact_scan_kernel: more than one entry
     per scan thread, trailing threads with none);
  B  byte I/O past one staging chunk (stage_rows(), golhip_handle.cpp);
  C  load_bits with set bits in the columns >= width (ignored: golhip.h);
  D  snapshot_rows on every row range, 8-byte-aligned ones included;
  E  the flip list's validity rules and fully alive boards.
Bar: exact equality, no case sampled.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle.oracle import COracle, alive_cells_np, flips_np, pack_bits, step_np, unpack_bits

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        _ORACLE = COracle()
    return _ORACLE


def frozen(*arrays):
    """Shared references stay as computed."""
    for a in arrays:
        a.flags.writeable = False
    return arrays


def assert_no_flip_list(b):
    with pytest.raises(golhip.GolHipError) as e:
        b.flips()
    assert e.value.code == golhip.GOLHIP_EINVAL


def random_board(W, H, seed, density=0.35):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((H, W)) < density, 255, 0).astype(np.uint8)


# ---------------------------------------------------------------- A: K3 past 1024 blocks
SCAN_THREADS = 1024  # compact_scan_kernel: one block of 1024 threads
K3_SHAPES = [(8192, 4100, (1025, 2, 513)), (8192, 8192, (2048, 2, 1024)), (8192, 8200, (2050, 3, 684))]


def k3_geometry(W, H):
    """(words a block, blocks, entries a scan thread, scan threads with work)
    as compact_blocks() and compact_scan_kernel compute them."""
    info = dict(kv.split("=", 1) for kv in golhip.load().golhip_build_info().decode().split())
    blk = 256 * int(info["GOL_COMPACT_WPT"])
    nblk = -(-(H * (W // 32)) // blk)
    per = -(-nblk // SCAN_THREADS)
    return blk, nblk, per, -(-nblk // per)


@functools.lru_cache(maxsize=1)
def k3_case(W, H):
    """A sparse board in bit words with set bits where the scan's ownership
    changes hands, and its oracle: (words, alive list, next board, flip list)."""
    blk, nblk, per, active = k3_geometry(W, H)
    Ww = W // 32
    nw = H * Ww
    rng = np.random.default_rng(W * 31 + H)
    flat = np.zeros(nw, dtype=np.uint32)
    flat[rng.choice(nw, 20000, replace=False)] = rng.integers(1, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32)
    # whole blocks with no cell next to blocks with many: two fully alive rows across a block boundary
    mid = nblk // 2
    flat[(mid - 4) * blk:(mid + 4) * blk] = 0
    row = mid * blk // Ww
    flat[(row - 1) * Ww:(row + 1) * Ww] = 0xFFFFFFFF
    # the last word of block k and the first of block k + 1 around the blocks where a scan thread's run starts:
    # near thread 0, near the last thread with work, and the last block of all
    ks = {nblk - 1}
    for t in (0, 1, 2, active - 2, active - 1):
        ks.update(k for k in (t * per - 1, t * per) if 0 <= k < nblk)
    for k in sorted(ks):
        flat[min((k + 1) * blk, nw) - 1] |= 0x80000001
        if (k + 1) * blk < nw:
            flat[(k + 1) * blk] |= 0x80000001
    flat[0] |= 0x80000001
    flat[nw - 1] |= 0x80000001
    words = flat.reshape(H, Ww)
    board = unpack_bits(words, W)
    nxt = oracle().run(board, 1)
    return frozen(words, alive_cells_np(board), nxt, flips_np(board, nxt))


@pytest.mark.parametrize("W,H,table", K3_SHAPES)
def test_compaction_past_1024_blocks(W, H, table):
    """alive_cells() and flips() of boards whose per-block counts take more than
    one entry per scan thread (per 2 and 3; the trailing scan threads own
    nothing at 1025 and 2050 blocks).  Asserted geometry at GOL_COMPACT_WPT 4:
    8192 x 4100: 1025 blocks, per 2, 513 threads with work; 8192 x 8192: 2048,
    2, 1024; 8192 x 8200: 2050, 3, 684."""
    blk, nblk, per, active = k3_geometry(W, H)
    assert nblk > SCAN_THREADS and per >= 2, (nblk, per)
    if blk == 1024:
        assert (nblk, per, active) == table
    words, alive, nxt, flips = k3_case(W, H)
    with golhip.Board(W, H) as b:
        b.load_bits(words)
        assert np.array_equal(b.alive_cells(), alive)
        assert b.alive_count() == (len(alive), 0)
        b.step(1, want_flips=True)
        assert np.array_equal(b.flips(), flips)
        assert np.array_equal(b.snapshot_bytes(), nxt)


@pytest.mark.parametrize("wpl", [1, 2, 4])
def test_compaction_past_1024_blocks_layouts(wpl):
    """The alive list of the stepped board in the canonical, pair and quad
    layouts (cword_canon across 2050 blocks)."""
    W, H = 8192, 8200
    assert k3_geometry(W, H)[1] > SCAN_THREADS
    words, _, nxt, _ = k3_case(W, H)
    with golhip.Board(W, H) as b:
        b.set_option("wpl", wpl)
        b.load_bits(words)
        b.step(1)
        assert b.perf()["words_per_lane"] == wpl
        want = alive_cells_np(nxt)
        assert np.array_equal(b.alive_cells(), want)
        assert b.alive_count() == (len(want), 1)


def test_compaction_past_1024_blocks_strip():
    """A strip handle with row0 > 0: the same list with global y."""
    W, H = 8192, 8200
    assert k3_geometry(W, H)[1] > SCAN_THREADS
    words, alive, _, _ = k3_case(W, H)
    with golhip.Board(W, 2 * H, row0=H, rows=H) as b:
        b.load_bits(words)
        assert np.array_equal(b.alive_cells(), alive + np.array([0, H], dtype=np.int32))
        assert b.alive_count() == (len(alive), 0)


# ---------------------------------------------------------------- B: chunked byte I/O
STAGE_BYTES = 64 << 20  # kStageBytes at stage_rows(), golhip_handle.cpp


@functools.lru_cache(maxsize=1)
def byte_case(W, H, turns):
    """(bytes as loaded, the board they mean, its bit words, the board after `turns`)."""
    rng = np.random.default_rng(W + 3 * H)
    raw = np.where(rng.integers(0, 256, (H, W), dtype=np.uint8) < 77, 255, 0).astype(np.uint8)  # density 0.3
    for r in (0, H // 2, H - 2, H - 1):  # other byte values are dead cells: in the first chunk and in the last
        cols = rng.choice(W, 96, replace=False)
        raw[r, cols] = np.tile(np.array([1, 128, 254], dtype=np.uint8), 32)
    clean = np.where(raw == 255, 255, 0).astype(np.uint8)
    return frozen(raw, clean, pack_bits(clean), oracle().run(clean, turns))


@pytest.mark.parametrize("W,H,wpl,turns", [(8192, 8193, 0, 2), (8192, 8193, 1, 2), (8192, 8193, 2, 2),
                                           (8192, 8193, 4, 2), (262144, 257, 0, 2), (8200, 8185, 0, 1)])
def test_chunked_byte_io(W, H, wpl, turns):
    """load_bytes / snapshot_bytes of boards of more than 64 MiB: two staging
    chunks, the second of one row (8192 + 1, 256 + 1 and 8184 + 1 rows).
    8192 wide packs by 16-byte vectors, in every layout; 262144 wide runs in
    the layout the engine picks; 8200 wide (W % 32 == 8) takes the scalar pack
    path and the generic step kernel."""
    per = max(1, STAGE_BYTES // W)
    assert W * H > STAGE_BYTES and -(-H // per) == 2 and H - per == 1
    raw, clean, bits, want = byte_case(W, H, turns)
    with golhip.Board(W, H) as b:
        b.set_option("wpl", wpl)
        b.load_bytes(raw)
        if wpl:
            assert b.perf()["words_per_lane"] == wpl
        assert np.array_equal(b.snapshot_bytes(), clean)
        assert np.array_equal(b.snapshot_bits(), bits)
        assert b.alive_count() == (int(np.count_nonzero(clean)), 0)
        assert b.board_hash() == golhip.board_hash_np(bits)
        b.step(turns)
        assert np.array_equal(b.snapshot_bytes(), want)


# ---------------------------------------------------------------- C: load_bits ignores columns >= width
PAD_SHAPES = [(100, 7), (33, 64), (1, 1), (17, 9), (48, 20), (8200, 5)]


def dirty_bits(board, garbage):
    """pack_bits(board) with bits set in the columns >= width of each row's last word."""
    H, W = board.shape
    rng = np.random.default_rng(W * 1000 + H)
    pad = np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
    words = pack_bits(board)
    junk = np.full(H, pad) if garbage == "all" else rng.integers(0, 1 << 32, H, dtype=np.uint64).astype(np.uint32) & pad
    if garbage == "random":
        junk[0] |= np.uint32(1 << (W % 32))  # (at least the first padding bit of row 0)
    words[:, -1] |= junk
    assert not np.array_equal(words, pack_bits(board))
    return words


def oracle_lists(board, turns):
    lists, cur = [], board
    for _ in range(turns):
        nxt = step_np(cur)
        lists.append(flips_np(cur, nxt))
        cur = nxt
    return lists, cur


@pytest.mark.parametrize("W,H", PAD_SHAPES)
@pytest.mark.parametrize("garbage", ["all", "random"])
def test_load_bits_ignores_padding(W, H, garbage):
    """Bits of columns >= width in a row's last word are no cells: count, list,
    digest, snapshots and the first turn's flips equal the clean board's."""
    board = random_board(W, H, W + 100 * H)
    clean = pack_bits(board)
    with golhip.Board(W, H) as b:
        b.load_bits(dirty_bits(board, garbage))
        assert b.alive_count() == (int(np.count_nonzero(board)), 0)
        assert np.array_equal(b.alive_cells(), alive_cells_np(board))
        assert b.board_hash() == golhip.board_hash_np(clean)
        assert np.array_equal(b.snapshot_bits(), clean)
        assert np.array_equal(b.snapshot_bytes(), board)
        lists, last = oracle_lists(board, 4)
        b.step(1, want_flips=True)
        assert np.array_equal(b.flips(), lists[0])
        xy, counts = b.step_flips(3, cap=3 * W * H)
        assert [int(c) for c in counts] == [len(x) for x in lists[1:]]
        assert np.array_equal(xy, np.concatenate(lists[1:]))
        assert np.array_equal(b.snapshot_bits(), pack_bits(last))


@pytest.mark.parametrize("W,H", [s for s in PAD_SHAPES if s[1] >= 2])  # (two strips need two rows)
@pytest.mark.parametrize("garbage", ["all", "random"])
def test_load_bits_ignores_padding_strips(W, H, garbage):
    """The same on two row strips stepped as a group."""
    board = random_board(W, H, W + 100 * H)
    clean = pack_bits(board)
    dirty = dirty_bits(board, garbage)
    cuts = [0, H // 2, H]
    strips = []
    try:
        for a, e in zip(cuts[:-1], cuts[1:]):
            s = golhip.Board(W, H, row0=a, rows=e - a)
            s.load_bits(dirty[a:e])
            strips.append(s)
        assert [s.alive_count() for s in strips] == [(int(np.count_nonzero(board[a:e])), 0)
                                                     for a, e in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate([s.alive_cells() for s in strips]), alive_cells_np(board))
        assert sum(s.board_hash() for s in strips) % (1 << 64) == golhip.board_hash_np(clean)
        assert np.array_equal(np.concatenate([s.snapshot_bits() for s in strips]), clean)
        assert np.array_equal(np.concatenate([s.snapshot_bytes() for s in strips]), board)
        lists, last = oracle_lists(board, 4)
        golhip.group_step(strips, 1, want_flips=True)
        assert np.array_equal(np.concatenate([s.flips() for s in strips]), lists[0])
        xy, counts, done = golhip.group_flip_stream(strips, 3, cap=3 * W * H)
        assert done == 3 and [int(c) for c in counts] == [len(x) for x in lists[1:]]
        assert np.array_equal(xy, np.concatenate(lists[1:]))
        assert np.array_equal(np.concatenate([s.snapshot_bits() for s in strips]), pack_bits(last))
    finally:
        for s in strips:
            s.close()


# ---------------------------------------------------------------- D: snapshot_rows on any row range
@pytest.mark.parametrize("W,H,wpl,lanes", [(320, 33, 1, 1), (320, 33, 2, 2), (640, 9, 2, 2), (1024, 12, 1, 1),
                                           (1024, 12, 2, 2), (1024, 12, 4, 4)])
def test_snapshot_rows_every_range(W, H, wpl, lanes):
    """Every row range of a board stepped in its layout.  320 wide has 10 words
    a row, so in the pair layout an odd first row starts 8 bytes off a 16-byte
    boundary and odd row counts end in half a quad.  The board is unchanged
    afterwards (each call converts the range to canonical words and back)."""
    board = oracle().fill_random(W, H, 0x5EED00D0 + W)
    want5, want10 = oracle().run(board, 5), oracle().run(board, 10)
    bits = pack_bits(want5)
    with golhip.Board(W, H) as b:
        b.set_option("wpl", wpl)
        b.load_bytes(board)
        b.step(5)
        assert b.perf()["words_per_lane"] == lanes
        digest = b.board_hash()
        assert digest == golhip.board_hash_np(bits)
        ranges = [(r, n) for r in range(H) for n in range(1, H - r + 1)]
        assert len(ranges) == H * (H + 1) // 2
        for r, n in ranges:
            assert np.array_equal(b.snapshot_rows(r, n), bits[r:r + n]), (r, n)
        assert b.board_hash() == digest
        assert np.array_equal(b.snapshot_bytes(), want5)
        for r in (0, H // 2, H):
            assert b.snapshot_rows(r, 0).shape == (0, W // 32)
        out = np.zeros((H + 2, W // 32), dtype=np.uint32)
        for r, n in [(-1, 1), (0, -1), (H, 1), (0, H + 1), (H - 1, 2), (2**31 - 1, 1)]:
            rc = golhip.load().golhip_snapshot_rows(b.handle, r, n, out.ctypes.data_as(ctypes.c_void_p))
            assert rc == golhip.GOLHIP_EINVAL, (r, n)
        assert not out.any()
        b.step(5)
        assert np.array_equal(b.snapshot_bytes(), want10)


# ---------------------------------------------------------------- E: the flip list's contract
@pytest.mark.parametrize("W,H,wpl", [(64, 64, 0), (100, 37, 0), (64, 64, 2)])
def test_flip_list_validity(W, H, wpl):
    """A flip list belongs to the turn that made it: a later step retires it,
    the read-only side channels do not -- nor does alive_cells(), which reuses
    the block counts: flips() then counts again and still gives the turn's list."""
    board = random_board(W, H, 7 * W + H)
    boards = [board]
    for _ in range(6):
        boards.append(step_np(boards[-1]))
    lists = [flips_np(a, c) for a, c in zip(boards[:-1], boards[1:])]
    with golhip.Board(W, H) as b:
        b.set_option("wpl", wpl)
        b.load_bytes(board)
        assert_no_flip_list(b)
        b.step(1, want_flips=True)
        assert np.array_equal(b.flips(), lists[0])
        b.step(1)
        assert_no_flip_list(b)  # never the list of turn 1 at turn 2
        b.step(1, want_flips=True)
        assert np.array_equal(b.alive_cells(), alive_cells_np(boards[3]))
        assert np.array_equal(b.flips(), lists[2])  # not a list scanned for another input: the turn's own
        b.step(3, want_flips=True)
        assert np.array_equal(b.snapshot_bits(), pack_bits(boards[6]))
        assert np.array_equal(b.snapshot_rows(H // 3, H // 2), pack_bits(boards[6])[H // 3:H // 3 + H // 2])
        assert b.board_hash() == golhip.board_hash_np(pack_bits(boards[6]))
        assert b.alive_count() == (int(np.count_nonzero(boards[6])), 6)
        assert np.array_equal(b.snapshot_bytes(), boards[6])
        assert np.array_equal(b.flips(), lists[5])
        assert np.array_equal(b.flips(), lists[5])  # and again: reading it does not consume it


@pytest.mark.parametrize("W,H", [(96, 40), (100, 37)])
def test_fully_alive_board(W, H):
    """Every cell alive: the alive list is all W * H cells in row-major order;
    one turn later every cell has died of eight neighbours and flipped."""
    every = np.stack([np.tile(np.arange(W), H), np.repeat(np.arange(H), W)], axis=1).astype(np.int32)
    with golhip.Board(W, H) as b:
        b.load_bytes(np.full((H, W), 255, dtype=np.uint8))
        assert b.alive_count() == (W * H, 0)
        assert np.array_equal(b.alive_cells(), every)
        b.step(1, want_flips=True)
        assert np.array_equal(b.flips(), every)
        assert b.alive_count() == (0, 1)
        assert len(b.alive_cells()) == 0
        assert not b.snapshot_bytes().any()
