"""Checkpoints on the device (golhip_checkpoint_begin / _wait / _load, K8;
DESIGN.md §5.16): the file is the board of the turn `begin` was called at,
whatever layout, strips or chunk size held it, and a load brings back that
board, at that turn, verified.

Shapes (W x H): 32x3 one word a lane; 64x5, 256x33 pairs; 128x4, 256x9 quads;
16x16, 40x7 the generic kernel (40: padding bits).  Heights are odd or small
so that the 16-byte groups of the kernels end in a tail.
"""
import functools
import os

import numpy as np
import pytest

from oracle.oracle import fill_random_np, pack_bits, run_np, unpack_bits

pytestmark = pytest.mark.gpu
golhip = pytest.importorskip("golhip")

SEED = 0xC0FFEE
# (W, H, wpl the board is stepped with, wpl of the board the file is loaded into)
SHAPES = [(32, 3, 0, 0), (64, 5, 2, 1), (256, 33, 2, 4), (128, 4, 4, 2), (256, 9, 4, 1), (16, 16, 0, 0), (40, 7, 0, 0)]


@functools.lru_cache(maxsize=None)
def ref(W, H, turns):
    """fill_random(SEED) after `turns` turns (0/255 bytes); computed once, shared read-only."""
    b = run_np(fill_random_np(W, H, SEED), turns)
    b.setflags(write=False)
    return b


def board(W, H, wpl=0, **kw):
    b = golhip.Board(W, H, **kw)
    if wpl:
        b.set_option("wpl", wpl)
    return b


def stepped(W, H, wpl, turns=7):
    b = board(W, H, wpl)
    b.fill_random(SEED)
    b.step(turns)
    return b


@pytest.mark.parametrize("W,H,wpl,wpl2", SHAPES)
def test_round_trip(tmp_path, W, H, wpl, wpl2):
    path = str(tmp_path / "a.ckpt")
    with stepped(W, H, wpl) as b:
        info = golhip.checkpoint_begin(b, path).wait()
        bits, count, digest = b.snapshot_bits(), b.alive_count()[0], b.board_hash()
    assert not os.path.exists(path + ".tmp")
    finfo, words = golhip.checkpoint_read_np(path)
    assert np.array_equal(words, bits)
    assert np.array_equal(unpack_bits(words, W), ref(W, H, 7))
    assert finfo["turn"] == 7 and finfo["alive"] == count
    assert finfo["hash"] == digest == golhip.board_hash_np(words)
    assert {k: info[k] for k in finfo} == finfo == golhip.checkpoint_info(path)
    assert info["stall_ms"] > 0 and info["drain_ms"] > 0 and info["write_ms"] > 0
    # a file written by numpy alone is the same file
    path2 = str(tmp_path / "np.ckpt")
    golhip.checkpoint_write_np(path2, pack_bits(ref(W, H, 7)), W, H, 7)
    assert open(path2, "rb").read() == open(path, "rb").read()
    for p in (path, path2):
        with board(W, H, wpl2) as c:
            assert golhip.checkpoint_load(c, p) == finfo
            assert c.turn() == 7 and c.board_hash() == digest and c.alive_count() == (count, 7)
            c.step(5)
            assert c.turn() == 12
            assert np.array_equal(c.snapshot_bytes(), ref(W, H, 12))


@pytest.mark.parametrize("source", ["image_16", "image_64"])
def test_round_trip_fixture_image(tmp_path, fixtures, source):
    W = int(source.split("_")[1])
    start = unpack_bits(fixtures[source], W)
    path = str(tmp_path / "img.ckpt")
    with golhip.Board(W, W) as b:
        b.load_bytes(start)
        b.step(7)
        golhip.checkpoint_begin(b, path).wait()
    at7 = run_np(start, 7)
    info, words = golhip.checkpoint_read_np(path)
    assert info["turn"] == 7 and np.array_equal(unpack_bits(words, W), at7)
    with golhip.Board(W, W) as c:
        golhip.checkpoint_load(c, path)
        c.step(5)
        assert c.turn() == 12 and np.array_equal(c.snapshot_bytes(), run_np(at7, 5))


def test_chunk_edges(tmp_path):
    W, H = 64, 7
    files, hashes = [], []
    with stepped(W, H, 2) as b:
        for chunk in (1, 3, 7, 64):
            p = str(tmp_path / f"c{chunk}.ckpt")
            golhip.checkpoint_begin(b, p, chunk_rows=chunk).wait()
            files.append(open(p, "rb").read())
        want = b.board_hash()
    assert all(f == files[0] for f in files)
    assert np.array_equal(unpack_bits(golhip.checkpoint_read_np(str(tmp_path / "c1.ckpt"))[1], W), ref(W, H, 7))
    for chunk in (1, 3, 7, 64):
        with board(W, H, 1) as c:
            golhip.checkpoint_load(c, str(tmp_path / "c3.ckpt"), chunk_rows=chunk)
            hashes.append(c.board_hash())
    assert hashes == [want] * 4
    with board(W, H) as c, pytest.raises(golhip.GolHipError) as e:
        golhip.checkpoint_load(c, str(tmp_path / "c3.ckpt"), chunk_rows=-1)
    assert e.value.code == golhip.GOLHIP_EINVAL


def test_consistent_while_stepping(tmp_path):
    W, H = 256, 64
    path = str(tmp_path / "s.ckpt")
    with stepped(W, H, 2) as b:
        ck = golhip.checkpoint_begin(b, path)
        b.step(50)  # enqueued behind the checkpoint kernel; both board buffers are overwritten
        info = ck.wait()
        assert info["turn"] == 7
        assert np.array_equal(unpack_bits(golhip.checkpoint_read_np(path)[1], W), ref(W, H, 7))
        assert b.turn() == 57 and np.array_equal(b.snapshot_bytes(), ref(W, H, 57))


def strips(W, H, cuts, wpl=0):
    bs = []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        bs.append(board(W, H, wpl, row0=r0, rows=r1 - r0))
    return bs


@pytest.mark.parametrize("W,H,cuts,wpl", [(64, 23, (0, 8, 16, 23), 0), (128, 10, (0, 3, 6, 10), 4)])
def test_strips(tmp_path, W, H, cuts, wpl):
    pg, pw = str(tmp_path / "group.ckpt"), str(tmp_path / "whole.ckpt")
    bs = strips(W, H, cuts, wpl)
    for b in bs:
        b.fill_random(SEED)
    golhip.group_step(bs, 7)
    golhip.checkpoint_begin(bs, pg, chunk_rows=3).wait()
    for b in bs:
        b.close()
    with stepped(W, H, wpl) as b:
        golhip.checkpoint_begin(b, pw).wait()
    assert open(pg, "rb").read() == open(pw, "rb").read()
    for n in (1, 2, 4):
        cs = strips(W, H, tuple(H * i // n for i in range(n + 1)), wpl) if n > 1 else [board(W, H, wpl)]
        assert golhip.checkpoint_load(cs, pg, chunk_rows=2)["turn"] == 7
        assert [c.turn() for c in cs] == [7] * n
        golhip.group_step(cs, 9)
        got = np.concatenate([c.snapshot_bits() for c in cs])
        assert np.array_equal(unpack_bits(got, W), ref(W, H, 16)), n
        for c in cs:
            c.close()


def test_begin_refuses_a_group_that_is_not_one_board_at_one_turn(tmp_path):
    W, H = 64, 16
    bs = strips(W, H, (0, 8, 16))
    for b in bs:
        b.fill_random(SEED)
    golhip.group_step(bs, 2)
    bs[1].fill_random(SEED)  # back at turn 0, its neighbour at 2
    with pytest.raises(golhip.GolHipError) as e:
        golhip.checkpoint_begin(bs, str(tmp_path / "no.ckpt"))
    assert e.value.code == golhip.GOLHIP_EINVAL and "turn" in str(e.value)
    with pytest.raises(golhip.GolHipError) as e:  # a strip alone does not cover the board
        golhip.checkpoint_begin(bs[0], str(tmp_path / "no.ckpt"))
    assert e.value.code == golhip.GOLHIP_EINVAL
    assert os.listdir(tmp_path) == []
    for b in bs:
        b.close()


def _write(tmp_path, W, H, turn, name="w.ckpt"):
    p = str(tmp_path / name)
    golhip.checkpoint_write_np(p, pack_bits(ref(W, H, turn)), W, H, turn)
    return p


def test_damage(tmp_path):
    # one payload bit flipped
    p = _write(tmp_path, 64, 5, 7)
    data = bytearray(open(p, "rb").read())
    data[64 + 13] ^= 0x10
    open(p, "wb").write(bytes(data))
    with board(64, 5) as c:
        with pytest.raises(golhip.GolHipError) as e:
            golhip.checkpoint_load(c, p)
        assert e.value.code == golhip.GOLHIP_ECORRUPT
        assert "digest" in str(e.value) or "count" in str(e.value)
    # a padding bit set (column 40 of row 2), the header made to match the payload as it stands
    W, H = 40, 7
    words = pack_bits(ref(W, H, 7)).copy()
    words[2, 1] |= np.uint32(1 << 8)
    p = str(tmp_path / "pad.ckpt")
    alive = int(np.unpackbits(words.view(np.uint8)).sum())
    with open(p, "wb") as f:
        f.write(golhip.checkpoint_header_np(W, H, 7, alive, golhip.board_hash_np(words)))
        f.write(words.astype("<u4").tobytes())
    assert golhip.checkpoint_info(p)["alive"] == alive  # header and size are sound
    with board(W, H) as c:
        with pytest.raises(golhip.GolHipError) as e:
            golhip.checkpoint_load(c, p)
        assert e.value.code == golhip.GOLHIP_ECORRUPT
    # another board size
    p = _write(tmp_path, 64, 5, 7, "small.ckpt")
    with board(64, 6) as c:
        with pytest.raises(golhip.GolHipError) as e:
            golhip.checkpoint_load(c, p)
        assert e.value.code == golhip.GOLHIP_EINVAL


def test_failed_checkpoint_leaves_board_and_nothing_behind(tmp_path):
    W, H = 64, 5
    path = str(tmp_path / "no_such_dir" / "a.ckpt")
    with stepped(W, H, 2) as b:
        ck = golhip.checkpoint_begin(b, path)
        with pytest.raises(golhip.GolHipError) as e:
            ck.wait()
        assert e.value.code == golhip.GOLHIP_EINVAL and "a.ckpt.tmp" in str(e.value)
        b.step(5)
        assert b.turn() == 12 and np.array_equal(b.snapshot_bytes(), ref(W, H, 12))
    assert not os.path.exists(str(tmp_path / "no_such_dir"))


def test_atomic_replace(tmp_path):
    """A good checkpoint, then a begin on the same path that cannot create its
    .tmp: the earlier file stays byte-identical and nothing is left beside it.
    Two obstacles, both in every run: a directory in the .tmp's place (open
    fails with EISDIR, for the superuser too), then the directory read-only.
    Permissions do not bind the superuser; there the second begin succeeds, and
    must then have replaced the file whole, again with no .tmp left."""
    W, H = 64, 5
    d = tmp_path / "ro"
    d.mkdir()
    path = str(d / "a.ckpt")
    with stepped(W, H, 2) as b:
        golhip.checkpoint_begin(b, path).wait()
        before = open(path, "rb").read()
        assert golhip.checkpoint_info(path)["turn"] == 7
        b.step(3)

        os.mkdir(path + ".tmp")
        ck = golhip.checkpoint_begin(b, path)
        with pytest.raises(golhip.GolHipError) as e:
            ck.wait()
        assert e.value.code == golhip.GOLHIP_EINVAL and "a.ckpt.tmp" in str(e.value)
        assert open(path, "rb").read() == before
        assert sorted(os.listdir(d)) == ["a.ckpt", "a.ckpt.tmp"] and os.listdir(path + ".tmp") == []
        os.rmdir(path + ".tmp")  # (the test's own)

        os.chmod(d, 0o555)
        try:
            ck = golhip.checkpoint_begin(b, path)
            if os.geteuid() != 0:
                with pytest.raises(golhip.GolHipError):
                    ck.wait()
            else:
                assert ck.wait()["turn"] == 10
        finally:
            os.chmod(d, 0o755)
        assert sorted(os.listdir(d)) == ["a.ckpt"]
        if os.geteuid() != 0:
            assert open(path, "rb").read() == before
        else:
            assert np.array_equal(unpack_bits(golhip.checkpoint_read_np(path)[1], W), ref(W, H, 10))
        # the board was not disturbed by either
        b.step(2)
        assert b.turn() == 12 and np.array_equal(b.snapshot_bytes(), ref(W, H, 12))


def test_destroy_before_wait(tmp_path):
    W, H = 256, 33
    path = str(tmp_path / "d.ckpt")
    b = stepped(W, H, 2)
    ck = golhip.checkpoint_begin(b, path, chunk_rows=4)
    b.close()
    info = ck.wait()
    assert info["turn"] == 7 and not os.path.exists(path + ".tmp")
    assert np.array_equal(unpack_bits(golhip.checkpoint_read_np(path)[1], W), ref(W, H, 7))


def test_second_begin_waits_for_the_first_drain(tmp_path):
    W, H = 256, 33
    with stepped(W, H, 4) as b:
        a = golhip.checkpoint_begin(b, str(tmp_path / "1.ckpt"), chunk_rows=1)
        b.step(3)
        c = golhip.checkpoint_begin(b, str(tmp_path / "2.ckpt"), chunk_rows=5)
        assert c.wait()["turn"] == 10 and a.wait()["turn"] == 7
    for name, t in (("1.ckpt", 7), ("2.ckpt", 10)):
        assert np.array_equal(unpack_bits(golhip.checkpoint_read_np(str(tmp_path / name))[1], W), ref(W, H, t))
