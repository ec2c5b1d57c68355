"""Padded strips on the GPU (golhip_group_set_pad_step): a
board whose width is no multiple of 32, held as row strips and stepped by
golhip_group_step[_ex], on the fast per-launch kernels as wide strips with
ghost columns, against the per-cell oracle.

Every case runs with mode 1 (always) unless it says otherwise; odd widths take
the per-cell oracle, so the cases stay under about 5e7 cell-updates.
"""
import contextlib
import functools

import numpy as np
import pytest

from oracle.oracle import COracle, flips_np, pack_bits, pgm_bytes, read_pgm, step_np

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

SHAPES = [(3, 40), (17, 66), (63, 96), (65, 9), (100, 37), (127, 80), (129, 7), (1000, 300)]
PLANS = [(1, 32), (1, 16), (2, 18), (2, 20)]  # (words per lane, tb_depth)
PERF_KEYS = ("step_launches", "step_turns", "pad_launches", "skew_launches", "pair_launches", "kernel_variant",
             "halo_bytes")


@functools.lru_cache(maxsize=None)
def oracle():
    return COracle()


def soup(W, H, seed, p=0.35):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((H, W)) < p, 255, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def truth(W, H, seed, turns):
    """The oracle's board after `turns` turns (computed once, never written)."""
    out = oracle().run_exact(soup(W, H, seed), turns)
    out.setflags(write=False)
    return out


def alive(board):
    return int(np.count_nonzero(board == 255))


def cuts_of(H):
    """One strip; two strips; three uneven strips; three strips whose first has
    one row (the group's launch depth is capped by its shortest strip: 1)."""
    cs = [[0, H], [0, H // 2, H], [0, H // 4 + 1, H // 4 + 1 + H // 3 + 1, H], [0, 1, 1 + (H - 1) // 2, H]]
    return [c for c in cs if all(b > a for a, b in zip(c[:-1], c[1:]))]


@contextlib.contextmanager
def strips_of(W, H, cuts, board=None, mode=1, **opts):
    """The board on the row strips [cuts[i], cuts[i + 1]) of device 0."""
    bs = []
    try:
        for a, e in zip(cuts[:-1], cuts[1:]):
            st = golhip.Board(W, H, row0=a, rows=e - a)
            bs.append(st)
            for k, v in opts.items():
                if k == "tb_depth":
                    st.set_tb_depth(v)
                else:
                    st.set_option(k, v)
            if board is not None:
                st.load_bytes(board[a:e])
        if mode is not None:
            golhip.group_set_pad_step(bs, mode)
        yield bs
    finally:
        for st in bs:
            st.close()


def check_strips(bs, cuts, want, turns, what):
    """Snapshots, the strips' own counts and the hash sum against the oracle's board."""
    got = np.concatenate([st.snapshot_bytes() for st in bs])
    assert np.array_equal(got, want), what
    for st, a, e in zip(bs, cuts[:-1], cuts[1:]):
        assert st.alive_count() == (alive(want[a:e]), turns), (what, a, e)
        assert st.turn() == turns, what
        assert np.array_equal(st.snapshot_bits(), pack_bits(want[a:e])), (what, a, e)  # (padding bits clear)
    mask = (1 << 64) - 1
    assert sum(st.board_hash() for st in bs) & mask == golhip.board_hash_np(pack_bits(want)), what


# ---------------------------------------------------------------- parity with the oracle
@pytest.mark.parametrize("skew", [0, 2])
@pytest.mark.parametrize("wpl,depth", PLANS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_parity_with_oracle(W, H, wpl, depth, skew):
    """2 depth + 5 turns: the pad pass, exchanges of wide rows, the seam refresh
    over the halo rows and the unpad pass all run.  (63, 96) and (127, 80) are
    the tight widths (ghosts of 33 / 32 cells)."""
    turns = 2 * depth + 5
    board, want = soup(W, H, 1000 * W + H), truth(W, H, 1000 * W + H, turns)
    for cuts in cuts_of(H):
        what = (W, H, wpl, depth, skew, cuts)
        with strips_of(W, H, cuts, board, wpl=wpl, skew=skew, tb_depth=depth) as bs:
            golhip.group_step(bs, turns)
            perf = [st.perf() for st in bs]
            print(what, {k: perf[0][k] for k in PERF_KEYS})
            check_strips(bs, cuts, want, turns, what)
            for p in perf:
                assert p["step_turns"] == turns and p["persist_launches"] == 0, (what, p)
                assert p["pad_launches"] == p["step_launches"] >= -(-turns // depth), (what, p)
                assert p["kernel_variant"] in (1, 3) and (skew or p["skew_launches"] == 0), (what, p)
                assert len(cuts) == 2 or p["halo_bytes"] > 0, (what, p)


# ---------------------------------------------------------------- the refresh reaches the halo rows
# (W, H, cuts, tb_depth, turns, rounds, launches, numpy controls that are wrong)
CONTROLS = [
    (63, 96, [0, 32, 64, 96], 16, 96, [(16, 2)] * 3, 6, ("own",)),
    (63, 96, [0, 32, 64, 96], 32, 96, [(32, 1)] * 3, 3, ("own",)),
    (127, 80, [0, 40, 80], 20, 100, [(20, 2), (20, 2), (20, 1)], 5, ("own", "once")),
]


@pytest.mark.parametrize("W,H,cuts,tb,turns,rounds,launches,wrong", CONTROLS)
def test_refresh_reaches_the_halo_rows(W, H, cuts, tb, turns, rounds, launches, wrong):
    """The controls first: the numpy restatement of the same rounds with the
    refresh kept to the strip's own rows (and, at 127 wide, with one refresh a
    round) is wrong at the end, on a board that is still alive.  So the GPU's
    result shows the seam kernel at work on the rows received in an exchange,
    before every launch."""
    board, want = soup(W, H, 1000 * W + H), truth(W, H, 1000 * W + H, turns)
    assert alive(want) > 0
    assert golhip.group_halo_rounds([b - a for a, b in zip(cuts[:-1], cuts[1:])], tb, turns) == rounds
    for seam in wrong:
        assert not np.array_equal(golhip.pad_group_run_np(board, cuts, turns, rounds, seam), want), seam
    assert np.array_equal(golhip.pad_group_run_np(board, cuts, turns, rounds), want)
    with strips_of(W, H, cuts, board, wpl=1, tb_depth=tb) as bs:
        golhip.group_step(bs, turns)
        check_strips(bs, cuts, want, turns, (W, H, tb))
        for st in bs:
            p = st.perf()
            assert p["pad_launches"] == p["step_launches"] == launches and p["step_turns"] == turns, p
            assert p["halo_bytes"] == 2 * sum(d * k for d, k in rounds) * (golhip.pad_plan_np(W)[0] // 8), p


# ---------------------------------------------------------------- sequences on one group
def test_sequence_on_one_group():
    """Steps, a snapshot between them, a new board, a want_flips step (its last
    turn on K1g from the unpadded strips), the padded path off, then the flip
    stream and a frame across the same strips: the canonical strips are whole
    after every call."""
    W, H, cuts = 100, 37, [0, 10, 25, 37]
    with strips_of(W, H, cuts, soup(W, H, 5)) as bs:
        golhip.group_step(bs, 7)
        assert np.array_equal(np.concatenate([st.snapshot_bytes() for st in bs]), truth(W, H, 5, 7))
        for st in bs:
            p = st.perf()
            assert p["pad_launches"] == p["step_launches"] > 0 and p["step_turns"] == 7, p
        golhip.group_step(bs, 1)
        check_strips(bs, cuts, truth(W, H, 5, 8), 8, "8")
        golhip.group_step(bs, 40)
        check_strips(bs, cuts, truth(W, H, 5, 48), 48, "48")
        for st, a, e in zip(bs, cuts[:-1], cuts[1:]):
            st.load_bytes(soup(W, H, 6)[a:e])
            st.perf_reset()
        assert all(st.turn() == 0 for st in bs)
        golhip.group_step(bs, 33, want_flips=True)
        before, after = truth(W, H, 6, 32), truth(W, H, 6, 33)
        assert np.array_equal(after, step_np(before))
        assert np.array_equal(np.concatenate([st.flips() for st in bs]), flips_np(before, after))
        check_strips(bs, cuts, after, 33, "flips")
        for st in bs:
            p = st.perf()
            # 32 turns on the wide strips, then the last one alone on the any-width kernel
            assert 0 < p["pad_launches"] == p["step_launches"] - 1 and p["step_turns"] == 33, p
            assert p["kernel_variant"] == 0, p
            st.perf_reset()
        golhip.group_set_pad_step(bs, 0)
        golhip.group_step(bs, 5)
        check_strips(bs, cuts, truth(W, H, 6, 38), 38, "mode 0")
        for st in bs:
            p = st.perf()
            assert p["pad_launches"] == 0 and p["step_launches"] == 5 and p["kernel_variant"] == 0, p
        ent, counts, done = golhip.group_flip_stream(bs, 3, cap=3 * W * H)
        assert done == 3 and int(counts.sum()) == len(ent)
        t = 38
        for c in counts:
            got, ent = ent[: int(c)], ent[int(c):]
            assert np.array_equal(got, flips_np(truth(W, H, 6, t), truth(W, H, 6, t + 1))), t
            t += 1
        frame, at = golhip.group_view_frame(bs, fmt=golhip.VIEW_GRAY8)
        assert at == 41 and np.array_equal(frame, truth(W, H, 6, 41))
        check_strips(bs, cuts, truth(W, H, 6, 41), 41, "stream + frame")
        assert all(st.perf()["pad_launches"] == 0 for st in bs)


# ---------------------------------------------------------------- against K1g at a size the oracle cannot reach
def test_large_board_against_generic_kernel():
    W, H, turns = 5001, 4999, 40
    cuts = [0, 1666, 3333, H]
    res = []
    for mode in (0, 1):
        with strips_of(W, H, cuts, mode=mode) as bs:
            for i, st in enumerate(bs):
                st.fill_random(12345 + i)
            golhip.group_step(bs, turns)
            mask = (1 << 64) - 1
            res.append((sum(st.board_hash() for st in bs) & mask, [st.alive_count() for st in bs]))
            for st in bs:
                p = st.perf()
                print(mode, {k: p[k] for k in PERF_KEYS})
                if mode == 0:
                    assert p["step_launches"] == turns and p["pad_launches"] == 0 and p["kernel_variant"] == 0, p
                else:
                    assert p["pad_launches"] == p["step_launches"] <= 3 and p["step_turns"] == turns, p
                    assert p["halo_bytes"] > 0, p
    assert res[0] == res[1], res
    assert all(c > 0 and at == turns for c, at in res[0][1]), res


# ---------------------------------------------------------------- the default rule
# profiles/strip_widths/bench_strip_widths.json: the fewest turns a call from
# which mode 1 beat mode 0 in every repetition at 2, 4 and 8 strips alike is 4
# at 100^2, 8 at 1000^2, 2 at 5000^2 and 1 from 10001^2 on; a board takes the
# row of the largest measured board no larger than it (below 100^2: its row).
# (W, H, strips, turns a call, padded)
RULE = [(100, 100, 2, 4, True), (100, 100, 8, 2, False), (100, 37, 3, 3, False), (1000, 300, 3, 4, True),
        (1000, 1000, 4, 8, True), (1000, 1000, 2, 4, False), (5000, 5000, 4, 2, True), (5000, 5000, 2, 1, False)]


@pytest.mark.parametrize("W,H,k,n,padded", RULE)
def test_default_rule(W, H, k, n, padded):
    cuts = [H * i // k for i in range(k + 1)]
    with strips_of(W, H, cuts, soup(W, H, 3), mode=None) as bs:
        golhip.group_step(bs, n)
        for st in bs:
            p = st.perf()
            assert (p["pad_launches"] > 0) == padded, ((W, H, k, n), p)
            assert p["kernel_variant"] == (0 if not padded else 3 if p["skew_launches"] else 1), ((W, H, k, n), p)
        check_strips(bs, cuts, truth(W, H, 3, n), n, (W, H, k, n))


# ---------------------------------------------------------------- refusals
def test_refusals():
    with strips_of(96, 8, [0, 3, 8], mode=None) as bs:  # a width the fast kernels take as it is
        with pytest.raises(golhip.GolHipError) as e:
            golhip.group_set_pad_step(bs, 1)
        assert e.value.code == golhip.GOLHIP_EINVAL
        golhip.group_set_pad_step(bs, 0)
        golhip.group_set_pad_step(bs, -1)
    with strips_of(100, 37, [0, 10, 25, 37], mode=None) as bs:
        for bad in (-2, 2):
            with pytest.raises(golhip.GolHipError) as e:
                golhip.group_set_pad_step(bs, bad)
            assert e.value.code == golhip.GOLHIP_EINVAL
        for not_a_group in (bs[:2], bs[1:], [bs[1], bs[0], bs[2]]):
            with pytest.raises(golhip.GolHipError) as e:
                golhip.group_set_pad_step(not_a_group, 1)
            assert e.value.code == golhip.GOLHIP_EINVAL
        golhip.group_set_pad_step(bs, 1)
        with pytest.raises(golhip.GolHipError) as e:  # the single handle's switch keeps its contract
            bs[0].set_pad_step(1)
        assert e.value.code == golhip.GOLHIP_EINVAL


# ---------------------------------------------------------------- callers
# A strip's launch is at most as deep as the group's shortest strip (its halo
# rows come from one neighbour), so three strips of a 37-row board cannot run a
# 20-turn batch in one launch: 12 + 8 at strips of 12 / 12 / 13 rows, 6
# refreshes over the three batches.  The 66-row board's strips of 22 rows can:
# 3 refreshes, one per batch.
@pytest.mark.parametrize("H,cuts,launches", [(37, [0, 12, 24, 37], 6), (66, [0, 22, 44, 66], 3)])
def test_group_view_stream_through_the_hook(H, cuts, launches):
    """golhip_group_view_stream's batches step through group_step_locked: three
    batches of 20 turns on the wide strips, frames and final board the oracle's."""
    W = 100
    rounds = golhip.group_halo_rounds([b - a for a, b in zip(cuts[:-1], cuts[1:])], 20, 20)
    assert 3 * sum(k for _, k in rounds) == launches
    with strips_of(W, H, cuts, soup(W, H, 8)) as bs:
        frames, done = golhip.group_view_stream(bs, 60, 20, fmt=golhip.VIEW_GRAY8)
        assert done == 60 and frames.shape == (3, H, W)
        for i, t in enumerate((20, 40, 60)):
            assert np.array_equal(frames[i], truth(W, H, 8, t)), t
        check_strips(bs, cuts, truth(W, H, 8, 60), 60, "view")
        for st in bs:
            p = st.perf()
            assert p["pad_launches"] == p["step_launches"] == launches, p


def test_run_headless_100x100x300_on_three_strips(tmp_path, monkeypatch):
    """gol.Run's 256-turn batches (no cell events) of a 100 x 100 board on three
    strips, under the default rule: the final PGM is the oracle's board."""
    monkeypatch.setenv("GOL_STRIPS", "3")
    board = soup(100, 100, 9)
    (tmp_path / "images").mkdir()
    (tmp_path / "images" / "100x100.pgm").write_bytes(pgm_bytes(board))
    r = golhip.Run(300, 8, 100, 100, str(tmp_path), cell_events=False)
    counts, last, final_alive, _, _ = r.drain()
    assert r.wait() == ""
    r.close()
    want = truth(100, 100, 9, 300)
    assert counts["FinalTurnComplete"] == 1 and last == 300 and final_alive == alive(want)
    assert np.array_equal(read_pgm(str(tmp_path / "out" / "100x100x300.pgm"), 100, 100), want)
