"""The fused turn + CellFlipped list kernel of the Life-like rules (K14,
csrc/gol_rule_flip.hip) behind golhip_set_rule_flips(h, 1): K5's per-launch
machinery with the rule as a policy.  Judged entry for entry by
golhip.life_like_np with oracle.flips_np; perf()["flip_launches"] shows that
the fused kernel did the work and "rule_launches" that the step kernel did not.

Shapes: one per instance (CONTIG, ODD) and edge: one block, two blocks with a
partial second one, block boundaries in mid-row, rows that are their own
neighbours.  B0/S8 raises every padding bit and every lane past the board's
end that the kernel forgets to mask.
"""
import numpy as np
import pytest

from oracle.oracle import flips_np, pack_bits, unpack_bits

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

HIGHLIFE, DAYNIGHT, UNLISTED, B0S8 = "B36/S23", "B3678/S34678", "B3578/S1246", "B0/S8"
STATIC = [HIGHLIFE, DAYNIGHT]
RULES = STATIC + [UNLISTED, B0S8]
EINVAL = -1

# W, H: what the shape covers
SHAPES = [(64, 37),    # Ww 2: strided, one block
          (33, 7),     # ODD, strided
          (128, 37),   # Ww 4: CONTIG
          (100, 9),    # CONTIG + ODD
          (512, 70),   # 1120 words: two blocks, the second partial; wave and row edges inside a block
          (4000, 20),  # ODD, three blocks, block boundaries in mid-row
          (32, 1),     # a row that is its own neighbour above and below
          (64, 2)]     # two rows: the row above is the row below


def start(W, H, seed=0):
    rng = np.random.default_rng(0xF11B + 977 * W + 31 * H + seed)
    b = (rng.random((H, W)) < 0.37).astype(np.uint8) * np.uint8(255)
    b.setflags(write=False)
    return b


_truth = {}


def truth(W, H, rule, turns, seed=0):
    """The model's boards of turns 0..turns and the flip lists (x, y) of turns 1..turns, computed once."""
    key = (W, H, rule, seed)
    if key not in _truth or len(_truth[key][1]) < turns:
        masks = golhip.rule_parse(rule)
        boards, lists = [start(W, H, seed)], []
        for _ in range(turns):
            nxt = golhip.life_like_np(boards[-1], *masks, 1)
            nxt.setflags(write=False)
            lists.append(flips_np(boards[-1], nxt))
            boards.append(nxt)
        _truth[key] = (boards, lists)
    boards, lists = _truth[key]
    return boards[:turns + 1], lists[:turns]


def to_index(xy, W):
    return (xy[:, 1].astype(np.int64) * W + xy[:, 0]).astype(np.uint32)


def cat(lists, W, fmt=golhip.FLIPS_XY):
    xy = np.concatenate(lists) if lists else np.zeros((0, 2), np.int32)
    return xy if fmt == golhip.FLIPS_XY else to_index(xy, W)


def check_board(b, want, turn, what):
    assert np.array_equal(b.snapshot_bytes(), want), what
    assert np.array_equal(b.snapshot_bits(), pack_bits(want)), what  # (padding bits zero)
    assert b.alive_count() == (int((want == 255).sum()), turn), what


class Launches:
    """The launches a sequence of flip-stream calls makes: a
    call launches every turn it was asked for unless it stops at the cap and
    the handle has an estimate, the largest list of its last batch that
    delivered a turn; then the turns the buffer probably holds, plus one."""

    def __init__(self, W, H):
        self.cells, self.est, self.n = W * H, 0, 0

    def call(self, nturns, cap, counts, stop=True):
        dcap = min(cap, nturns * self.cells)
        self.n += min(nturns, dcap // self.est + 1) if stop and self.est > 0 else nturns
        if len(counts) > 0:
            self.est = int(max(counts))


def six_turns(b, W, H, lists, final, what):
    """6 turns split as tests/test_gpu_rules.py::test_flip_streams splits them;
    returns the fused launches the calls should have made."""
    ln = Launches(W, H)
    with pytest.raises(golhip.GolHipError) as e:  # not even the first turn fits
        b.flip_stream(3, len(lists[0]) - 1)
    assert e.value.code == golhip.GOLHIP_ERANGE and b.turn() == 0, what
    ln.call(3, len(lists[0]) - 1, [])
    cap = len(lists[0]) + len(lists[1]) + len(lists[2]) - 1  # stops before the third turn
    ent, counts, done = b.flip_stream(5, cap)
    assert done == 2 and b.turn() == 2 and list(counts) == [len(lists[0]), len(lists[1])], what
    assert np.array_equal(ent, cat(lists[:2], W)), what
    ln.call(5, cap, counts)
    ent, counts, done = b.flip_stream(2, cap, golhip.FLIPS_INDEX)
    assert done == 2 and b.turn() == 4 and list(counts) == [len(lists[2]), len(lists[3])], what
    assert np.array_equal(ent, cat(lists[2:4], W, golhip.FLIPS_INDEX)), what
    ln.call(2, cap, counts)
    xy, counts = b.step_flips(2, W * H * 2)
    assert list(counts) == [len(lists[4]), len(lists[5])] and np.array_equal(xy, cat(lists[4:6], W)), what
    ln.call(2, W * H * 2, counts, stop=False)
    check_board(b, final, 6, what)
    return ln.n


# ---------------------------------------------------------------- every instance shape, every rule
@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes(W, H):
    with golhip.Board(W, H) as b:
        assert b.rule_flips() == 0
        b.set_rule_flips(1)
        assert b.rule_flips() == 1
        for rule in RULES:
            boards, lists = truth(W, H, rule, 6)
            assert all(len(x) for x in lists[:3]), (W, H, rule)  # (the caps below need them)
            b.set_rule(rule)
            b.load_bytes(boards[0])
            b.perf_reset()
            want = six_turns(b, W, H, lists, boards[6], (W, H, rule))
            p = b.perf()
            assert p["flip_launches"] == want and p["rule_launches"] == 0 and p["step_launches"] == 0, (W, H, rule, p)
            assert p["flip_entries"] == sum(len(x) for x in lists), (W, H, rule, p)
            assert p["flip_fallbacks"] == 0 and p["flip_resident_launches"] == 0, (W, H, rule, p)


# ---------------------------------------------------------------- both policies
@pytest.mark.parametrize("W,H", [(64, 37), (100, 9), (512, 70), (4000, 20)])
def test_dynamic_policy_on_the_static_rules(W, H, test_hooks):
    with golhip.Board(W, H) as b:
        b.set_option("rule_kernel", 2)
        b.set_rule_flips(1)
        for rule in STATIC:
            boards, lists = truth(W, H, rule, 6)
            b.set_rule(rule)
            b.load_bytes(boards[0])
            b.perf_reset()
            want = six_turns(b, W, H, lists, boards[6], (W, H, rule, "dynamic"))
            p = b.perf()
            assert p["flip_launches"] == want and p["rule_launches"] == 0, (W, H, rule, p)


# ---------------------------------------------------------------- Conway through both policies
@pytest.mark.parametrize("policy", [1, 2])
def test_conway_through_k14(policy, fixtures, test_hooks):
    """rule_kernel 1 / 2 with mode 1 on the 512 x 512 fixture board: byte-equal
    lists to those of an untouched Conway handle given the same calls."""
    board = unpack_bits(fixtures["image_512"], 512)
    with golhip.Board(512, 512) as plain, golhip.Board(512, 512) as b:
        b.set_option("rule_kernel", policy)
        b.set_rule_flips(1)
        for x in (plain, b):
            x.load_bytes(board)
        first = [x.flip_stream(3, 3 * 512 * 512) for x in (plain, b)]
        second = [x.flip_stream(5, 5 * 512 * 512, golhip.FLIPS_INDEX) for x in (plain, b)]
        for (e0, c0, d0), (e1, c1, d1) in (first, second):
            assert d0 == d1 and np.array_equal(c0, c1) and e0.tobytes() == e1.tobytes()
        assert first[0][2] == 3 and second[0][2] == 5
        assert np.array_equal(b.snapshot_bytes(), plain.snapshot_bytes()) and b.alive_count() == plain.alive_count()
        p, q = b.perf(), plain.perf()
        assert p["flip_launches"] == q["flip_launches"] == 8 and p["rule_launches"] == 0, (p, q)


# ---------------------------------------------------------------- dense blocks
@pytest.mark.parametrize("fmt", [golhip.FLIPS_XY, golhip.FLIPS_INDEX])
def test_dense_blocks(fmt):
    """B012345678/S: every cell flips every turn, 32768 entries a block, past
    the LDS staging (the direct-store form)."""
    W, H, rule = 1024, 33, "B012345678/S"
    with golhip.Board(W, H) as b:
        b.set_rule(rule)
        b.set_rule_flips(1)
        b.load_bytes(np.zeros((H, W), np.uint8))
        ent, counts, done = b.flip_stream(2, 2 * W * H, fmt)
        assert done == 2 and list(counts) == [W * H, W * H]
        ys, xs = np.divmod(np.arange(W * H, dtype=np.int64), W)
        one = np.stack([xs, ys], axis=1).astype(np.int32)
        assert np.array_equal(ent, cat([one, one], W, fmt))
        check_board(b, np.zeros((H, W), np.uint8), 2, fmt)
        assert b.perf()["flip_launches"] == 2


# ---------------------------------------------------------------- pinned output: the copy blocks
@pytest.mark.parametrize("fmt,shift", [(golhip.FLIPS_INDEX, 0), (golhip.FLIPS_INDEX, 1), (golhip.FLIPS_INDEX, 2),
                                       (golhip.FLIPS_INDEX, 3), (golhip.FLIPS_XY, 0), (golhip.FLIPS_XY, 1)])
def test_pinned_output(fmt, shift):
    """512 x 70 into golhip_host_alloc memory, `shift` entries into the buffer:
    destination offsets of 0, 4, 8, 12 bytes (indices) and 0, 8 (pairs)."""
    W, H = 512, 70
    boards, lists = truth(W, H, HIGHLIFE, 6)
    cap = sum(len(x) for x in lists)
    buf = golhip.host_array((cap + shift, 2) if fmt == golhip.FLIPS_XY else (cap + shift,),
                            np.int32 if fmt == golhip.FLIPS_XY else np.uint32)
    out = buf[shift:]
    with golhip.Board(W, H) as b:
        b.set_rule(HIGHLIFE)
        b.set_rule_flips(1)
        b.load_bytes(boards[0])
        ent, counts, done = b.flip_stream(6, cap, fmt, out=out)
        assert done == 6 and list(counts) == [len(x) for x in lists]
        assert np.array_equal(ent, cat(lists, W, fmt))
        check_board(b, boards[6], 6, (fmt, shift))
        p = b.perf()
        assert p["flip_launches"] == 6 and p["flip_resident_launches"] == 0 and p["rule_launches"] == 0, p
    del out, buf


# ---------------------------------------------------------------- forced co-residency fallback
def test_coresidency_fallback(test_hooks):
    W, H = 512, 70
    boards, lists = truth(W, H, UNLISTED, 6)
    with golhip.Board(W, H) as b:
        b.set_rule(UNLISTED)
        b.set_rule_flips(1)
        b.load_bytes(boards[0])
        b.set_option("flip_debug", 4)
        ent, counts, done = b.flip_stream(4, 4 * W * H)
        assert done == 4 and b.perf()["flip_fallbacks"] == 1
        assert np.array_equal(ent, cat(lists[:4], W))
        ent, counts, done = b.flip_stream(2, 2 * W * H)  # ticket order from now on
        assert done == 2 and np.array_equal(ent, cat(lists[4:6], W))
        check_board(b, boards[6], 6, "fallback")
        assert b.perf()["flip_fallbacks"] == 1 and b.perf()["rule_launches"] == 0


# ---------------------------------------------------------------- mode 0 after mode 1
def test_mode_0_after_mode_1():
    W, H = 100, 9
    boards, lists = truth(W, H, DAYNIGHT, 6)
    with golhip.Board(W, H) as b:
        b.set_rule(DAYNIGHT)
        b.set_rule_flips(1)
        b.load_bytes(boards[0])
        ent, counts, done = b.flip_stream(3, 3 * W * H)
        assert done == 3 and np.array_equal(ent, cat(lists[:3], W))
        p1 = b.perf()
        assert p1["flip_launches"] == 3 and p1["rule_launches"] == 0, p1
        kept = b.alive_count()
        b.set_rule_flips(0)  # the board, the turn and the kept count stay
        assert b.rule_flips() == 0 and b.turn() == 3 and b.alive_count() == kept
        ent, counts, done = b.flip_stream(3, 3 * W * H)
        assert done == 3 and np.array_equal(ent, cat(lists[3:6], W))
        p0 = b.perf()
        assert p0["flip_launches"] == 3 and p0["rule_launches"] == 3, p0
        check_board(b, boards[6], 6, "mode 0")


# ---------------------------------------------------------------- the rule changes between batches
def test_set_rule_mid_run():
    W, H = 128, 37
    cur = start(W, H)
    with golhip.Board(W, H) as b:
        b.set_rule_flips(1)
        b.load_bytes(cur)
        turn = 0
        for rule in (HIGHLIFE, UNLISTED, "B3/S23", B0S8, DAYNIGHT):
            b.set_rule(rule)
            assert b.rule_flips() == 1
            masks, want = golhip.rule_parse(rule), []
            for _ in range(2):
                nxt = golhip.life_like_np(cur, *masks, 1)
                want.append(flips_np(cur, nxt))
                cur = nxt
            ent, counts, done = b.flip_stream(2, 2 * W * H)
            turn += 2
            assert done == 2 and list(counts) == [len(x) for x in want], rule
            assert np.array_equal(ent, cat(want, W)), rule
            check_board(b, cur, turn, rule)
        p = b.perf()
        assert p["flip_launches"] == 10 and p["rule_launches"] == 0, p


# ---------------------------------------------------------------- three strips of uneven height
CUTS = [(0, 5), (5, 20), (25, 12)]


@pytest.mark.parametrize("W", [64, 1000])
def test_strips(W):
    H = 37
    boards, lists = truth(W, H, HIGHLIFE, 4)
    bs = [golhip.Board(W, H, row0=r0, rows=n) for r0, n in CUTS]

    def load():
        for b, (r0, n) in zip(bs, CUTS):
            b.load_bytes(np.ascontiguousarray(boards[0][r0:r0 + n]))
            b.perf_reset()

    def run():
        """A cap that stops the batch after two turns, then the rest."""
        cap = len(lists[0]) + len(lists[1]) + len(lists[2]) - 1
        ent, counts, done = golhip.group_flip_stream(bs, 4, cap)
        assert done == 2 and list(counts) == [len(lists[0]), len(lists[1])]
        assert np.array_equal(ent, cat(lists[:2], W))
        assert all(b.turn() == 2 for b in bs)
        ent, counts, done = golhip.group_flip_stream(bs, 2, cap, golhip.FLIPS_INDEX)
        assert done == 2 and np.array_equal(ent, cat(lists[2:4], W, golhip.FLIPS_INDEX))
        assert all(b.turn() == 4 for b in bs)
        assert np.array_equal(np.concatenate([b.snapshot_bytes() for b in bs]), boards[4])
        assert np.array_equal(np.concatenate([b.snapshot_bits() for b in bs]), pack_bits(boards[4]))
        assert sum(b.alive_count()[0] for b in bs) == int((boards[4] == 255).sum())

    try:
        golhip.group_set_rule(bs, HIGHLIFE)
        golhip.group_set_rule_flips(bs, 1)
        assert all(b.rule_flips() == 1 for b in bs)
        load()
        run()
        perf = [b.perf() for b in bs]
        # (the first batch launched 4 turns and stopped at the third: the strips were restored and stepped
        # two turns on the step kernel, so rule_launches moves here, as step_launches does on Conway strips)
        assert all(p["flip_launches"] >= 4 for p in perf), perf
        # one strip left at mode 0: the per-turn path, the same lists
        bs[1].set_rule_flips(0)
        load()
        run()
        perf = [b.perf() for b in bs]
        assert all(p["flip_launches"] == 0 and p["rule_launches"] > 0 for p in perf), perf
    finally:
        for b in bs:
            b.close()


# ---------------------------------------------------------------- refusals
def test_refusals():
    W, H = 64, 37
    boards, lists = truth(W, H, HIGHLIFE, 6)
    with golhip.Board(W, H) as b:
        b.set_rule(HIGHLIFE)
        b.load_bytes(boards[0])
        for mode, bad in ((0, 2), (0, -1), (1, 2), (1, -1)):
            b.set_rule_flips(mode)
            with pytest.raises(golhip.GolHipError) as e:
                b.set_rule_flips(bad)
            assert e.value.code == EINVAL and b.rule_flips() == mode
        ent, counts, done = b.flip_stream(1, W * H)  # still mode 1
        assert done == 1 and np.array_equal(ent, lists[0]) and b.perf()["flip_launches"] == 1
