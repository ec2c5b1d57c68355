"""Life-like rules on the GPU: golhip_set_rule and the rule kernel K11
(csrc/gol_rule.hip), its static and its dynamic policy, judged bit for bit
(board, alive count, golhip_board_hash) by golhip.life_like_np, the numpy
restatement that tests/test_rule_cpu.py pins to the reference's golden boards.

The shapes are the ones at which K11 can go wrong: one word, one tile exactly
(62 words), one word into a second tile, several tiles; fewer rows than a
launch fuses turns (rows that wrap onto the band's own halo); every launch
depth and the turn counts around the cap; widths that are no multiple of 32
on the padded torus and on K11's own one-turn seam; strips of uneven height.
"""
import numpy as np
import pytest

from oracle.oracle import flips_np, pack_bits, unpack_bits

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

CAP = 16  # golk::kRuleMaxDepth: most turns a K11 launch fuses
HIGHLIFE, DAYNIGHT, SEEDS = "B36/S23", "B3678/S34678", "B2/S"
LISTED = [HIGHLIFE, DAYNIGHT, SEEDS]                      # rules with a static instance
RULES = LISTED + ["B0/S8", "B012345678/S", "B3578/S1246"]  # B0, all births, an unlisted rule
RESIDENT_OR_SKEW = ("persist_launches", "skew_launches", "lds_launches", "pair_launches")


def start(W, H, seed=0):
    rng = np.random.default_rng(0xB36 + 977 * W + 31 * H + seed)
    b = (rng.random((H, W)) < 0.37).astype(np.uint8) * np.uint8(255)
    b.setflags(write=False)
    return b


def model(board, rule, turns):
    return golhip.life_like_np(board, *golhip.rule_parse(rule), turns)


def check(b, want, turn, what):
    """Board, alive count and digest of handle b against the model's board."""
    assert np.array_equal(b.snapshot_bytes(), want), what
    assert b.alive_count() == (int((want == 255).sum()), turn), what
    assert b.board_hash() == golhip.board_hash_np(pack_bits(want)), what


def tail_bits_zero(b, W):
    if W % 32:
        last = b.snapshot_bits()[:, -1]
        return not np.any(last >> np.uint32(W % 32))
    return True


# ---------------------------------------------------------------- Conway through K11
@pytest.mark.parametrize("policy", [1, 2])
def test_conway_through_rule_kernel(policy, fixtures, test_hooks):
    """Option "rule_kernel" sends a Conway handle through K11's static (1) and
    dynamic (2) policy: the reference's golden boards judge both."""
    for n in (64, 512):
        board = unpack_bits(fixtures[f"image_{n}"], n)
        golden = unpack_bits(fixtures[f"check_{n}x100"], n)
        with golhip.Board(n, n) as b:
            b.set_option("rule_kernel", policy)
            b.load_bytes(board)
            b.step(100)
            assert np.array_equal(b.snapshot_bytes(), golden), (policy, n)
            assert b.alive_count() == (int(fixtures[f"alive_{n}"][100]), 100)
            p = b.perf()
            assert p["kernel_variant"] == 5 and p["rule_launches"] == p["step_launches"] > 0, p
            assert all(p[k] == 0 for k in RESIDENT_OR_SKEW), p
    W, H = 2016, 67
    board = start(W, H)
    with golhip.Board(W, H) as shipped, golhip.Board(W, H) as b:
        b.set_option("rule_kernel", policy)
        for x in (shipped, b):
            x.load_bytes(board)
            x.step(2 * CAP + 3)
        assert shipped.perf()["rule_launches"] == 0
        assert np.array_equal(b.snapshot_bytes(), shipped.snapshot_bytes())
        assert b.board_hash() == shipped.board_hash() and b.alive_count() == shipped.alive_count()


def test_rule_kernel_option_needs_consent(monkeypatch):
    monkeypatch.delenv("GOLHIP_TEST_HOOKS", raising=False)
    with golhip.Board(64, 64) as b:
        with pytest.raises(golhip.GolHipError, match="GOLHIP_TEST_HOOKS"):
            b.set_option("rule_kernel", 1)
        b.set_option("rule_kernel", 0)


# ---------------------------------------------------------------- shapes x rules x turns
@pytest.mark.parametrize("H", [1, 2, 3, 5, 67])
@pytest.mark.parametrize("W", [32, 64, 1984, 2016, 4000])
def test_shapes_rules_turns(W, H, test_hooks):
    board = start(W, H)
    with golhip.Board(W, H) as b, golhip.Board(W, H) as d:
        d.set_option("rule_kernel", 2)
        for rule in RULES:
            b.set_rule(rule)
            assert golhip.rule_format(*b.rule()) == golhip.rule_format(*golhip.rule_parse(rule))
            b.load_bytes(board)
            want, turn = board, 0
            for n in (1, CAP, CAP + 1, 2 * CAP + 3):
                want, turn = model(want, rule, n), turn + n
                b.step(n)
                check(b, want, turn, (W, H, rule, turn))
            p = b.perf()
            assert p["kernel_variant"] == 5 and all(p[k] == 0 for k in RESIDENT_OR_SKEW), p
            if rule in LISTED:  # the dynamic policy on a listed rule: the same board
                d.set_rule(rule)
                d.load_bytes(board)
                d.step(turn)
                check(d, want, turn, (W, H, rule, "dynamic"))


# ---------------------------------------------------------------- widths that are no multiple of 32
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("H", [7, 37])
@pytest.mark.parametrize("W", [16, 33, 1000, 2017])
def test_odd_widths(W, H, pad):
    """pad 1: the wide board inherits the rule and fuses turns on K11; pad 0:
    K11's own one-turn form closes the row seam.  B0 rules raise every padding
    bit a kernel forgets to clear."""
    board = start(W, H)
    with golhip.Board(W, H) as b:
        b.set_pad_step(pad)
        for rule in (HIGHLIFE, "B0/S8", "B012345678/S", "B3578/S1246"):
            b.set_rule(rule)
            b.load_bytes(board)
            b.perf_reset()
            want, turn = board, 0
            for n in (1, 2, CAP + 3):
                want, turn = model(want, rule, n), turn + n
                b.step(n)
                check(b, want, turn, (W, H, pad, rule, turn))
                assert tail_bits_zero(b, W), (W, H, pad, rule, turn)
            p = b.perf()
            assert p["kernel_variant"] == 5 and p["rule_launches"] == p["step_launches"] > 0, p
            assert (p["pad_launches"] > 0) == bool(pad), p
            if not pad:
                assert p["step_launches"] == turn, p


# ---------------------------------------------------------------- the rule changes mid-run
def test_set_rule_mid_run():
    W, H = 192, 37
    board = start(W, H)
    conway = golhip.rule_format(*golhip.CONWAY)
    with golhip.Board(W, H) as b:
        assert b.rule() == golhip.CONWAY
        b.load_bytes(board)
        b.step(10, want_flips=True)
        want = model(board, conway, 10)
        kept = b.alive_count()
        flips = b.flips()
        b.set_rule(HIGHLIFE)  # the board, the turn, the kept count and the flip list stay
        assert b.turn() == 10 and b.alive_count() == kept == (int((want == 255).sum()), 10)
        assert np.array_equal(b.flips(), flips) and np.array_equal(b.snapshot_bytes(), want)
        assert b.perf()["rule_launches"] == 0
        b.step(10)
        want = model(want, HIGHLIFE, 10)
        check(b, want, 20, "HighLife")
        assert b.perf()["kernel_variant"] == 5
        b.set_rule(golhip.CONWAY)
        n0 = b.perf()["rule_launches"]
        b.step(10)
        check(b, model(want, conway, 10), 30, "Conway again")
        p = b.perf()
        assert p["rule_launches"] == n0 and p["kernel_variant"] != 5, p
        for bad in ((0x200, 0), (0, 0x200)):
            with pytest.raises(golhip.GolHipError) as e:
                b.set_rule(bad)
            assert e.value.code == -1 and "0x1FF" in str(e.value)


# ---------------------------------------------------------------- closure: every planned depth has a kernel
def test_every_tb_depth_has_a_rule_kernel():
    """tb_depth 1..32 on a rule handle (128 x 40): the deepest launch is the
    largest of K11's depths within min(tb_depth, 16), step(E) is one K11
    launch, a longer step is exact, and nothing resident or skewed runs."""
    W, H = 128, 40
    depths = [1, 2, 4, 6, 8, 12, 16]
    board = start(W, H)
    with golhip.Board(W, H) as b:
        b.set_rule(HIGHLIFE)
        for t in range(1, 33):
            E, more = max(d for d in depths if d <= t), 2 * t + 5
            b.set_tb_depth(t)
            b.load_bytes(board)
            p0 = b.perf()
            b.step(E)
            p1 = b.perf()
            want = model(board, HIGHLIFE, E)
            check(b, want, E, (t, E))
            assert p1["step_launches"] - p0["step_launches"] == 1 and p1["step_turns"] - p0["step_turns"] == E, (t, p1)
            assert p1["tb_depth"] == min(t, CAP) if t != 9 else p1["tb_depth"] == 8, (t, p1)
            b.step(more)
            p2 = b.perf()
            check(b, model(want, HIGHLIFE, more), E + more, (t, more))
            assert p2["step_launches"] - p1["step_launches"] >= -(-more // E), (t, p2)
            assert p2["kernel_variant"] == 5 and p2["words_per_lane"] == 1, (t, p2)
            assert p2["rule_launches"] == p2["step_launches"] > 0, (t, p2)
            assert all(p2[k] == 0 for k in RESIDENT_OR_SKEW), (t, p2)


# ---------------------------------------------------------------- three strips of uneven height
CUTS = [(0, 5), (5, 20), (25, 12)]


def strips(W, H=37):
    return [golhip.Board(W, H, row0=r0, rows=n) for r0, n in CUTS]


def load_strips(bs, board):
    for b, (r0, n) in zip(bs, CUTS):
        b.load_bytes(np.ascontiguousarray(board[r0:r0 + n]))


def gather(bs):
    return np.concatenate([b.snapshot_bytes() for b in bs])


def diffs(board, rule, turns):
    """The model's boards and per-turn flip lists (x, y), row-major."""
    out, cur = [], board
    for _ in range(turns):
        nxt = model(cur, rule, 1)
        out.append(flips_np(cur, nxt))
        cur = nxt
    return cur, out


@pytest.mark.parametrize("W", [64, 1000])
def test_strips(W):
    H = 37
    board = start(W, H)
    bs = strips(W)
    try:
        golhip.group_set_rule(bs, HIGHLIFE)
        load_strips(bs, board)
        golhip.group_step(bs, CAP + 3)
        want = model(board, HIGHLIFE, CAP + 3)
        assert np.array_equal(gather(bs), want)
        assert sum(b.alive_count()[0] for b in bs) == int((want == 255).sum())
        assert all(b.turn() == CAP + 3 and tail_bits_zero(b, W) for b in bs)
        assert all(b.perf()["kernel_variant"] == 5 and b.perf()["skew_launches"] == 0 for b in bs)
        # group_step_ex with flips(): the last turn's list, strip by strip
        golhip.group_step(bs, 5, want_flips=True)
        prev, want = model(want, HIGHLIFE, 4), model(want, HIGHLIFE, 5)
        assert np.array_equal(gather(bs), want)
        got = np.concatenate([b.flips() for b in bs])
        assert np.array_equal(got, flips_np(prev, want))
        # group_flip_stream: a cap that stops the batch after two turns
        final, lists = diffs(want, HIGHLIFE, 4)
        cap = len(lists[0]) + len(lists[1]) + len(lists[2]) - 1
        ent, counts, done = golhip.group_flip_stream(bs, 4, cap)
        assert done == 2 and list(counts) == [len(lists[0]), len(lists[1])]
        assert np.array_equal(ent, np.concatenate(lists[:2]))
        assert all(b.turn() == CAP + 10 for b in bs)
        ent, counts, done = golhip.group_flip_stream(bs, 2, cap)
        assert done == 2 and np.array_equal(ent, np.concatenate(lists[2:]))
        assert np.array_equal(gather(bs), final)
        # strips that disagree on the rule are no group
        bs[1].set_rule(SEEDS)
        for call in (lambda: golhip.group_step(bs, 1), lambda: golhip.group_flip_stream(bs, 1, 1 << 16),
                     lambda: golhip.group_view_frame(bs), lambda: golhip.group_stamp(bs, np.ones((2, 2), bool), 0, 0)):
            with pytest.raises(golhip.GolHipError, match="another rule") as e:
                call()
            assert e.value.code == -1
        assert np.array_equal(gather(bs), final)
    finally:
        for b in bs:
            b.close()


# ---------------------------------------------------------------- flip streams of one handle
@pytest.mark.parametrize("W,H", [(64, 37), (33, 7)])
def test_flip_streams(W, H):
    board = start(W, H)
    final, lists = diffs(board, HIGHLIFE, 6)
    with golhip.Board(W, H) as b:
        b.set_rule(HIGHLIFE)
        b.load_bytes(board)
        # not even the first turn fits: ERANGE and nothing advanced
        with pytest.raises(golhip.GolHipError) as e:
            b.flip_stream(3, len(lists[0]) - 1)
        assert e.value.code == golhip.GOLHIP_ERANGE and b.turn() == 0
        assert np.array_equal(b.snapshot_bytes(), board)
        # a cap that stops the batch before its third turn
        cap = len(lists[0]) + len(lists[1]) + len(lists[2]) - 1
        ent, counts, done = b.flip_stream(5, cap)
        assert done == 2 and b.turn() == 2 and list(counts) == [len(lists[0]), len(lists[1])]
        assert np.array_equal(ent, np.concatenate(lists[:2]))
        ent, counts, done = b.flip_stream(2, cap, golhip.FLIPS_INDEX)
        assert done == 2 and b.turn() == 4
        xy = np.concatenate(lists[2:4])
        assert np.array_equal(ent, (xy[:, 1].astype(np.int64) * W + xy[:, 0]).astype(np.uint32))
        xy, counts = b.step_flips(2, W * H * 2)
        assert list(counts) == [len(lists[4]), len(lists[5])] and np.array_equal(xy, np.concatenate(lists[4:]))
        check(b, final, 6, (W, H))
        assert tail_bits_zero(b, W)
        p = b.perf()
        assert p["kernel_variant"] == 5 and p["flip_launches"] == 0, p


# ---------------------------------------------------------------- rings run Conway only
def test_rings_refuse_rules(test_hooks):
    hl = golhip.rule_parse(HIGHLIFE)
    with golhip.Board(64, 64) as b:
        b.comm_init(golhip.unique_id(), 1, 0)
        with pytest.raises(golhip.GolHipError, match="communicator") as e:
            b.set_rule(hl)
        assert e.value.code == -1 and b.rule() == golhip.CONWAY
        b.set_rule(golhip.CONWAY)
    with golhip.Board(64, 64) as b:
        b.set_rule(hl)
        with pytest.raises(golhip.GolHipError, match="Conway") as e:
            b.comm_init(golhip.unique_id(), 1, 0)
        assert e.value.code == -1
    with golhip.Board(64, 64, row0=0, rows=32) as b:
        b.set_rule(hl)
        with pytest.raises(golhip.GolHipError, match="Conway"):
            b.test_ring_init(2, 0, 32, lambda *a: 0)
        b.set_rule(golhip.CONWAY)
        b.test_ring_init(2, 0, 32, lambda *a: 0)
        with pytest.raises(golhip.GolHipError, match="communicator"):
            b.set_rule(hl)


# ---------------------------------------------------------------- the rule-agnostic neighbours
def test_neighbours_on_a_highlife_board(tmp_path):
    W, H = 96, 37
    board = start(W, H)
    want = model(board, HIGHLIFE, 7)
    rle = lambda rule: f"x = 3, y = 3{', rule = ' + rule if rule else ''}\nbo$2bo$3o!\n"
    files = {}
    for name, rule in (("highlife", "B36/S23"), ("conway", "B3/S23"), ("none", ""), ("legacy", "23/36")):
        files[name] = str(tmp_path / f"{name}.rle")
        with open(files[name], "w") as f:
            f.write(rle(rule))
    glider = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], bool)
    with golhip.Board(W, H) as b, golhip.Board(W, H) as c:
        b.set_rule(HIGHLIFE)
        b.load_bytes(board)
        b.step(7)
        frame, at = b.view_frame(fmt=golhip.VIEW_GRAY8)
        assert at == 7 and np.array_equal(frame, golhip.view_frame_np(pack_bits(want), W, H, fmt=golhip.VIEW_GRAY8))
        # checkpoint: the file keeps no rule, the resume sets it again
        path = str(tmp_path / "hl.ckpt")
        golhip.checkpoint_begin([b], path).wait()
        c.set_rule(HIGHLIFE)
        info = golhip.checkpoint_load([c], path)
        assert info["turn"] == 7 and c.turn() == 7
        for x in (b, c):
            x.step(CAP + 1)
        check(c, model(want, HIGHLIFE, CAP + 1), 7 + CAP + 1, "resumed")
        assert c.board_hash() == b.board_hash()
        # pattern files: the board's rule or none
        cells = b.snapshot_bytes() == 255
        for name in ("highlife", "legacy", "none"):
            golhip.stamp_file(b, files[name], 5, 6, golhip.STAMP_COPY)
        cells[6:9, 5:8] = glider
        assert np.array_equal(b.snapshot_bytes() == 255, cells)
        with pytest.raises(golhip.GolHipError, match=r"rule B3/S23 is not the board's B36/S23") as e:
            golhip.stamp_file(b, files["conway"], 0, 0)
        assert e.value.code == -1
        # a Conway board: today's behaviour, word for word
        c.set_rule(golhip.CONWAY)
        with pytest.raises(golhip.GolHipError, match=r"RLE: rule B36/S23 is not Conway's B3/S23"):
            golhip.stamp_file(c, files["highlife"], 0, 0)
        golhip.stamp_file(c, files["conway"], 0, 0)
        assert np.array_equal(b.snapshot_bytes() == 255, cells)
