"""The bounded plane on the GPU: golhip_set_topology and K15
(csrc/gol_rule_plane.hip), K11 with every cell outside the board forced dead at
every fused turn.  Judged bit for bit (board, alive count, golhip_board_hash,
the padding bits of a row's last word) by golhip.life_like_plane_np, the numpy
model that tests/test_plane_cpu.py pins to the definition.

Every case starts from an input that tells the plane from the torus (a border
ring, blinkers across every edge and corner, gliders aimed at every edge, a
seeded soup) and asserts on the host that the two models disagree after each
of its calls: a case in which they agree would pass on the torus kernel too.

Shapes: one partial word, one word, a word and a bit, a full tile (62 words),
a tile and a bit, two tiles, two full tiles and a bit; boards with fewer rows
than a launch fuses turns; one-turn and fused calls and the counts around the
cap of 16.
"""
import functools

import numpy as np
import pytest

from oracle.oracle import flips_np, pack_bits

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

CAP = 16
CONWAY, HIGHLIFE, UNLISTED, B0S8, ALLB = "B3/S23", "B36/S23", "B3578/S1246", "B0/S8", "B012345678/S"
RULES = [CONWAY, HIGHLIFE, UNLISTED, B0S8, ALLB]
LISTED = [CONWAY, HIGHLIFE]  # rules with a static instance: both policies
TURNS = (1, 2, 16, 17, 35)   # the calls of a case, one after the other
WS = [16, 31, 32, 33, 64, 1984, 1985, 2016, 3969]
HS = [1, 2, 3, 17, 67]
# every W and every H, each with every rule and every call; the corners of the product
SHAPES = [(16, 17), (31, 1), (32, 2), (33, 3), (64, 67), (1984, 17), (1985, 67), (2016, 1), (3969, 2),
          (33, 67), (1985, 3), (3969, 17), (16, 1)]
assert {w for w, _ in SHAPES} == set(WS) and {h for _, h in SHAPES} == set(HS)
KINDS = ("ring", "blinkers", "gliders", "soup")


# ---------------------------------------------------------------- inputs
def ring(W, H):
    b = np.zeros((H, W), np.uint8)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = 255
    return b


def blinkers(W, H):
    """Blinkers whose middle cell sits on an edge or a corner cell: on the torus
    their third cell is on the far side."""
    b = np.zeros((H, W), np.uint8)
    for x in (W // 3, (2 * W) // 3):
        for y in (-1, 0, 1):                      # across the top and the bottom edge
            b[y % H, x] = 255
            b[(H - 1 + y) % H, (x + 3) % W] = 255
    for y in (H // 3, (2 * H) // 3):
        for x in (-1, 0, 1):                      # across the left and the right edge
            b[y, x % W] = 255
            b[(y + 3) % H, (W - 1 + x) % W] = 255
    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        for k in (-1, 0, 1):                      # the corners, along the diagonal's row
            b[cy, (cx + k) % W] = 255
    return b


GLIDER_SE = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], np.uint8) * np.uint8(255)  # moves +x, +y


def gliders(W, H):
    """One glider flush against each edge, heading out through it: its first
    turn already bears cells beyond the edge, which only the torus keeps."""
    b = np.zeros((H, W), np.uint8)
    if W < 16 or H < 16:
        return None
    b[H - 3:H, W // 2:W // 2 + 3] = GLIDER_SE                        # out through the bottom
    b[0:3, W // 2 - 6:W // 2 - 3] = GLIDER_SE[::-1, ::-1]            # out through the top
    b[H // 2:H // 2 + 3, W - 3:W] = GLIDER_SE.T                      # ... the right
    b[H // 2 - 6:H // 2 - 3, 0:3] = GLIDER_SE.T[::-1, ::-1]          # ... the left
    return b


def soup(W, H, seed=0):
    rng = np.random.default_rng(0x9C4E + 977 * W + 31 * H + seed)
    return (rng.random((H, W)) < 0.37).astype(np.uint8) * np.uint8(255)


def make(kind, W, H):
    b = {"ring": ring, "blinkers": blinkers, "gliders": gliders, "soup": soup}[kind](W, H)
    if b is not None:
        b.setflags(write=False)
    return b


def masks(rule):
    return golhip.rule_parse(rule)


def plane(board, rule, turns):
    return golhip.life_like_plane_np(board, *masks(rule), turns)


def torus(board, rule, turns):
    return golhip.life_like_np(board, *masks(rule), turns)


def topology_blind(rule):
    """A rule whose next state does not look at the neighbour count (B012345678/S
    inverts the board every turn, on any topology): the one kind of rule under
    which no input can tell the plane from the torus.  It stays in RULES for
    what it does show: every padding bit and every outside row a kernel forgets
    to clear comes alive at once."""
    b, s = masks(rule)
    return b in (0, 0x1FF) and s in (0, 0x1FF)


SOUP_SEEDS = range(16)


def make_all(kind, W, H):
    """The boards of one input kind: the deterministic ones have one (none where
    the kind does not fit the shape), the soup one a seed."""
    if kind == "soup":
        return [soup(W, H, seed) for seed in SOUP_SEEDS]
    b = make(kind, W, H)
    return [] if b is None else [b]


@functools.lru_cache(maxsize=None)
def tells(kind, W, H, rule, turns=TURNS):
    """(board, [plane board after each call]) of input `kind`, and of no other:
    the plane and the torus model differ after every one of the calls
    (topology_blind rules excepted: there they cannot).  The soup is the first
    seed of SOUP_SEEDS for which that holds.  None where the kind does not fit
    the shape or does not tell the two apart at it."""
    for board in make_all(kind, W, H):
        board.setflags(write=False)
        p, t, out = board, board, []
        for n in turns:
            p, t = plane(p, rule, n), torus(t, rule, n)
            if np.array_equal(p, t) and not topology_blind(rule):
                break
            p.setflags(write=False)
            out.append(p)
        else:
            return board, out
    return None


def trajectory(kind, W, H, rule, turns=TURNS):
    """tells(), where the case needs that input: none is a test error, never a skip."""
    got = tells(kind, W, H, rule, turns)
    assert got is not None, f"{kind} does not tell the plane from the torus at {W} x {H}, {rule}, calls {turns}"
    return (kind, *got)


def check(b, want, turn, W, what):
    """Board, alive count, digest and the padding bits of handle b against the model's board."""
    assert np.array_equal(b.snapshot_bytes(), want), what
    assert b.alive_count() == (int((want == 255).sum()), turn), what
    assert b.board_hash() == golhip.board_hash_np(pack_bits(want)), what
    if W % 32:
        assert not np.any(b.snapshot_bits()[:, -1] >> np.uint32(W % 32)), what


# ---------------------------------------------------------------- the inputs disagree by construction
@pytest.mark.parametrize("W,H", [(64, 67), (1985, 17)])
def test_inputs_tell_the_plane_from_the_torus(W, H):
    """Ring, blinkers and gliders differ between the models by construction (no
    fallback to another kind), under Conway's rule, after every call; the soup
    under every rule."""
    for kind in KINDS:
        for rule in (RULES if kind == "soup" else [CONWAY]):
            assert tells(kind, W, H, rule) is not None, (kind, rule)
    with golhip.Board(W, H) as b:  # and the torus kernel does not pass for the plane's
        board = make("ring", W, H)
        b.load_bytes(board)
        b.step(3)
        assert np.array_equal(b.snapshot_bytes(), torus(board, CONWAY, 3))
        assert not np.array_equal(b.snapshot_bytes(), plane(board, CONWAY, 3))


# ---------------------------------------------------------------- shapes x rules x calls
@pytest.mark.parametrize("W,H", SHAPES)
def test_shapes_rules_turns(W, H, test_hooks):
    with golhip.Board(W, H) as b, golhip.Board(W, H) as d:
        assert b.topology() == golhip.TOPOLOGY_TORUS
        b.set_topology(golhip.TOPOLOGY_PLANE)
        d.set_topology(golhip.TOPOLOGY_PLANE)
        assert b.topology() == golhip.TOPOLOGY_PLANE
        d.set_option("rule_kernel", 2)
        for j, rule in enumerate(RULES):
            # the soup at every shape under every rule (a seed that tells: an error if none does), and
            # one of the constructed inputs in turn wherever it fits the shape and tells the two apart there
            cases = [trajectory("soup", W, H, rule)]
            built = KINDS[(j + W + H) % 3]
            if tells(built, W, H, rule) is not None:
                cases.append(trajectory(built, W, H, rule))
            for kind, board, wants in cases:
                b.set_rule(rule)
                b.load_bytes(board)
                b.perf_reset()
                turn = 0
                for n, want in zip(TURNS, wants):
                    p0 = b.perf()
                    b.step(n)
                    turn += n
                    check(b, want, turn, W, (W, H, rule, kind, turn))
                    p1 = b.perf()
                    if n <= CAP and n in (1, 2, 16):  # a depth with an instance: one launch, at any width
                        assert p1["step_launches"] - p0["step_launches"] == 1, (W, H, n, p1)
                p = b.perf()
                assert p["kernel_variant"] == 6 and p["pad_launches"] == 0 and p["words_per_lane"] == 1, p
                assert p["rule_launches"] == p["step_launches"] > 0 and p["step_turns"] == turn, p
                assert all(p[k] == 0 for k in ("persist_launches", "skew_launches", "lds_launches", "pair_launches")), p
            kind, board, wants = cases[0]
            if rule in LISTED:  # the dynamic policy on a listed rule: the same boards
                d.set_rule(rule)
                d.load_bytes(board)
                d.step(TURNS[0] + TURNS[1] + TURNS[2])
                check(d, wants[2], 19, W, (W, H, rule, "dynamic"))
                assert d.perf()["kernel_variant"] == 6


@pytest.mark.parametrize("W", [33, 1985])
def test_sixteen_turns_are_one_launch_at_any_width(W):
    H = 17
    kind, board, wants = trajectory("ring", W, H, HIGHLIFE, (16,))
    with golhip.Board(W, H) as b:
        b.set_rule(HIGHLIFE)
        b.set_topology(golhip.TOPOLOGY_PLANE)
        b.load_bytes(board)
        b.perf_reset()
        b.step(16)
        check(b, wants[0], 16, W, (W, kind))
        p = b.perf()
        assert p["step_launches"] == 1 and p["kernel_variant"] == 6 and p["pad_launches"] == 0, p
        assert p["rule_launches"] == 1 and p["step_turns"] == 16, p


# ---------------------------------------------------------------- strips
CUTS3 = [(0, 5), (5, 20), (25, 12)]  # a strip of 5 rows: shorter than the fused depth
CUTS2 = [(0, 20), (20, 17)]


def strips(W, cuts, H=37):
    return [golhip.Board(W, H, row0=r0, rows=n) for r0, n in cuts]


def load_strips(bs, cuts, board):
    for b, (r0, n) in zip(bs, cuts):
        b.load_bytes(np.ascontiguousarray(board[r0:r0 + n]))


def gather(bs):
    return np.concatenate([b.snapshot_bytes() for b in bs])


STRIP_INPUT = {(64, 2): "ring", (64, 3): "soup", (1000, 2): "gliders", (1000, 3): "soup"}


@pytest.mark.parametrize("cuts", [CUTS2, CUTS3], ids=["2", "3"])
@pytest.mark.parametrize("W", [64, 1000])
def test_strips(W, cuts):
    H = 37
    rule = HIGHLIFE if W == 64 else B0S8
    kind, board, wants = trajectory(STRIP_INPUT[W, len(cuts)], W, H, rule, (1, 16, 40))
    bs = strips(W, cuts)
    try:
        golhip.group_set_rule(bs, rule)
        golhip.group_set_topology(bs, golhip.TOPOLOGY_PLANE)
        load_strips(bs, cuts, board)
        turn = 0
        for n, want in zip((1, 16, 40), wants):
            golhip.group_step(bs, n)
            turn += n
            assert np.array_equal(gather(bs), want), (W, n)
            assert sum(b.alive_count()[0] for b in bs) == int((want == 255).sum())
            for b in bs:
                assert b.turn() == turn
                if W % 32:
                    assert not np.any(b.snapshot_bits()[:, -1] >> np.uint32(W % 32))
        for b in bs:
            p = b.perf()
            assert p["kernel_variant"] == 6 and p["pad_launches"] == 0 and p["skew_launches"] == 0, p
            assert p["rule_launches"] == p["step_launches"] > 0, p
        # strips that disagree on the topology are no group
        bs[1].set_topology(golhip.TOPOLOGY_TORUS)
        for call in (lambda: golhip.group_step(bs, 1), lambda: golhip.group_flip_stream(bs, 1, 1 << 16),
                     lambda: golhip.group_alive_box(bs)):
            with pytest.raises(golhip.GolHipError, match="another topology") as e:
                call()
            assert e.value.code == -1
        assert np.array_equal(gather(bs), wants[-1])
    finally:
        for b in bs:
            b.close()


# ---------------------------------------------------------------- flip streams
def diffs(board, rule, turns):
    """The plane model's board and per-turn flip lists (x, y), row-major."""
    out, cur = [], board
    for _ in range(turns):
        nxt = plane(cur, rule, 1)
        out.append(flips_np(cur, nxt))
        cur = nxt
    return cur, out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("W,H", [(64, 37), (33, 7)])
def test_flip_streams(W, H, mode):
    kind, board, _ = trajectory("ring", W, H, HIGHLIFE, (6,))
    final, lists = diffs(board, HIGHLIFE, 6)
    assert not np.array_equal(final, torus(board, HIGHLIFE, 6))
    with golhip.Board(W, H) as b:
        b.set_rule(HIGHLIFE)
        b.set_rule_flips(mode)
        b.set_topology(golhip.TOPOLOGY_PLANE)
        b.load_bytes(board)
        cap = len(lists[0]) + len(lists[1]) + len(lists[2]) - 1  # stops the batch before its third turn
        ent, counts, done = b.flip_stream(5, cap)
        assert done == 2 and b.turn() == 2 and list(counts) == [len(lists[0]), len(lists[1])]
        assert np.array_equal(ent, np.concatenate(lists[:2]))
        ent, counts, done = b.flip_stream(2, len(lists[2]) + len(lists[3]), golhip.FLIPS_INDEX)
        assert done == 2 and b.turn() == 4
        xy = np.concatenate(lists[2:4])
        assert np.array_equal(ent, (xy[:, 1].astype(np.int64) * W + xy[:, 0]).astype(np.uint32))
        xy, counts = b.step_flips(2, W * H * 2)
        assert list(counts) == [len(lists[4]), len(lists[5])] and np.array_equal(xy, np.concatenate(lists[4:]))
        check(b, final, 6, W, (W, H, mode))
        p = b.perf()
        # no K14 launch: one K15 turn a list, and the turn the stopped batch ran and took back
        assert p["kernel_variant"] == 6 and p["flip_launches"] == 0 and p["rule_launches"] == 6 + 1, p
        # golhip_step with want_flips: the last turn's list
        b.step(3, want_flips=True)
        prev, want = plane(final, HIGHLIFE, 2), plane(final, HIGHLIFE, 3)
        assert np.array_equal(b.flips(), flips_np(prev, want))
        check(b, want, 9, W, (W, H, mode, "want_flips"))


CUTS_7 = [(0, 2), (2, 3), (5, 2)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("W,H,cuts", [(64, 37, CUTS3), (64, 37, CUTS2), (33, 7, CUTS_7)], ids=["64x37-3", "64x37-2", "33x7-3"])
def test_group_flip_stream(W, H, cuts, mode):
    kind, board, _ = trajectory("ring", W, H, HIGHLIFE, (5,))
    final, lists = diffs(board, HIGHLIFE, 5)
    bs = strips(W, cuts, H)
    try:
        golhip.group_set_rule(bs, HIGHLIFE)
        golhip.group_set_rule_flips(bs, mode)
        golhip.group_set_topology(bs, golhip.TOPOLOGY_PLANE)
        load_strips(bs, cuts, board)
        cap = len(lists[0]) + len(lists[1]) + len(lists[2]) - 1  # stops the batch before its third turn
        ent, counts, done = golhip.group_flip_stream(bs, 4, cap)
        assert done == 2 and list(counts) == [len(lists[0]), len(lists[1])]
        assert np.array_equal(ent, np.concatenate(lists[:2]))
        ent, counts, done = golhip.group_flip_stream(bs, 2, len(lists[2]) + len(lists[3]))
        assert done == 2 and np.array_equal(ent, np.concatenate(lists[2:4]))
        assert np.array_equal(gather(bs), plane(board, HIGHLIFE, 4))
        # group_step with want_flips: the last turn's list, strip by strip
        golhip.group_step(bs, 1, want_flips=True)
        assert np.array_equal(np.concatenate([b.flips() for b in bs]), lists[4])
        assert np.array_equal(gather(bs), final)
        assert sum(b.alive_count()[0] for b in bs) == int((final == 255).sum())
        for b in bs:
            p = b.perf()
            assert b.turn() == 5 and p["flip_launches"] == 0 and p["kernel_variant"] == 6 and p["pad_launches"] == 0, p
            assert p["rule_launches"] == p["step_launches"] > 0, p
            if W % 32:
                assert not np.any(b.snapshot_bits()[:, -1] >> np.uint32(W % 32))
    finally:
        for b in bs:
            b.close()


# ---------------------------------------------------------------- refusals and switches
def test_refusals(test_hooks):
    with golhip.Board(64, 64, row0=0, rows=32) as b:
        b.test_ring_init(2, 0, 32, lambda *a: 0)
        with pytest.raises(golhip.GolHipError, match="communicator") as e:
            b.set_topology(golhip.TOPOLOGY_PLANE)
        assert e.value.code == -1 and b.topology() == golhip.TOPOLOGY_TORUS
        b.set_topology(golhip.TOPOLOGY_TORUS)
    with golhip.Board(64, 64, row0=0, rows=32) as b:
        b.set_topology(golhip.TOPOLOGY_PLANE)
        with pytest.raises(golhip.GolHipError, match="torus only") as e:
            b.test_ring_init(2, 0, 32, lambda *a: 0)
        assert e.value.code == -1
    with golhip.Board(64, 64) as b:
        b.set_topology(golhip.TOPOLOGY_PLANE)
        with pytest.raises(golhip.GolHipError, match="torus only"):
            b.comm_init(golhip.unique_id(), 1, 0)
        for bad in (-1, 2):
            with pytest.raises(golhip.GolHipError, match="topology") as e:
                b.set_topology(bad)
            assert e.value.code == -1 and b.topology() == golhip.TOPOLOGY_PLANE
    with golhip.Board(33, 7) as b:  # the padded torus and the plane refuse each other
        b.set_pad_step(1)
        with pytest.raises(golhip.GolHipError, match="pad_step") as e:
            b.set_topology(golhip.TOPOLOGY_PLANE)
        assert e.value.code == -1 and b.topology() == golhip.TOPOLOGY_TORUS
        b.set_pad_step(-1)
        b.set_topology(golhip.TOPOLOGY_PLANE)
        with pytest.raises(golhip.GolHipError, match="plane") as e:
            b.set_pad_step(1)
        assert e.value.code == -1
        b.set_pad_step(0)
        b.set_pad_step(-1)


@pytest.mark.parametrize("W,H", [(64, 37), (1000, 37)])
def test_switching_mid_run(W, H):
    board = make("ring", W, H)
    with golhip.Board(W, H) as b:
        b.load_bytes(board)
        b.step(10, want_flips=True)  # Conway's own kernels, on the torus
        want = torus(board, CONWAY, 10)
        kept, flips = b.alive_count(), b.flips()
        b.set_topology(golhip.TOPOLOGY_PLANE)  # the board, the turn, the kept count and the flip list stay
        assert b.turn() == 10 and b.alive_count() == kept and np.array_equal(b.flips(), flips)
        assert np.array_equal(b.snapshot_bytes(), want) and b.perf()["rule_launches"] == 0
        b.step(CAP + 3)
        assert not np.array_equal(plane(want, CONWAY, CAP + 3), torus(want, CONWAY, CAP + 3))
        want = plane(want, CONWAY, CAP + 3)
        check(b, want, 10 + CAP + 3, W, "plane from turn 10")
        assert b.perf()["kernel_variant"] == 6
        b.set_topology(golhip.TOPOLOGY_TORUS)
        n0 = b.perf()["rule_launches"]
        ringed = want.copy()  # the ring again, so the torus has something to carry across the seam
        ringed[board == 255] = 255
        b.load_bytes(ringed)
        b.step(CAP + 3)
        assert not np.array_equal(plane(ringed, CONWAY, CAP + 3), torus(ringed, CONWAY, CAP + 3))
        assert np.array_equal(b.snapshot_bytes(), torus(ringed, CONWAY, CAP + 3))
        p = b.perf()
        assert p["rule_launches"] == n0 and p["kernel_variant"] != 6, p


# ---------------------------------------------------------------- observers
def test_observers(tmp_path):
    W, H = 96, 37
    glider = np.array([[0, 1, 0], [0, 0, 1], [1, 1, 1]], bool)
    with golhip.Board(W, H) as b, golhip.Board(W, H) as t:
        b.set_topology(golhip.TOPOLOGY_PLANE)
        for x in (b, t):
            x.clear()
            x.stamp(glider, W - 1, H - 1)  # a stamp still addresses the torus: across the corner seam
        cells = b.snapshot_bytes()
        assert (cells == 255).sum() == 5 and np.array_equal(cells, t.snapshot_bytes())
        # one 3 x 3 box across both seams on the torus; two fragments in a full-board box on the plane
        assert t.alive_box() == (W - 1, H - 1, 3, 3)
        assert b.alive_box() == (0, 0, W, H)
        ys, xs = np.nonzero(cells == 255)
        assert (xs.min(), ys.min(), xs.max(), ys.max()) == (0, 0, W - 1, H - 1)
        path = str(tmp_path / "plane.rle")
        info = golhip.save_rle(b, path)
        assert info["width"] == W and info["height"] == H and info["alive"] == 5
        head = [l for l in open(path).read().split("\n") if l.startswith("x =")][0]
        assert head == f"x = {W}, y = {H}, rule = B3/S23:P{W},{H}"
        tpath = str(tmp_path / "torus.rle")
        golhip.save_rle(t, tpath)
        assert [l for l in open(tpath).read().split("\n") if l.startswith("x =")][0] == "x = 3, y = 3, rule = B3/S23"
        assert golhip.rule_parse_ex(head.split("rule = ")[1]) == (*golhip.CONWAY, golhip.TOPOLOGY_PLANE, W, H)
        # the file goes back onto a torus handle and onto a plane handle: its bounds are not the board's
        for x in (b, t):
            x.clear()
            golhip.stamp_file(x, path, 0, 0, golhip.STAMP_COPY)
            assert np.array_equal(x.snapshot_bytes(), cells)
        # and the two handles part ways from there
        b.step(4)
        t.step(4)
        assert np.array_equal(b.snapshot_bytes(), plane(cells, CONWAY, 4))
        assert np.array_equal(t.snapshot_bytes(), torus(cells, CONWAY, 4))
        assert not np.array_equal(b.snapshot_bytes(), t.snapshot_bytes())
        # a HighLife plane names its rule and its bounds
        b.set_rule(HIGHLIFE)
        b.load_bytes(make("ring", W, H))
        golhip.save_rle(b, path, box=(2, 3, 40, 30))
        assert "x = 40, y = 30, rule = B36/S23:P96,37\n" in open(path).read()
