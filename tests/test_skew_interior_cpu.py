"""The interior span of a K1w band's main loop (csrc/gol_skew_span.h, DESIGN.md
§5.20), through golhip_skew_span, by brute force against the predicates the
general loop body evaluates row by row (gol_kernels.hip stream_skew: the row
cursor's wrap and clamp, the store's row range, the count range).  No GPU.

For every case: each body inside the span meets every condition for every
lane (both halves of a half-tile wave), consecutive bodies of the span read
consecutive rows, the span is the longest run of such bodies to within one
body at each end, and it is empty for a counting launch and with option
skew_interior off."""
import ctypes

import pytest

golhip = pytest.importorskip("golhip")

i32 = ctypes.c_int32


class SpanIn(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("ab", "eb", "depth", "self", "pair", "off", "wrap", "rmax", "half", "dr",
                                   "row_words", "counts", "enabled")]


@pytest.fixture(scope="module")
def span():
    lib = golhip.load()
    fn = lib.golhip_skew_span
    fn.argtypes = [ctypes.POINTER(SpanIn), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    fn.restype = ctypes.c_int
    lo, hi = i32(), i32()

    def call(**kw):
        a = SpanIn(**kw)
        assert fn(ctypes.byref(a), ctypes.byref(lo), ctypes.byref(hi)) == 0, kw
        return lo.value, hi.value
    return call


def body_rows(c):
    return 6 if c["pair"] else 3


def main_range(c):
    """(first push, end) of the main loop: gol_kernels.hip stream_skew."""
    D, S = c["depth"], c["eb"] - c["ab"]
    k0 = 3 * ((2 * D + 2) // 3)
    return k0, S + (2 * D if c["self"] else 2 * (6 if D > 20 else 3))


def first_rows(c, k):
    """The row each half's cursor stands on when the body at push k loads its first row."""
    out = []
    for rofs in ([0, c["dr"]] if c["half"] else [0]):
        r = c["ab"] + rofs + c["off"] + k + 3
        out.append(r % c["wrap"] if c["wrap"] > 0 else r)
    return out


def body_is_interior(c, k):
    """The general body's own decisions, row by row."""
    B, D, S = body_rows(c), c["depth"], c["eb"] - c["ab"]
    if c["counts"] or not c["enabled"]:
        return False
    for r in first_rows(c, k):                      # load_next: min(r, rmax), then r = r + 1 == wrap ? 0 : r + 1
        for i in range(B):
            if r > c["rmax"]:
                return False                        # clamped
            nxt = 0 if (c["wrap"] > 0 and r + 1 == c["wrap"]) else r + 1
            if i + 1 < B and nxt != r + 1:
                return False                        # wraps inside the body
            r = nxt
    for oi in range(k - 3 - 2 * D, k - 3 - 2 * D + B):  # emit: (unsigned)oi < S
        if not 0 <= oi < S:
            return False
    return True


def check(span, c):
    B = body_rows(c)
    k0, kmain = main_range(c)
    lo, hi = span(**c)
    bodies = list(range(k0, kmain, B))
    where = (c, lo, hi)
    assert lo <= hi and (lo - k0) % B == 0 and (hi - k0) % B == 0, where
    if lo == hi:
        inside = []
    else:
        assert lo >= k0 and hi - B in bodies, where
        inside = list(range(lo, hi, B))
    good = {k: body_is_interior(c, k) for k in bodies}
    joined = {k: good[k] and good.get(k + B, False) and
              all(b == a + B for a, b in zip(first_rows(c, k), first_rows(c, k + B))) for k in bodies}
    for k in inside:
        assert good[k], ("a body of the span is not interior", k, where)
        if k + B < hi:
            assert joined[k], ("the span's rows are not consecutive", k, where)
    # the runs of interior bodies that read consecutive rows, and the longest of them
    runs, cur = [], []
    for k in bodies:
        if good[k]:
            cur.append(k)
            if not joined[k]:
                runs.append(cur)
                cur = []
        elif cur:
            runs.append(cur)
            cur = []
    if cur:
        runs.append(cur)
    longest = max((len(r) for r in runs), default=0)
    assert len(inside) >= longest - 2, ("not the longest run to within a body at each end", longest, where)
    if inside:
        # no two more bodies fit at either end
        assert not (lo - 2 * B in good and joined[lo - 2 * B] and joined[lo - B]), ("extends down", where)
        assert not (joined[hi - B] and joined.get(hi, False)), ("extends up", where)
    return len(inside)


def base_case(S, D, pair, self_, ab=0):
    return dict(ab=ab, eb=ab + S, depth=D, self=self_, pair=pair, off=128, wrap=0, rmax=1 << 30, half=0, dr=0,
                row_words=64, counts=0, enabled=1)


KERNELS = [(8, 0), (8, 1), (9, 0), (16, 0), (18, 1), (20, 0)]  # (depth, pair rule): the K1w instances
HEIGHTS = [21, 22, 24, 27, 30, 33, 36, 42, 45, 48, 54, 60, 66, 72, 90, 99, 120, 150, 198, 199, 200]


def heights(pair):
    """Band heights: bands above a stack's bottom one are multiples of 3 rows (6 on the pair rule)."""
    for S in HEIGHTS:
        for self_ in (0, 1):
            if self_ or S % (6 if pair else 3) == 0:
                yield S, self_


@pytest.mark.parametrize("D,pair", KERNELS)
def test_span_without_wrap_or_clamp(span, D, pair):
    """A strip's band far from its halo clamp: everything between the first and the last stored rows."""
    B = 6 if pair else 3
    some = 0
    for S, self_ in heights(pair):
        for ab in (-D, 0, 37):
            c = base_case(S, D, pair, self_, ab)
            n = check(span, c)
            k0, kmain = main_range(c)
            want = sum(body_is_interior(c, k) for k in range(k0, kmain, B))
            assert n == want, (c, n, want)
            some += n
            assert check(span, dict(c, counts=1)) == 0
            assert check(span, dict(c, enabled=0)) == 0
            assert span(**dict(c, counts=1))[0] == span(**dict(c, counts=1))[1]
            assert span(**dict(c, enabled=0))[0] == span(**dict(c, enabled=0))[1]
    assert some > 0


@pytest.mark.parametrize("D,pair", KERNELS)
def test_span_with_the_wrap_at_every_row(span, D, pair):
    """A torus band: the row map wraps at every position of the band's rows in turn."""
    for S, self_ in heights(pair):
        if S > 66 and S != 200:
            continue
        rows = S + 2 * D + 12
        for wrap in (rows + 5, 4 * rows):
            for p in range(rows + 1):
                c = base_case(S, D, pair, self_, ab=-D)
                c.update(wrap=wrap, rmax=wrap - 1, off=(-(c["ab"] + p)) % wrap)  # band row p is the torus's row 0
                check(span, c)


@pytest.mark.parametrize("D,pair", KERNELS)
def test_span_with_the_clamp_at_every_row(span, D, pair):
    """A strip's band against the end of its buffer: rmax at every position of the band's rows."""
    for S, self_ in heights(pair):
        if S > 66 and S != 199:
            continue
        rows = S + 2 * D + 12
        for p in range(-2, rows + 1):
            c = base_case(S, D, pair, self_, ab=5)
            c.update(rmax=c["ab"] + c["off"] + p)
            check(span, c)
        # a wrap and a clamp below it
        for p in range(0, rows + 1, 5):
            c = base_case(S, D, pair, self_, ab=5)
            c.update(wrap=rows + 30, rmax=S // 2 + 7, off=(-(c["ab"] + p)) % (rows + 30))
            check(span, c)


@pytest.mark.parametrize("D,pair", [(16, 0), (18, 1), (20, 0)])   # the half-tile instances
def test_span_of_half_tiles(span, D, pair):
    """Half-wave tiles: the upper lanes' rows are dr further down, and either half may meet the wrap."""
    some = 0
    for S, self_ in heights(pair):
        if S > 60 and S != 198:
            continue
        rows = S + 2 * D + 12
        for dr in (rows + 3, 5 * rows):
            wrap = 2 * dr                                    # a torus of two halves
            for p in range(0, wrap, 1 if S <= 36 else 7):
                c = base_case(S, D, pair, self_, ab=-D)
                c.update(half=1, dr=dr, wrap=wrap, rmax=wrap - 1, off=p)
                some += check(span, c)
            c = base_case(S, D, pair, self_, ab=-D)          # a strip: no wrap, the clamp in the upper half's rows
            for p in range(0, rows + 1, 3):
                c.update(half=1, dr=dr, rmax=c["ab"] + c["off"] + dr + p)
                some += check(span, c)
    assert some > 0


def test_span_of_half_tiles_needs_both_halves_near_one_base(span):
    """Half tiles address both halves' rows from one base with 31-bit byte offsets: no span beyond that."""
    c = base_case(120, 18, 1, 1, ab=-18)
    c.update(half=1, dr=1 << 20, wrap=1 << 21, rmax=(1 << 21) - 1, off=0)
    assert check(span, dict(c, row_words=128)) > 0       # 2^21 rows of 512 bytes: 1 GiB
    lo, hi = span(**dict(c, row_words=256))              # 2 GiB
    assert lo == hi


def test_span_request_is_checked():
    lib = golhip.load()
    fn = lib.golhip_skew_span
    fn.argtypes = [ctypes.POINTER(SpanIn), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    fn.restype = ctypes.c_int
    lo, hi = i32(), i32()
    ok = base_case(60, 18, 1, 1)
    assert fn(ctypes.byref(SpanIn(**ok)), ctypes.byref(lo), ctypes.byref(hi)) == 0
    assert fn(None, ctypes.byref(lo), ctypes.byref(hi)) == -1
    assert fn(ctypes.byref(SpanIn(**ok)), None, ctypes.byref(hi)) == -1
    for bad in (dict(depth=3), dict(depth=33), dict(eb=-1), dict(dr=-1), dict(row_words=0)):
        assert fn(ctypes.byref(SpanIn(**dict(ok, **bad))), ctypes.byref(lo), ctypes.byref(hi)) == -1, bad
