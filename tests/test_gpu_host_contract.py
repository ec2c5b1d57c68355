"""Characterization of two host-side behaviours of libgolhip.so that no other
suite pins: the accepted range of every option, and the timing sums /
counters behind golhip_perf with their reset.

Both tables below are literal: read off golhip_set_option and
golhip_perf_reset, not generated from the library, so a host-side change that
moves a bound or forgets a counter fails here."""
import numpy as np
import pytest

from oracle.oracle import COracle

pytestmark = pytest.mark.gpu

golhip = pytest.importorskip("golhip")

GOLHIP_EINVAL = -1
ANY = [0, 1, -1, 2, 1 << 40, -(1 << 40)]  # options that take value != 0

# key: (accepted, refused, default).  Both ends of every range and one step
# outside each; for the set-valued options also a value between two members.
OPTIONS = {
    # product options
    "wpl": ([0, 1, 2, 4], [-1, 3, 5], 0),
    "persistent": ([-1, 0, 1], [-2, 2], -1),
    "lds_band": ([-1, 0, 1], [-2, 2], -1),
    "skew": ([0, 1, 2], [-1, 3], 1),
    "timing": (ANY, [], 0),
    "persist_timeout_us": ([1, 60000000], [0, 60000001], 1000000),
    "force_halo": (ANY, [], 0),
    # A/B tuning knobs (GOLHIP_TUNING=1)
    "persist_depth": ([0, 32], [-1, 33], 0),
    "persist_waves": ([0, 4, 8, 16], [-1, 1, 6, 12, 17], 0),
    "dummy_rows": ([0, 128], [-1, 129], 0),
    "paired_bands": ([0, 1], [-1, 2], 1),
    "persist_half": ([0, 1], [-1, 2], 1),
    "persist_wg_tx": ([0, 16], [-1, 17], 0),
    "trace": (ANY, [], 0),
    "fill_skip": (ANY, [], 1),
    "skew_young": ([0, 10, 400], [-1, 1, 5, 9, 401], 0),
    "skew_hcap": ([-1, 256], [-2, 257], -1),
    "skew_prio": ([0, 1], [-1, 2], 0),
    "skew_half": ([-1, 1], [-2, 2], 0),
    "skew_tx": ([0, 2], [-1, 3], 0),
    "lds_depth": ([0, 64], [-1, 65], 0),
    "lds_waves": ([0, 8, 16], [-1, 4, 12, 17], 0),
    "lds_wg_cu": ([1, 2], [0, 3], 1),
    "lds_age": ([0, 25, 400], [-1, 12, 24, 401], 0),
    "lds_pre": ([0, 64], [-1, 65], 2),
    "lds_stride": ([0, 1], [-1, 2], 1),
    "lds_xcd": ([0, 1], [-1, 2], 1),
    "flip_overlap": ([0, 3], [-1, 4], 2),
    "skew_pairs": ([0, 7], [-1, 8], 5),
    # upper bound: the device's CU count (0: all of them)
    "cu_count": ([0, 1], [-1, 1 << 20], 0),
    # wrong results by design (GOLHIP_MEASUREMENT=1) and test hooks (GOLHIP_TEST_HOOKS=1)
    "halo_skip": (ANY, [], 0),
    "flip_debug": ([0, 7], [-1, 8], 0),
    "resident_fault": ([0, 2], [-1, 3], 0),
    "resident_max_turns": ([1, 1 << 30], [0, (1 << 30) + 1], 1 << 30),
}


@pytest.fixture(scope="module")
def coracle():
    return COracle()


def refused(call, *args):
    with pytest.raises(golhip.GolHipError) as e:
        call(*args)
    assert e.value.code == GOLHIP_EINVAL, (args, str(e.value))


def test_option_bounds(monkeypatch):
    for env in ("GOLHIP_TUNING", "GOLHIP_MEASUREMENT", "GOLHIP_TEST_HOOKS"):
        monkeypatch.setenv(env, "1")
    with golhip.Board(64, 64) as b:
        for key, (ok, bad, default) in OPTIONS.items():
            for v in ok:
                b.set_option(key, v)
            for v in bad:
                refused(b.set_option, key, v)
            b.set_option(key, default)
        for v in (1, 32):
            b.set_tb_depth(v)
        for v in (0, 33, -1):
            refused(b.set_tb_depth, v)
        b.set_tb_depth(20)
        for v in (0, 1, (1 << 31) - 1):
            b.set_rows_per_wave(v)
        refused(b.set_rows_per_wave, -1)
        b.set_rows_per_wave(0)
        refused(b.set_option, "no_such_option", 0)
        refused(b.set_option, "", 0)
        lib = golhip.load()
        assert lib.golhip_set_option(b.handle, None, 0) == GOLHIP_EINVAL
        assert lib.golhip_set_option(None, b"wpl", 0) == GOLHIP_EINVAL


# golhip_perf fields that golhip_perf_reset zeroes (cell_updates and alg_bytes
# are derived from them), and those it leaves alone.
RESET = ["step_launches", "step_turns", "step_kernel_ms", "persist_launches", "persist_turns", "persist_kernel_ms",
         "cell_updates", "alg_bytes", "halo_bytes", "flip_launches", "flip_entries", "flip_kernel_ms",
         "skew_launches", "halo_exchanges", "halo_ms", "skew_half_launches", "lds_launches", "pair_launches",
         "pair_turns", "flip_resident_launches", "view_frames", "view_kernel_ms"]
KEPT = ["turns", "persist_fallbacks", "flip_fallbacks"]
PAIRS = {"step": ["step_launches", "step_kernel_ms"],
         "persist": ["persist_launches", "persist_kernel_ms"],
         "flip": ["flip_launches", "flip_kernel_ms"],
         "halo": ["halo_exchanges", "halo_ms", "halo_bytes"]}

W = H = 256


def check_path(b, p0, moved):
    """Every field of the `moved` pairs is positive, the other pairs are as in p0."""
    p = b.perf()
    for name, fields in PAIRS.items():
        for f in fields:
            if name in moved:
                assert p[f] > 0, (f, p)
            else:
                assert p[f] == p0[f], (f, p0, p)
    return p


def check_reset(b, kept):
    p = b.perf()
    assert {k: p[k] for k in KEPT} == kept, p
    b.perf_reset()
    p = b.perf()
    assert {k: p[k] for k in RESET} == {k: 0 for k in RESET}, p
    assert {k: p[k] for k in KEPT} == kept, p


def test_timing_per_launch(coracle):
    board = coracle.fill_random(W, H, 0x5EED0081)
    with golhip.Board(W, H, timing=True) as b:
        b.set_option("persistent", 0)
        b.set_option("lds_band", 0)
        b.load_bytes(board)
        p0 = b.perf()
        b.step(10)
        p = check_path(b, p0, {"step"})
        assert p["step_turns"] == 10
        assert np.array_equal(b.snapshot_bytes(), coracle.run(board, 10))
        check_reset(b, {"turns": 10, "persist_fallbacks": 0, "flip_fallbacks": 0})


@pytest.mark.usefixtures("test_hooks")
def test_timing_resident(coracle):
    board = coracle.fill_random(W, H, 0x5EED0082)
    with golhip.Board(W, H, timing=True) as b:
        b.set_option("persistent", 1)
        b.set_option("lds_band", 1)
        b.load_bytes(board)
        p0 = b.perf()
        b.step(10)
        p = check_path(b, p0, {"persist"})
        assert p["persist_turns"] == 10 and p["lds_launches"] == 1
        assert np.array_equal(b.snapshot_bytes(), coracle.run(board, 10))
        # a resident launch abandoned (band 0 never reports): the step re-runs on
        # the per-launch kernels and the counters forget the abandoned launch
        b.set_option("resident_fault", 1)
        b.set_option("persist_timeout_us", 2000)
        b.step(30)
        q = check_path(b, p, {"step"})
        assert q["persist_fallbacks"] == 1 and q["step_turns"] == 30 and q["persist_turns"] == 10
        assert np.array_equal(b.snapshot_bytes(), coracle.run(board, 40))
        check_reset(b, {"turns": 40, "persist_fallbacks": 1, "flip_fallbacks": 0})


@pytest.mark.usefixtures("test_hooks")
def test_timing_flip_stream(coracle):
    board = coracle.fill_random(W, H, 0x5EED0083)
    with golhip.Board(W, H, timing=True) as b:
        b.load_bytes(board)
        p0 = b.perf()
        b.set_option("flip_debug", 4)  # one reported co-residency failure: the batch re-runs in ticket order
        ent, counts, done = b.flip_stream(6, cap=6 * W * H)
        assert done == 6 and int(counts.sum()) == len(ent)
        p = check_path(b, p0, {"flip"})
        assert p["flip_fallbacks"] == 1 and p["flip_entries"] == len(ent)
        assert np.array_equal(b.snapshot_bytes(), coracle.run(board, 6))
        check_reset(b, {"turns": 6, "persist_fallbacks": 0, "flip_fallbacks": 1})


def test_timing_one_rank_ring(coracle):
    board = coracle.fill_random(W, H, 0x5EED0084)
    with golhip.Board(W, H, timing=True) as b:
        b.comm_init(golhip.unique_id(), 1, 0)
        b.set_option("force_halo", 1)
        b.set_option("persistent", 0)
        b.load_bytes(board)
        p0 = b.perf()
        b.step(10)
        check_path(b, p0, {"halo", "step"})  # the exchanges feed per-launch kernels
        assert np.array_equal(b.snapshot_bytes(), coracle.run(board, 10))
        check_reset(b, {"turns": 10, "persist_fallbacks": 0, "flip_fallbacks": 0})
