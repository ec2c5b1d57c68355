#!/usr/bin/env python3
"""The CellFlipped stream of a Life-like rule: golhip_set_rule_flips 0 (a step
on K11, a three-pass compaction and two host synchronisations a turn, the
parent commit's only path) against 1 (K14, the fused turn + list kernel,
csrc/gol_rule_flip.hip), DESIGN.md §5.24 and §7.10.

turns/s of golhip_flip_stream on fill_random boards of 512^2, 5120^2 and
5121^2 (W % 32 != 0: the kernels close the row seam themselves), HighLife
(static policy) and B3578/S1246 (dynamic policy), into pageable and into
golhip_host_alloc memory, as (x, y) pairs and as cell indices.  Both modes run
on one handle in one process, alternating; every window starts from the same
board (fill_random, then SETTLE turns on the step kernel, so the lists are
those of a settled soup, not of white noise) and streams the same turns, so
the two modes deliver the same entries.  A host-clock window around whole
calls; one warm-up window a mode, then REPS windows a mode, the median.

    python scripts/bench_rule_events.py [--out profiles/rule_events/bench_rule_events.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "game-of-life-distributed_amd")]

import golhip  # noqa: E402

SHAPES = [(512, 512), (5120, 5120), (5121, 5121)]
RULES = [("highlife_static", "B36/S23"), ("b3578_s1246_dynamic", "B3578/S1246")]
SETTLE = 64
REPS = 3
# turns a call and calls a window by board width: ~0.1 s a window on the slower mode
BATCH = {512: (64, 4), 5120: (8, 1), 5121: (8, 1)}
PERF_KEYS = ("flip_launches", "flip_entries", "flip_fallbacks", "rule_launches", "step_launches")


def window(b, mode, turns, calls, fmt, out):
    """One window: the same board, then `calls` flip_stream calls of `turns` turns; (seconds, turns, entries)."""
    b.set_rule_flips(mode)
    b.fill_random(2024)
    b.step(SETTLE)
    b.sync()
    done_all, n_all = 0, 0
    t0 = time.perf_counter()
    for _ in range(calls):
        ent, counts, done = b.flip_stream(turns, out.shape[0], fmt, out=out)
        done_all += done
        n_all += len(ent)
    b.sync()
    return time.perf_counter() - t0, done_all, n_all


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rule_events", "bench_rule_events.json"))
    ap.add_argument("--shapes", default=",".join(f"{w}x{h}" for w, h in SHAPES))
    args = ap.parse_args()
    lib = golhip.load()
    rows = []
    for W, H in [tuple(map(int, s.split("x"))) for s in args.shapes.split(",")]:
        turns, calls = BATCH.get(W, (8, 1))
        cap = turns * W * H // 4  # a settled soup flips under a tenth of its cells a turn
        for name, rule in RULES:
            for mem in ("pageable", "pinned"):
                for fmt_name, fmt in (("xy", golhip.FLIPS_XY), ("index", golhip.FLIPS_INDEX)):
                    shape, dt = ((cap, 2), np.int32) if fmt == golhip.FLIPS_XY else ((cap,), np.uint32)
                    out = golhip.host_array(shape, dt) if mem == "pinned" else np.empty(shape, dt)
                    with golhip.Board(W, H) as b:
                        b.set_rule(rule)
                        secs, seen, perf = {0: [], 1: []}, {}, {}
                        for mode in (0, 1):  # warm-up: buffers, occupancy queries
                            window(b, mode, turns, calls, fmt, out)
                        for rep in range(REPS):
                            for mode in ((0, 1) if rep % 2 == 0 else (1, 0)):
                                b.perf_reset()
                                s, done, n = window(b, mode, turns, calls, fmt, out)
                                secs[mode].append(s / max(done, 1))
                                seen.setdefault(mode, (done, n))
                                assert seen[mode] == (done, n), (mode, seen[mode], done, n)
                                p = b.perf()
                                perf[mode] = {k: p[k] for k in PERF_KEYS if k in p}
                        med = {m: sorted(secs[m])[REPS // 2] for m in (0, 1)}
                        row = {"shape": f"{W}x{H}", "rule": rule, "policy": name, "memory": mem, "format": fmt_name,
                               "turns_per_window": seen[0][0], "same_turns_and_entries": seen[0] == seen[1],
                               "entries_per_turn": round(seen[0][1] / max(seen[0][0], 1)),
                               "mode0_turns_per_s": round(1 / med[0], 1), "mode1_turns_per_s": round(1 / med[1], 1),
                               "mode0_min_max": [round(1 / max(secs[0]), 1), round(1 / min(secs[0]), 1)],
                               "mode1_min_max": [round(1 / max(secs[1]), 1), round(1 / min(secs[1]), 1)],
                               "mode1_over_mode0": round(med[0] / med[1], 2), "perf_mode0": perf[0], "perf_mode1": perf[1]}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                    del out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"version": lib.golhip_version().decode(), "settle_turns": SETTLE, "reps": REPS,
                   "batch_turns_calls_by_width": {str(k): v for k, v in BATCH.items()}, "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
