#!/usr/bin/env python3
"""The bounded plane (K15, csrc/gol_rule_plane.hip) against the torus (K11,
csrc/gol_rule.hip) on HighLife: fill_random, 256 turns a
golhip_step call, timed as scripts/bench_rules.py times its calls (a
host-clock window around whole calls that ends in a synchronise; one warm-up
call, three windows, the median).

  plane_highlife   B36/S23 on a plane handle: K15, 16 turns a launch at any width
  torus_highlife   B36/S23 on a torus handle: K11 (16385^2: the padded torus)

  (a) plane_highlife at 16384^2 and 65536^2 against the parent commit's torus_highlife
  (b) plane_highlife at 16385^2 against the parent's padded torus at 16385^2
  (c) torus_highlife on this commit against the parent's

The parent's rows belong to the commit before K15: --pkg names a built checkout
of that commit (its golhip package and library are imported instead of this
tree's) and --variants picks what runs, so the two libraries are measured in
the same session into two files.

    python scripts/bench_plane.py [--out profiles/plane/bench_plane.json]
    python scripts/bench_plane.py --pkg <parent checkout> --variants torus_highlife \\
        --out profiles/plane/bench_plane_parent.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = next((os.path.abspath(sys.argv[i + 1]) for i, a in enumerate(sys.argv[:-1]) if a == "--pkg"), ROOT)
sys.path[:0] = [PKG, os.path.join(PKG, "game-of-life-distributed_amd")]

import golhip  # noqa: E402

SIZES = [16384, 65536, 16385]
TURNS = 256
REPS = 3
WINDOW_S = 0.15
VARIANTS = ["plane_highlife", "torus_highlife"]
PERF_KEYS = ("step_launches", "step_turns", "rule_launches", "pad_launches", "skew_launches", "persist_launches",
             "kernel_variant", "words_per_lane", "tb_depth", "rows_per_wave")


def configure(b, variant):
    b.set_rule("B36/S23")
    if variant == "plane_highlife":
        b.set_topology(golhip.TOPOLOGY_PLANE)


def window(b, calls):
    b.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        b.step(TURNS)
    b.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane", "bench_plane.json"))
    ap.add_argument("--pkg", default=ROOT, help="a built checkout whose golhip package runs (the parent commit's)")
    ap.add_argument("--variants", default=",".join(VARIANTS))
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    args = ap.parse_args()
    lib = golhip.load()
    rows = []
    for n in [int(s) for s in args.sizes.split(",")]:
        for variant in args.variants.split(","):
            with golhip.Board(n, n) as b:
                configure(b, variant)
                b.fill_random(2024)
                window(b, 1)
                calls = max(1, min(200, int(WINDOW_S / max(window(b, 1), 1e-6))))
                secs = sorted(window(b, calls) / (calls * TURNS) for _ in range(REPS))
                per_turn = secs[REPS // 2]
                p = b.perf()
                row = {"size": n, "variant": variant, "turns_per_call": TURNS, "calls": calls,
                       "us_per_turn": round(per_turn * 1e6, 3), "tcups": round(n * n / per_turn / 1e12, 3),
                       "tcups_min_max": [round(n * n / s / 1e12, 3) for s in (secs[-1], secs[0])],
                       "perf": {k: p[k] for k in PERF_KEYS if k in p}}
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"version": lib.golhip_version().decode(), "parent_checkout": PKG != ROOT,
                   "turns_per_call": TURNS, "reps": REPS, "window_s": WINDOW_S, "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
