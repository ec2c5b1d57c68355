#!/usr/bin/env python3
"""The rule kernel (K11, csrc/gol_rule.hip) against Conway's kernels (DESIGN.md
§5.21): 16384^2 and 65536^2, fill_random, 256 turns a golhip_step call, timed
as scripts/bench_widths.py times its calls (a host-clock window around whole
calls that ends in a synchronise; one warm-up call, three repetitions, the
median).

  highlife_static    B36/S23 on K11's static policy (the plan a rule handle gets)
  highlife_dynamic   the same rule on the dynamic policy (test option rule_kernel 2)
  highlife_depth1    K11 one turn a launch (set_tb_depth(1)): the HBM-bound form
  conway_plain_k1    Conway on plain K1 (skew 0, persistent 0, wpl 1): the yardstick
  conway_shipped     Conway as a new handle plans it

The Conway variants are there for context and belong to the commit before
K11: --pkg names a built checkout of that commit (its golhip package and
library are imported instead of this tree's) and --variants picks what runs,
so the two libraries are measured in two runs into two files.

    GOLHIP_TEST_HOOKS=1 python scripts/bench_rules.py [--out profiles/rules/bench_rules.json]
    python scripts/bench_rules.py --pkg <parent checkout> --variants conway_plain_k1,conway_shipped \\
        --out profiles/rules/bench_rules_parent.json
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

SIZES = [16384, 65536]
TURNS = 256
REPS = 3
WINDOW_S = 0.15
VARIANTS = ["highlife_static", "highlife_dynamic", "highlife_depth1", "conway_plain_k1", "conway_shipped"]
PERF_KEYS = ("step_launches", "step_turns", "rule_launches", "skew_launches", "pair_launches", "persist_launches",
             "kernel_variant", "words_per_lane", "tb_depth", "rows_per_wave")
# one turn a launch reads and writes every cell once: 0.25 bytes a cell-turn
# against the MI355X's 8 TB/s of HBM3E
HBM_BOUND_CELLS_PER_S = 8e12 / 0.25


def configure(b, variant):
    if variant.startswith("highlife"):
        b.set_rule("B36/S23")
    if variant == "highlife_dynamic":
        b.set_option("rule_kernel", 2)
    if variant == "highlife_depth1":
        b.set_tb_depth(1)
    if variant == "conway_plain_k1":
        for k, v in (("skew", 0), ("persistent", 0), ("wpl", 1)):
            b.set_option(k, v)


def window(b, calls):
    b.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        b.step(TURNS)
    b.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rules", "bench_rules.json"))
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
                       "over_hbm_bound_of_one_turn_launches": round(n * n / per_turn / HBM_BOUND_CELLS_PER_S, 3),
                       "perf": {k: p[k] for k in PERF_KEYS if k in p}}
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"version": lib.golhip_version().decode(), "parent_checkout": PKG != ROOT,
                   "turns_per_call": TURNS, "reps": REPS, "window_s": WINDOW_S,
                   "hbm_bound_cells_per_s": HBM_BOUND_CELLS_PER_S, "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
