#!/usr/bin/env python3
"""Boards whose width is no multiple of 32: the any-width kernel (K1g, pad step
mode 0) against the padded torus (mode 1) and against the plain Wp x H board on
per-launch kernels, the ceiling the padding can reach.

For each board and each n (turns a golhip_step call) the three variants run
three repetitions each, alternating, after one warm-up call a variant.  A
repetition is a host-clock window around `calls` calls that ends in a
synchronise.  The automatic rule of golhip_set_pad_step takes the padded path
for the (cells, n) region where mode 1 beat mode 0 in every repetition; this
script prints that region and writes every window to the JSON.

    python scripts/bench_widths.py [--out profiles/widths/bench_widths.json] [--quick]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "game-of-life-distributed_amd")]

import golhip  # noqa: E402

BOARDS = [(100, 100), (1000, 1000), (1920, 1080), (5000, 5000), (10001, 10001), (16385, 16385)]
TURNS = [1, 2, 4, 8, 16, 64, 256]
REPS = 3
WINDOW_S = 0.15  # a repetition runs whole calls for about this long (at least one)


def window(board, n, calls):
    board.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        board.step(n)
    board.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "widths", "bench_widths.json"))
    ap.add_argument("--quick", action="store_true", help="the two smallest boards and n in {1, 16}: a rehearsal")
    args = ap.parse_args()
    boards = BOARDS[:2] if args.quick else BOARDS
    turns = [1, 16] if args.quick else TURNS
    windows, summary = [], []
    for W, H in boards:
        wp = golhip.pad_plan_np(W)[0]
        variants = {}
        if W % 32 == 0:  # (1920 x 1080: the fast kernels take the width as it is; timed for the record)
            with golhip.Board(W, H) as b:
                b.fill_random(2024)
                for n in turns:
                    window(b, n, 1)
                    calls = max(1, min(2000, int(WINDOW_S / max(window(b, n, 1), 1e-6))))
                    secs = sorted(window(b, n, calls) / (calls * n) for _ in range(REPS))
                    row = {"W": W, "H": H, "cells": W * H, "n": n, "padded_torus_applies": False,
                           "us_per_turn": {"plain": round(secs[REPS // 2] * 1e6, 3)}}
                    summary.append(row)
                    print(json.dumps(row), flush=True)
            continue
        for name, width, mode in (("mode0", W, 0), ("mode1", W, 1), ("ceiling", wp, None)):
            b = golhip.Board(width, H)
            if mode is None:
                b.set_option("persistent", 0)
            else:
                b.set_pad_step(mode)
            b.fill_random(2024)
            variants[name] = b
        for n in turns:
            calls = {}
            for name, b in variants.items():  # warm-up: the code objects, the wide board, the plans of this n
                window(b, n, 1)
                calls[name] = max(1, min(2000, int(WINDOW_S / max(window(b, n, 1), 1e-6))))
            secs = {name: [] for name in variants}
            for rep in range(REPS):
                for name, b in variants.items():
                    s = window(b, n, calls[name])
                    per_turn = s / (calls[name] * n)
                    secs[name].append(per_turn)
                    windows.append({"W": W, "H": H, "n": n, "variant": name, "rep": rep, "calls": calls[name],
                                    "seconds": s, "us_per_turn": per_turn * 1e6,
                                    "cell_updates_per_s": W * H / per_turn})
            med = {name: sorted(v)[len(v) // 2] for name, v in secs.items()}
            row = {"W": W, "H": H, "Wp": wp, "cells": W * H, "n": n,
                   "us_per_turn": {k: round(v * 1e6, 3) for k, v in med.items()},
                   "mode1_beats_mode0_every_rep": max(secs["mode1"]) < min(secs["mode0"]),
                   "mode0_beats_mode1_every_rep": max(secs["mode0"]) < min(secs["mode1"]),
                   "speedup_mode1_over_mode0": round(med["mode0"] / med["mode1"], 3),
                   # the ceiling steps Wp x H cells: its time per turn against mode 1's
                   "mode1_rate_over_ceiling": round(med["ceiling"] / med["mode1"], 3)}
            summary.append(row)
            print(json.dumps(row), flush=True)
        p1 = variants["mode1"].perf()
        summary.append({"W": W, "H": H, "mode1_perf": {k: p1[k] for k in ("step_launches", "pad_launches", "skew_launches",
                                                                          "pair_launches", "kernel_variant")},
                        "ceiling_words_per_lane": variants["ceiling"].perf()["words_per_lane"]})
        for b in variants.values():
            b.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"boards": boards, "turns": turns, "reps": REPS, "window_s": WINDOW_S,
                   "version": golhip.load().golhip_version().decode(), "summary": summary, "windows": windows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
