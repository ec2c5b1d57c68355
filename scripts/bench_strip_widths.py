#!/usr/bin/env python3
"""Row strips of a board whose width is no multiple of 32: the any-width kernel
(K1g, golhip_group_set_pad_step mode 0) against padded strips (mode 1) and
against the same strips of a plain Wp-wide board on per-launch kernels, the
ceiling the padding can reach.  The method is
scripts/bench_widths.py's.

For each board, each number of in-process strips on device 0 and each n (turns
a golhip_group_step call) the three variants run three repetitions each,
alternating, after one warm-up call a variant.  A repetition is a host-clock
window around `calls` whole calls, each of which ends synchronised.  The
automatic rule of golhip_group_set_pad_step pads the (cells, n) region where
mode 1 beat mode 0 in every repetition; this script prints that and writes
every window to the JSON.

Every board runs in a child process of its own under a time limit (one host
thread each, one at a time); the parent never opens the GPU and stops at the
first child that fails.

    python scripts/bench_strip_widths.py [--out profiles/strip_widths/bench_strip_widths.json] [--quick]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "game-of-life-distributed_amd")]

# (100 x 100, gol.Run's smallest usual board, and n = 2, 4, 8 bound the rule from below)
BOARDS = [(100, 100), (1000, 1000), (5000, 5000), (10001, 10001), (16385, 16385)]
STRIPS = [2, 4, 8]
TURNS = [1, 2, 4, 8, 16, 256]
REPS = 3
WINDOW_S = 0.15   # a repetition runs whole calls for about this long (at least one)
BOARD_LIMIT_S = 240  # a child's time limit


def window(golhip, bs, n, calls):
    for b in bs:
        b.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        golhip.group_step(bs, n)  # (returns with every strip's stream synchronised)
    return time.perf_counter() - t0


def make_strips(golhip, width, H, k, mode):
    cuts = [H * i // k for i in range(k + 1)]
    bs = []
    for i, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        b = golhip.Board(width, H, row0=a, rows=e - a)
        if mode is None:
            b.set_option("persistent", 0)
        b.fill_random(2024 + i)
        bs.append(b)
    if mode is not None:
        golhip.group_set_pad_step(bs, mode)
    return bs


def run_board(W, H, strips, turns):
    import golhip

    wp = golhip.pad_plan_np(W)[0]
    windows, summary = [], []
    for k in strips:
        variants = {name: make_strips(golhip, width, H, k, mode)
                    for name, width, mode in (("mode0", W, 0), ("mode1", W, 1), ("ceiling", wp, None))}
        for n in turns:
            calls = {}
            for name, bs in variants.items():  # warm-up: the code objects, the wide strips, the plans of this n
                window(golhip, bs, n, 1)
                calls[name] = max(1, min(2000, int(WINDOW_S / max(window(golhip, bs, n, 1), 1e-6))))
            secs = {name: [] for name in variants}
            for rep in range(REPS):
                for name, bs in variants.items():
                    s = window(golhip, bs, n, calls[name])
                    per_turn = s / (calls[name] * n)
                    secs[name].append(per_turn)
                    windows.append({"W": W, "H": H, "strips": k, "n": n, "variant": name, "rep": rep,
                                    "calls": calls[name], "seconds": s, "us_per_turn": per_turn * 1e6,
                                    "cell_updates_per_s": W * H / per_turn})
            med = {name: sorted(v)[len(v) // 2] for name, v in secs.items()}
            row = {"W": W, "H": H, "Wp": wp, "cells": W * H, "strips": k, "n": n,
                   "us_per_turn": {name: round(v * 1e6, 3) for name, v in med.items()},
                   "mode1_beats_mode0_every_rep": max(secs["mode1"]) < min(secs["mode0"]),
                   "mode0_beats_mode1_every_rep": max(secs["mode0"]) < min(secs["mode1"]),
                   "speedup_mode1_over_mode0": round(med["mode0"] / med["mode1"], 3),
                   # the ceiling steps Wp x H cells: its time per turn against mode 1's
                   "mode1_rate_over_ceiling": round(med["ceiling"] / med["mode1"], 3)}
            summary.append(row)
            print(json.dumps(row), flush=True)
        p1 = variants["mode1"][0].perf()
        summary.append({"W": W, "H": H, "strips": k,
                        "mode1_perf": {key: p1[key] for key in ("step_launches", "pad_launches", "skew_launches",
                                                                "pair_launches", "kernel_variant", "halo_bytes")},
                        "ceiling_words_per_lane": variants["ceiling"][0].perf()["words_per_lane"]})
        for bs in variants.values():
            for b in bs:
                b.close()
    return {"summary": summary, "windows": windows, "version": golhip.load().golhip_version().decode()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strip_widths", "bench_strip_widths.json"))
    ap.add_argument("--quick", action="store_true", help="1000 x 1000, 2 strips, n in {1, 16}: a rehearsal")
    ap.add_argument("--board", help="(child) W,H: run this board alone and print its JSON as the last line")
    args = ap.parse_args()
    strips = STRIPS[:1] if args.quick else STRIPS
    turns = [1, 16] if args.quick else TURNS
    if args.board:
        W, H = (int(x) for x in args.board.split(","))
        print(json.dumps(run_board(W, H, strips, turns)), flush=True)
        return 0
    boards = BOARDS[1:2] if args.quick else BOARDS
    summary, windows, version = [], [], ""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for W, H in boards:
        cmd = [sys.executable, os.path.abspath(__file__), "--board", f"{W},{H}"] + (["--quick"] if args.quick else [])
        try:
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=BOARD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{W} x {H}: no result in {BOARD_LIMIT_S} s; stopping", flush=True)
            return 1
        lines = r.stdout.strip().splitlines()
        if r.returncode != 0 or not lines:
            print(f"{W} x {H}: the child ended with {r.returncode}; stopping", flush=True)
            return 1
        for line in lines[:-1]:
            print(line, flush=True)
        res = json.loads(lines[-1])
        summary += res["summary"]
        windows += res["windows"]
        version = res["version"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"boards": boards, "strips": strips, "turns": turns, "reps": REPS, "window_s": WINDOW_S,
                   "version": version, "summary": summary, "windows": windows}, f, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
