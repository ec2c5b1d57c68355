"""What the read half of the pattern calls costs (golhip_alive_box,
golhip_extract_bits, golhip_save_rle).

    python scripts/bench_extract.py [--out profiles/extract/bench_extract.json] [--boards 16384 65536] [--reps 7]

In one process, per board size, on a fill_random soup and on a blank board with
one Gosper glider gun stamped at (100, 100) and run for 1000 turns:

1. alive_box (K13: one pass over the board, two small copies, the intervals on
   the host) against a forced recount by alive_count (K2, which also reads the
   board once; a no-op stamp before each repetition drops the kept count);
2. a 1024 x 1024 extract (K12) at a corner 5 off a word boundary against
   snapshot_rows of the same 1024 rows (whole rows, converted in place and back);
3. the gun only: save_rle of the alive box against the parent commit's only
   route to the same file: snapshot_bits of the whole board, the box found and
   cut on the host with numpy, rle_format_np -- each part timed; both texts are
   parsed and compared.

Every call is warmed once and repeated `reps` times (the parent route 3 times);
the JSON keeps every repetition, the median and the spread.  The timer is the
host's wall clock around calls that end in a stream synchronise.  Needs a GPU:
without one it fails."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "game-of-life-distributed_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import golhip  # noqa: E402

SEED = 0xE87AC7
GUN = ("x = 36, y = 9, rule = B3/S23\n24bo$22bobo$12b2o6b2o12b2o$11bo3bo4b2o12b2o$2o8bo5bo3b2o$2o8bo3bob2o4bobo$"
       "10bo5bo7bo$11bo3bo$12b2o!\n")
GUN_AT, GUN_TURNS = (100, 100), 1000


def timed(fn, reps, before=None):
    out = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def parent_route(b, n):
    """snapshot_bits, the box on the host, rle_format_np: (text, ms of each part)."""
    t0 = time.perf_counter()
    words = b.snapshot_bits()
    t1 = time.perf_counter()
    rows = np.flatnonzero(words.any(axis=1))
    cols = np.flatnonzero(words.any(axis=0))
    # (no seam logic: the gun's box does not wrap, which favours this route)
    cut = words[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
    bits = np.unpackbits(cut.astype("<u4").view(np.uint8).reshape(cut.shape[0], -1), axis=1, bitorder="little").astype(bool)
    xs = np.flatnonzero(bits.any(axis=0))
    bits = bits[:, xs[0]:xs[-1] + 1]
    t2 = time.perf_counter()
    text = golhip.rle_format_np(bits)
    t3 = time.perf_counter()
    return text, ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3)


def bench_board(b, n, what, reps, tmp):
    zero = np.zeros((1, 1), dtype=bool)
    row = {"board": f"{n}x{n}", "content": what, "words_per_lane": b.perf()["words_per_lane"], "turn": b.turn()}
    b.alive_box()
    row["alive_box"] = summary(timed(b.alive_box, reps))
    row["box"] = list(b.alive_box())
    drop = lambda: b.stamp(zero, 0, 0, golhip.STAMP_OR)  # noqa: E731  (changes nothing; the kept count goes)
    drop()
    b.alive_count()
    row["alive_count_recount"] = summary(timed(b.alive_count, reps, before=drop))
    row["alive_box_over_recount"] = round(row["alive_box"]["median_ms"] / row["alive_count_recount"]["median_ms"], 2)
    x0, y0 = (n // 2 + 5, n // 3) if what == "soup" else (GUN_AT[0] - 27, GUN_AT[1] - 40)
    ext = lambda: b.extract(x0, y0, 1024, 1024)  # noqa: E731
    ext()
    row["extract_1024"] = summary(timed(ext, reps))
    rows = lambda: b.snapshot_rows(y0, 1024)  # noqa: E731
    rows()
    row["snapshot_rows_1024"] = summary(timed(rows, reps))
    if what == "gun":
        path = os.path.join(tmp, f"gun{n}.rle")
        save = lambda: golhip.save_rle(b, path)  # noqa: E731
        info = save()
        row["save_rle"] = summary(timed(save, reps))
        row["save_rle"]["info"] = info
        text, _ = parent_route(b, n)  # warm
        same = np.array_equal(golhip.rle_parse_np(text), golhip.pattern_read(path))
        parts = [parent_route(b, n)[1] for _ in range(3)]
        row["parent_route"] = {"equals_save_rle": bool(same), "snapshot_bits": summary([p[0] for p in parts]),
                               "host_box": summary([p[1] for p in parts]), "rle_format_np": summary([p[2] for p in parts]),
                               "total": summary([sum(p) for p in parts])}
        row["parent_over_save_rle"] = round(row["parent_route"]["total"]["median_ms"] / row["save_rle"]["median_ms"], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract", "bench_extract.json"))
    ap.add_argument("--boards", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    if golhip.device_count() < 1:
        raise SystemExit("bench_extract: no HIP device")
    res = {"bench": "extract", "reps": a.reps, "timer": "host wall clock around calls that end in a stream synchronise",
           "rows": []}
    with tempfile.TemporaryDirectory() as tmp:
        gun = os.path.join(tmp, "gun.rle")
        with open(gun, "w") as f:
            f.write(GUN)
        for n in a.boards:
            with golhip.Board(n, n) as b:
                b.fill_random(SEED)
                b.step(8)  # the layout the board is stepped in
                b.sync()
                row = bench_board(b, n, "soup", a.reps, tmp)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                b.clear()
                golhip.stamp_file(b, gun, *GUN_AT)
                b.step(GUN_TURNS)
                b.sync()
                row = bench_board(b, n, "gun", a.reps, tmp)
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"bench": "extract", "out": a.out}))


if __name__ == "__main__":
    main()
