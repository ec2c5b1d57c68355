"""The live view's cost (golhip_view_frame / golhip_view_stream).

    python scripts/bench_view.py [--out profiles/view/bench_view.json] [--quick]

Timing follows bench.py: a warm-up call, then a host clock around calls that
each end in a device synchronise, for at least a second per window.  Kernel
time is the library's own (GOLHIP_FLAG_TIMING events, perf view_kernel_ms).

1. frame time and the board-read rate it implies, with the share of the bound
   (the least time the hardware could take over the kernel time; the bound
   is named per row);
2. the view's overhead: golhip_view_stream turns/s at every 1 / 16 / 64
   against the same turns through golhip_step alone, alternately;
3. what showed a running board before: golhip_flip_stream (indices into
   page-locked memory) on 5120^2, and golhip_snapshot_bytes plus a numpy block
   sum for one look at 65536^2.
Needs a GPU: without one it fails."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "game-of-life-distributed_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import golhip  # noqa: E402

# MI355X: HBM3E as a float4 copy measures it, the Infinity Cache's size and
# gathered-read rate, the host link's spec
HBM_BPS = 6.29e12
MALL_BYTES = 256 << 20
MALL_BPS = 8.6e12
LINK_SPEC_BPS = 63e9
SEED = 0xB0A2D


def timed(run, seconds=1.0):
    run()  # warm
    reps, t0 = 0, time.perf_counter()
    while True:
        run()
        reps += 1
        if time.perf_counter() - t0 > seconds:
            break
    return (time.perf_counter() - t0) / reps, reps


def frame_rows(link_bps, quick):
    rows = []
    cases = [(512, 1, golhip.VIEW_ARGB, ["pinned"]),
             (5120, 5, golhip.VIEW_GRAY8, ["pinned"]),
             (5120, 5, golhip.VIEW_ARGB, ["pinned"])]
    if not quick:
        cases.append((65536, 64, golhip.VIEW_ARGB, ["pinned", "pageable"]))
    for n, s, fmt, dests in cases:
        with golhip.Board(n, n, timing=True) as b:
            b.fill_random(SEED)
            b.step(3)
            ow = n // s
            dt = np.uint8 if fmt == golhip.VIEW_GRAY8 else np.uint32
            for dest in dests:
                out = golhip.host_array((ow * ow,), dt) if dest == "pinned" else np.empty(ow * ow, dtype=dt)
                b.view_frame(scale=s, fmt=fmt, out=out)
                b.perf_reset()
                wall, reps = timed(lambda: b.view_frame(scale=s, fmt=fmt, out=out))
                p = b.perf()
                kern = p["view_kernel_ms"] / p["view_frames"] * 1e-3
                board_bytes = n * (n // 32) * 4
                frame_bytes = ow * ow * np.dtype(dt).itemsize
                # the least time: the board from HBM (or the Infinity Cache when it fits),
                # the frame over the host link when the kernel writes it there
                t_board = board_bytes / (MALL_BPS if board_bytes <= MALL_BYTES else HBM_BPS)
                t_frame = frame_bytes / link_bps if dest == "pinned" else frame_bytes / HBM_BPS
                bound = max(t_board, t_frame)
                name = ("host link (measured kernel-write rate)" if t_frame >= t_board and dest == "pinned"
                        else "Infinity Cache" if board_bytes <= MALL_BYTES else "HBM")
                rows.append({"board": f"{n}x{n}", "scale": s, "format": "GRAY8" if fmt else "ARGB8888",
                             "frame": f"{ow}x{ow}", "dest": dest, "words_per_lane": p["words_per_lane"],
                             "board_bytes": board_bytes, "frame_bytes": frame_bytes,
                             "wall_us_per_frame": round(wall * 1e6, 2), "frames_timed": reps,
                             "kernel_us_per_frame": round(kern * 1e6, 2),
                             "board_read_GBps_kernel": round(board_bytes / kern / 1e9, 1),
                             "bound": name, "bound_us": round(bound * 1e6, 2),
                             "share_of_bound_kernel": round(bound / kern, 3)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def overhead_rows(quick):
    rows = []
    for n, s in ([(5120, 5)] if quick else [(5120, 5), (65536, 64)]):
        with golhip.Board(n, n) as b:
            b.fill_random(SEED)
            ow = n // s
            out = golhip.host_array((16, ow, ow), np.uint32)
            for every in (1, 16, 64):
                turns = 16 * every

                def stepped():
                    b.step(turns)
                    b.sync()

                def viewed():
                    b.view_stream(turns, every, scale=s, out=out)

                t_step, _ = timed(stepped)
                t_view, _ = timed(viewed)
                t_step2, _ = timed(stepped)
                t_view2, _ = timed(viewed)
                ts, tv = min(t_step, t_step2), min(t_view, t_view2)
                rows.append({"board": f"{n}x{n}", "scale": s, "format": "ARGB8888", "every": every,
                             "turns_per_call": turns, "step_turns_per_s": round(turns / ts, 1),
                             "view_turns_per_s": round(turns / tv, 1), "view_over_step": round(ts / tv, 4),
                             "extra_us_per_frame": round((tv - ts) / 16 * 1e6, 2)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def parent_rows(quick):
    out = {}
    with golhip.Board(5120, 5120) as b:
        b.fill_random(SEED)
        cap = 48 << 20
        buf = golhip.host_array((cap,), np.uint32)
        turns = entries = 0
        b.flip_stream(8, cap, golhip.FLIPS_INDEX, out=buf)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:
            e, _, done = b.flip_stream(8, cap, golhip.FLIPS_INDEX, out=buf)
            turns += done
            entries += len(e)
        dt = time.perf_counter() - t0
        out["flip_stream_5120"] = {"turns_per_s": round(turns / dt, 1), "entries_per_turn": round(entries / turns),
                                   "turns": turns, "note": "fresh random board, uint32 indices into page-locked memory"}
        print(json.dumps(out["flip_stream_5120"]), flush=True)
    if not quick:
        n, s = 65536, 64
        with golhip.Board(n, n) as b:
            b.fill_random(SEED)
            b.step(3)
            t0 = time.perf_counter()
            snap = b.snapshot_bytes()
            t1 = time.perf_counter()
            cnt = (snap.reshape(n // s, s, n // s, s) >> 7).sum(axis=(1, 3), dtype=np.uint32)
            t2 = time.perf_counter()
            frame, _ = b.view_frame(scale=s, fmt=golhip.VIEW_GRAY8)
            same = bool(np.array_equal(frame, ((255 * cnt.astype(np.int64) + s * s - 1) // (s * s)).astype(np.uint8)))
            out["snapshot_look_65536"] = {"snapshot_bytes_s": round(t1 - t0, 3), "numpy_block_sum_s": round(t2 - t1, 3),
                                          "bytes_copied": n * n, "equals_view_frame": same}
            print(json.dumps(out["snapshot_look_65536"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view", "bench_view.json"))
    ap.add_argument("--quick", action="store_true", help="skip the 65536^2 boards")
    a = ap.parse_args()
    if golhip.device_count() < 1:
        raise SystemExit("bench_view: no HIP device")
    link = golhip.host_link_probe(0, 64 << 20, 5)
    link_bps = link["kernel_write_GBps"] * 1e9
    res = {"bench": "view", "host_link_probe": link,
           "bounds": {"hbm_GBps": HBM_BPS / 1e9, "infinity_cache_GBps": MALL_BPS / 1e9,
                      "host_link_spec_GBps": LINK_SPEC_BPS / 1e9, "host_link_kernel_write_GBps": link["kernel_write_GBps"]},
           "frames": frame_rows(link_bps, a.quick), "overhead": overhead_rows(a.quick), "before": parent_rows(a.quick)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"bench": "view", "out": a.out}))


if __name__ == "__main__":
    main()
