"""The live view's cost (golhip_view_frame / golhip_view_stream).

    python scripts/bench_view.py [--out profiles/view/bench_view.json] [--quick]
    python scripts/bench_view.py --strips 8 [--out profiles/view/bench_view_strips.json] [--quick]

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
--strips n measures only the view across row strips (golhip_group_view_frame)
against the single-handle frame of the same run: the same board as one handle
and as n strips on the same device, both into page-locked memory, timed
alternately; once with the viewport at the origin (the H i / n strip
boundaries of these boards fall on pixel rows: every pixel row lies in one
strip) and once from row s / 2 (a pixel row straddles every boundary and the
y seam: the counts + resolve path).
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


def strips_rows(nstrips, quick):
    rows = []
    cases = [(5120, 5, golhip.VIEW_GRAY8)]
    if not quick:
        cases.append((65536, 64, golhip.VIEW_ARGB))
    for n, s, fmt in cases:
        cuts = [n * i // nstrips for i in range(nstrips + 1)]
        strips = []
        with golhip.Board(n, n, timing=True) as one:
            try:
                for r0, r1 in zip(cuts, cuts[1:]):
                    strips.append(golhip.Board(n, n, row0=r0, rows=r1 - r0, timing=True))
                    strips[-1].fill_random(SEED)
                one.fill_random(SEED)
                one.step(3)
                golhip.group_step(strips, 3)
                ow = n // s
                dt = np.uint8 if fmt == golhip.VIEW_GRAY8 else np.uint32
                out_one, out_strips = golhip.host_array((ow * ow,), dt), golhip.host_array((ow * ow,), dt)
                for y0 in (0, s // 2):
                    def whole():
                        one.view_frame(0, y0, s, fmt=fmt, out=out_one)

                    def group():
                        golhip.group_view_frame(strips, 0, y0, s, fmt=fmt, out=out_strips)

                    whole()
                    group()
                    same = bool(np.array_equal(out_one, out_strips))
                    for b in [one, *strips]:
                        b.perf_reset()
                    t_one, _ = timed(whole)
                    t_grp, _ = timed(group)
                    t_one2, _ = timed(whole)
                    t_grp2, reps = timed(group)
                    to, tg = min(t_one, t_one2), min(t_grp, t_grp2)
                    p1, ps = one.perf(), [st.perf() for st in strips]
                    rows.append({"board": f"{n}x{n}", "scale": s, "format": "GRAY8" if fmt else "ARGB8888",
                                 "frame": f"{ow}x{ow}", "dest": "pinned", "strips": nstrips, "y0": y0,
                                 "pixel_rows_across_strips": sum(1 for c in cuts[1:] if (c - y0) % s),
                                 "equals_single_handle_frame": same,
                                 "single_wall_us_per_frame": round(to * 1e6, 2),
                                 "strips_wall_us_per_frame": round(tg * 1e6, 2), "strips_over_single": round(tg / to, 3),
                                 "single_kernel_us_per_frame": round(p1["view_kernel_ms"] / p1["view_frames"] * 1e3, 2),
                                 # the strips' kernels run side by side: their sum is device work, not elapsed time
                                 "strips_kernel_us_per_frame_summed": round(
                                     sum(p["view_kernel_ms"] for p in ps) / ps[0]["view_frames"] * 1e3, 2),
                                 "strips_kernel_us_per_frame_slowest_strip": round(
                                     max(p["view_kernel_ms"] / p["view_frames"] for p in ps) * 1e3, 2),
                                 "frames_timed": reps})
                    print(json.dumps(rows[-1]), flush=True)
            finally:
                for st in strips:
                    st.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="skip the 65536^2 boards")
    ap.add_argument("--strips", type=int, default=0, help="only the view across this many row strips (>= 2)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "view", "bench_view_strips.json" if a.strips else "bench_view.json")
    if golhip.device_count() < 1:
        raise SystemExit("bench_view: no HIP device")
    if a.strips:
        if a.strips < 2:
            raise SystemExit("bench_view: --strips needs at least 2")
        res = {"bench": "view_strips", "strips": a.strips, "frames": strips_rows(a.strips, a.quick)}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"bench": "view_strips", "out": a.out}))
        return
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
