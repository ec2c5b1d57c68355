"""The CellFlipped stream on boards whose width is no multiple of 32
(DESIGN.md §5.5): turns/s of golhip_flip_stream and golhip_group_flip_stream,
cell indices (FLIPS_INDEX), into a golhip_host_alloc buffer ("pinned") and into
a pageable numpy buffer ("pageable").

Shapes: 1000^2, 5000^2, 5001 x 4999 and 16 x 16 on one handle; 1000^2 and
5000^2 on 4 row strips of one device (the group stream); 1024^2 and 5024^2,
the nearest boards whose width is a multiple of 32, as the ceiling; and, with
--regress, the 5120^2 stream_index_pinned leg of scripts/bench_events.py (same
seed, same 2064 turns before, same 200 turns, same 32 M-entry buffer).

Method (that of scripts/bench_events.py --strips): every leg starts from the
same state (fill_random(SEED), then PRE turns with events off), runs the same
turns in calls of as many turns as the 32 M-entry buffer holds, and is timed
with the host clock around the engine calls alone, which end synchronised.
After a 20-turn warm-up of each leg, three alternating repetitions, each
preceded by 20 untimed turns from the same state (so the stream's launch
estimate, the last batch's largest list, is that of the state the timed run
starts from and not of the end of the leg before).  The flip
totals and index sums of all legs of a shape must agree; they are summed
outside the timed calls.  One JSON object (--out FILE, else stdout).

The script uses only calls that exist before and after the change it measures:
run it on both builds (GOLHIP_LIB selects the library) with --label naming the
build.  --reps N: repetitions (3).  --only WxHxN: one shape.
--summarise DIR: no run; the turns/s of the <label>_<i>.json files under DIR
side by side (builds alternated a process at a time, one repetition each).
"""
import json
import os
import sys
import time

import numpy as np


def summarise(d):
    """The runs of <label>_<i>.json files under d side by side, per shape and leg."""
    out = {}
    for f in sorted(os.listdir(d)):
        stem = f[:-5].rsplit("_", 1)
        if not f.endswith(".json") or len(stem) != 2 or not stem[1].isdigit():
            continue
        with open(os.path.join(d, f)) as fh:
            j = json.load(fh)
        for r in j["shapes"] + ([j["regress_5120"]] if "regress_5120" in j else []):
            key = "%dx%d" % tuple(r["board"]) + (" x %d strips" % r["strips"] if r["strips"] > 1 else "") + \
                (" (%s)" % r["leg"] if "leg" in r else "")
            rec = out.setdefault(key, {"turns": r["turns"], "from_turn": r["from_turn"], "totals": [], "legs": {}})
            for leg, runs in r["runs"].items():
                for x in runs:
                    rec["legs"].setdefault(leg, {}).setdefault(j["label"], []).append(round(x["turns_per_s"], 1))
                    rec["totals"].append([x["flips"], x["index_sum"]])
    for rec in out.values():
        rec["same_lists_in_every_run"] = all(t == rec["totals"][0] for t in rec["totals"])
        rec["flips_per_turn"] = round(rec["totals"][0][0] / rec["turns"])
        del rec["totals"]
        for leg in rec["legs"].values():
            if "new" in leg and "parent" in leg:
                leg["new_over_parent"] = [round(min(leg["new"]) / max(leg["parent"]), 2),
                                          round(max(leg["new"]) / min(leg["parent"]), 2)]
    print(json.dumps(out, indent=1))


if "--summarise" in sys.argv:
    summarise(sys.argv[sys.argv.index("--summarise") + 1])
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "game-of-life-distributed_amd")]
import golhip  # noqa: E402

SEED = 0x5EED0005
PRE = 512
CAP = 32 << 20
# (W, H, strips, timed turns)
SHAPES = [(1000, 1000, 1, 2000), (5000, 5000, 1, 300), (5001, 4999, 1, 300), (16, 16, 1, 5000),
          (1000, 1000, 4, 2000), (5000, 5000, 4, 300),
          (1024, 1024, 1, 2000), (5024, 5024, 1, 300)]


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def stream(call, turns):
    """(flips, index sum, calls, seconds of the engine calls)."""
    done = flips = calls = digest = 0
    secs = 0.0
    while done < turns:
        t0 = time.perf_counter()
        ent, counts, k = call(turns - done)
        secs += time.perf_counter() - t0
        done, flips, calls = done + k, flips + len(ent), calls + 1
        digest += int(ent.sum(dtype=np.uint64))
    return flips, digest, calls, secs


def spread(rec):
    same = {(r["flips"], r["index_sum"]) for rs in rec["runs"].values() for r in rs}
    rec["same_lists"] = len(same) == 1
    for name, rs in rec["runs"].items():
        v = sorted(r["turns_per_s"] for r in rs)
        rec[name + "_turns_per_s"] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}


def bench_shape(W, H, n, turns, pre, bufs, reps):
    cuts = [H * i // n for i in range(n + 1)]
    boards = [golhip.Board(W, H)] if n == 1 else [golhip.Board(W, H, row0=a, rows=b - a)
                                                  for a, b in zip(cuts[:-1], cuts[1:])]

    def reset():
        for b in boards:
            b.fill_random(SEED)
        if n == 1:
            boards[0].step(pre)
        else:
            golhip.group_step(boards, pre)
        for b in boards:
            b.sync()
            b.perf_reset()

    def leg(buf):
        if n == 1:
            return lambda t: stream(lambda k: boards[0].flip_stream(k, cap=CAP, fmt=golhip.FLIPS_INDEX, out=buf), t)
        return lambda t: stream(lambda k: golhip.group_flip_stream(boards, k, cap=CAP, fmt=golhip.FLIPS_INDEX, out=buf), t)

    legs = [(name, leg(buf)) for name, buf in bufs]
    reset()
    for _, fn in legs:  # warm-up: code objects, scratch buffers, the stream's launch estimate
        fn(20)
    rec = {"board": [W, H], "strips": n, "turns": turns, "from_turn": pre, "runs": {k: [] for k, _ in legs}}
    for _ in range(reps):
        for name, fn in legs:
            # the stream launches as many turns as the last batch's largest list lets the buffer
            # hold: take that estimate from this state, not from the end of the leg before
            reset()
            fn(20)
            reset()
            flips, digest, calls, dt = fn(turns)
            p = [b.perf() for b in boards]
            rec["runs"][name].append({"seconds": dt, "turns_per_s": turns / dt, "flips": flips, "index_sum": digest,
                                      "calls": calls, "flip_launches": sum(q["flip_launches"] for q in p),
                                      "flip_resident_launches": sum(q["flip_resident_launches"] for q in p),
                                      "step_launches": sum(q["step_launches"] for q in p),
                                      "pad_launches": sum(q.get("pad_launches", 0) for q in p)})
    spread(rec)
    for b in boards:
        b.close()
    return rec


def main():
    reps = int(arg("--reps", "3"))
    res = {"label": arg("--label", ""), "library_override": bool(os.environ.get("GOLHIP_LIB")),"format": "index", "buffer_entries": CAP,
           "seed": SEED, "reps": reps, "shapes": []}
    pinned = golhip.host_array((CAP,), np.uint32)
    pinned.fill(0)
    pageable = np.empty((CAP,), dtype=np.uint32)
    pageable.fill(0)  # touch the pages outside the timed region
    bufs = [("pinned", pinned), ("pageable", pageable)]
    only = arg("--only")
    for W, H, n, turns in SHAPES:
        if only and only != f"{W}x{H}x{n}":
            continue
        res["shapes"].append(bench_shape(W, H, n, turns, PRE, bufs, reps))
    if "--regress" in sys.argv:  # bench_events.py's stream_index_pinned leg: 5120^2, turns 2065..2264
        rec = bench_shape(5120, 5120, 1, 200, 2064, bufs[:1], reps)
        rec["leg"] = "bench_events.py stream_index_pinned"
        res["regress_5120"] = rec
    text = json.dumps(res)
    out = arg("--out")
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)
    del pinned


main()
