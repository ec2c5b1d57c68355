"""`bench.py --dump-outputs DIR` on the GPU: a plain run (no --full) of
configs[1]'s board at 16 turns a step writes the board its last timed step
left -- sampled rows as cells, the whole board's digest and alive count --
and they equal the bit-packed CPU oracle's board at that turn, whatever the
clock-bound warmup ran before."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_is_the_last_timed_steps_board(tmp_path):
    import bench
    from oracle.oracle import COracle

    W, tps, steps, warmup = 16384, 16, 2, 1
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", str(W),
                        "--turns-per-step", str(tps), "--steps", str(steps), "--warmup", str(warmup),
                        "--warmup-seconds", "0.2", "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    (line,) = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    turn = (warmup + steps) * tps
    assert line["parity"] is True and line["parity_check"]["fixture"] == "tests/golden/fullsize.json c1 turn 16"
    assert line["final_turn"] == turn and line["steps"] == steps and line["warmup_extra_steps"] >= 1
    assert line["ms_per_step"] > 0 and "configs3" not in line and "cpu_baseline" not in line

    out = {f.name[:-4]: np.load(f) for f in (tmp_path / "out").iterdir()}
    assert sorted(out) == ["board_alive", "board_digest", "board_row_index", "board_rows"]
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20

    o, nth = COracle(), min(16, len(os.sched_getaffinity(0)))
    words = o.fill_random64(W, W, bench.WORKLOADS[W]["seed"], nth)
    o.run_fast_words(words, W, turn, nth)
    digest = o.hash64(words, W, nth)
    assert list(out["board_digest"]) == [digest >> 32, digest & 0xFFFFFFFF]
    assert list(out["board_alive"]) == [o.popcount64(words, W, nth), turn]
    rows = out["board_row_index"].astype(np.int64)
    assert rows[0] == 0 and rows[-1] == W - 1 and len(rows) > 100
    assert np.array_equal(rows, bench.dump_sample_rows(W, W))
    assert np.array_equal(out["board_rows"], o.unpack64(words[rows], W) != 0)
