"""bench.py's multi-rank path end to end on one GPU:
two rank processes run bench.main() exactly as `bench.py --gpus 2` ranks do
(measure() of configs[2] and the configs3 block, parity against the
full-size fixtures, the barrier-bracketed timed region, max over ranks, the
per-rank rows, rank 0's one JSON line), through bench.RankEnv itself (its
gloo control plane, as in production) with one substitution a single GPU
forces: RankEnv.ring_init, so each strip joins its halo ring through
golhip_test_ring_init (GOLHIP_TEST_HOOKS=1), the exchange and the global
alive count's allreduce riding gloo messages at the place of the RCCL calls.  The
line's timings are meaningless (two ranks share one GPU); its parity, plan
and plumbing are what is checked.  RCCL's own transport is left to the
driver's multi-GPU run.
"""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RANK_MAIN = r'''
import os, sys
sys.path[:0] = [{root!r}, os.path.join({root!r}, "game-of-life-distributed_amd")]
sys.argv = ["bench.py"] + {argv!r}
import torch
import torch.distributed as dist
import bench


class HostRingEnv(bench.RankEnv):
    """bench.RankEnv exactly as the driver's ranks run it (gloo control
    plane, the library's ring schedule, golhip_alive_count_global), except
    that the halo ring joins through the test transport instead of RCCL (two
    ranks cannot share one GPU in RCCL)."""

    def ring_init(self, board, tag=""):
        self.stage(tag + "golhip_test_ring_init (host transport over gloo)")
        rows = [None] * self.world
        dist.all_gather_object(rows, board.rows)

        def exchange(prev, nxt, up, down):
            n = len(up)
            top, bottom = torch.empty(n, dtype=torch.uint8), torch.empty(n, dtype=torch.uint8)
            reqs = [dist.isend(torch.frombuffer(bytearray(up), dtype=torch.uint8), prev, tag=0),
                    dist.isend(torch.frombuffer(bytearray(down), dtype=torch.uint8), nxt, tag=1),
                    dist.irecv(top, prev, tag=1), dist.irecv(bottom, nxt, tag=0)]
            for r in reqs:
                r.wait()
            return top.numpy().tobytes(), bottom.numpy().tobytes()

        def allreduce(x):  # golhip_alive_count_global's sum
            t = torch.tensor([x], dtype=torch.int64)
            dist.all_reduce(t)
            return int(t.item())

        board.test_ring_init(self.world, self.rank, min(rows), exchange, allreduce)


# the tested env differs from the production one in ring_init alone
assert sorted(k for k in vars(HostRingEnv) if not k.startswith("__")) == ["ring_init"]
bench.main(env_factory=HostRingEnv)
'''


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(450)
def test_bench_two_ranks_host_ring(tmp_path):
    world = 2
    argv = ["--gpus", str(world), "--steps", "1", "--warmup", "1", "--warmup-seconds", "0", "--full",
            "--no-cpu-baseline", "--configs3-warmup-seconds", "0", "--stage-timeout", "200"]
    script = tmp_path / "rank_main.py"
    script.write_text(RANK_MAIN.format(root=ROOT, argv=argv))
    port = _free_port()
    procs, files = [], []
    for r in range(world):
        env = dict(os.environ, GOLHIP_TEST_HOOKS="1", RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world),
                   LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        out, err = tmp_path / f"rank{r}.out", tmp_path / f"rank{r}.err"
        files.append((out, err))
        with open(out, "w") as fo, open(err, "w") as fe:
            procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=fo, stderr=fe))
    try:
        for p in procs:
            p.wait(timeout=400)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    outs = [(o.read_text(), e.read_text()) for o, e in files]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1, outs[0][0][-2000:]
    assert not [ln for ln in outs[1][0].splitlines() if ln.startswith("{")]  # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["parity"] is True, d.get("parity_check")
    assert d["parity_check"]["ok"] is True and d["configs3"]["parity"] is True, d["configs3"].get("parity_check")
    for blk in (d, d["configs3"]):
        ranks = blk["config"]["ranks"]
        assert [r["rank"] for r in ranks] == list(range(world)), ranks
        assert blk["config"]["comm"]["nranks"] == world
        assert blk["value"] > 0 and blk["ms_per_step"] > 0


@pytest.mark.timeout(300)
def test_bench_one_rank_rccl_ring_production_path(tmp_path):
    """`bench.py --ring`: the production RankEnv unchanged (gloo control
    plane of one rank, rank 0's RCCL unique id over it, golhip_comm_init's
    ncclCommInitRank and strip-row allreduce), the whole configs[2] board as
    a one-rank RCCL ring (force_halo: the ncclSend / ncclRecv group of every
    exchange), and the parity step's alive count from
    golhip_alive_count_global's ncclAllReduce -- against the c2 fixture at
    turn 1000."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GOLHIP_TEST_HOOKS"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--ring", "--steps", "1", "--warmup", "1",
                        "--warmup-seconds", "0", "--no-cpu-baseline", "--no-configs3", "--stage-timeout", "200"],
                       env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    (line,) = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert line["parity"] is True, line["parity_check"]
    assert line["parity_check"]["fixture"] == "tests/golden/fullsize.json c2 turn 1000"
    cfg = line["config"]
    assert cfg["comm"] == {"nranks": 1, "rank": 0, "ring_rows": 65536}
    assert cfg["parallelism"] == "one-rank RCCL ring (force_halo)" and cfg["halo_exchanges"] > 0
    assert cfg["control_plane"].startswith("gloo")
    assert line["final_turn"] == 2000
