"""N > 1 path: one process per device, contiguous env shards, no data-path collective.
Checked on CPU with 2 gloo ranks: the shard partition logic of the product (optical_rl_gym_amd.sharding) plus
the oracle as the stepper must give every env the same trajectory as a 1-process run."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from optical_rl_gym_amd.sharding import shard_range, shard_seeds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(load=300, mean_service_holding_time=25, episode_length=40, num_spectrum_resources=320)
N_TOTAL, STEPS, BASE_SEED = 10, 120, 10


def _run(seeds):
    sys.path.insert(0, ROOT)
    from oracle.oracle import OracleBatch

    env = OracleBatch("RMSA", "nsfnet_chen", seeds, **KW)
    acc = np.zeros(len(seeds))
    for _ in range(STEPS):
        _, r, _, _ = env.step(env.policy("SAP_FF"), auto_reset=True)
        acc += r
    return np.concatenate([env.counters().astype(np.float64), env.services()[:, :2], acc[:, None]], axis=1)


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    local = torch.from_numpy(_run(shard_seeds(BASE_SEED, N_TOTAL, rank, world)))
    sizes = [shard_range(N_TOTAL, r, world) for r in range(world)]
    bufs = [torch.zeros((hi - lo, local.shape[1]), dtype=torch.float64) for lo, hi in sizes]
    dist.all_gather(bufs, local)  # test-only gather of the results; the data path itself has no collective
    dist.barrier()
    if rank == 0:
        np.save(out, torch.cat(bufs).numpy())
    dist.destroy_process_group()


def test_shard_partition():
    for n, w in ((10, 2), (65536, 8), (7, 3), (262144, 8), (65537, 8), (1000003, 7)):
        bounds = [shard_range(n, r, w) for r in range(w)]
        # contiguous, in order, covering [0, n) exactly once, balanced to within one env
        assert bounds[0][0] == 0 and bounds[-1][1] == n
        for (lo0, hi0), (lo1, _) in zip(bounds, bounds[1:]):
            assert hi0 == lo1 and lo0 <= hi0
        sizes = [hi - lo for lo, hi in bounds]
        assert sum(sizes) == n and max(sizes) - min(sizes) <= 1
        if n < 100:
            assert [i for lo, hi in bounds for i in range(lo, hi)] == list(range(n))
    assert shard_range(65536, 3, 8) == (24576, 32768) and shard_range(262144, 7, 8) == (229376, 262144)
    assert shard_seeds(10, 10, 1, 2) == [15, 16, 17, 18, 19]


def _bench(*flags, env=None):
    import json
    import subprocess

    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(flags), env=e, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None)


@pytest.mark.timeout(300)
def test_bench_gpus_n_starts_n_ranks():
    """`bench.py --gpus 2` started by hand launches two ranks itself (the plumbing only: rendezvous, barrier, report)."""
    p, out = _bench("--gpus", "2", "--launch-check")
    assert p.returncode == 0, p.stderr
    assert out["n_gpus"] == 2 and [r["rank"] for r in out["ranks"]] == [0, 1] and [r["device"] for r in out["ranks"]] == [0, 1]
    assert len({r["pid"] for r in out["ranks"]}) == 2
    # a world size that contradicts --gpus is an error, not a silent 1-GPU measurement
    p, _ = _bench("--gpus", "2", "--launch-check", env={"WORLD_SIZE": "1", "RANK": "0"})
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_two_ranks_on_one_device_and_refusal():
    import torch

    if torch.cuda.device_count() < 2:  # asked for more GPUs than there are: refuse loudly
        p, out = _bench("--gpus", "2", "--steps", "20", "--no-cpu-baseline")
        assert p.returncode != 0 and out is None and "only 1 GPU" in p.stderr
    p, out = _bench("--gpus", "2", "--device", "0", "--batch", "4096", "--steps", "20", "--no-cpu-baseline")
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["n_gpus"] == 2 and len(out["per_rank"]) == 2 and out["scaling"] == "weak"
    assert out["value"] > 0 and all(r["env_steps_per_s"] > 0 for r in out["per_rank"])
    assert [r["envs"] for r in out["per_rank"]] == [4096, 4096] and out["config"]["envs_total"] == 8192
    # strong scaling: --batch is the job's; the ranks own contiguous blocks of it (here 4 104 envs -> 2 052 + 2 052)
    p, out = _bench("--gpus", "2", "--device", "0", "--scaling", "strong", "--batch", "4104", "--steps", "20", "--no-cpu-baseline")
    assert p.returncode == 0, p.stderr[-2000:]
    assert out["scaling"] == "strong" and [r["envs"] for r in out["per_rank"]] == [2052, 2052]
    assert out["config"]["envs_total"] == 4104 and out["config"]["envs_per_gpu"] == [2052, 2052] and out["value"] > 0


@pytest.mark.timeout(300)
def test_two_rank_shards_match_single_process(tmp_path):
    out = str(tmp_path / "gathered.npy")
    port = 29500 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    sharded = np.load(out)
    single = _run([BASE_SEED + i for i in range(N_TOTAL)])
    assert np.array_equal(sharded, single)
