"""bench.py --dump-outputs: what the timed run() computed, written as float32 / float64 .npy files within the size budget; the
same arguments give the same arrays from run to run, and those arrays are the oracle's state after the same steps."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {os.path.basename(p)[:-4]: np.load(p) for p in sorted(glob.glob(os.path.join(d, "*.npy")))}


def test_dump_outputs_layout_and_budget(tmp_path):
    """dump_outputs on a batch of the CPU oracle (same read-back methods as the product): every array float32 / float64,
    the whole batch where it fits, a fixed sample of it where it does not, and the files within the budget."""
    from bench import WORKLOADS, dump_outputs
    from tests.oracle_backend import OracleBackend

    fam, topo, kw, policy = WORKLOADS["cfg3"]  # (DeepRMSA: the observation too)
    seeds = [10 + i for i in range(40)]
    env = OracleBackend(fam, topo, seeds, **kw)
    env.run(policy, 30)
    whole, small = str(tmp_path / "whole"), str(tmp_path / "small")
    dump_outputs(env, whole, 100)
    dump_outputs(env, small, 100, budget=40_000)
    dump_outputs(env, str(tmp_path / "again"), 100, budget=40_000)
    a, s, again = _load(whole), _load(small), _load(str(tmp_path / "again"))
    assert sorted(a) == ["active", "counters", "env_index", "link_stats", "net_stats", "observation", "sample_env_index",
                         "services", "slots"]
    assert all(v.dtype in (np.float32, np.float64) for v in list(a.values()) + list(s.values()))
    assert np.array_equal(a["env_index"], 100 + np.arange(40)) and np.array_equal(a["sample_env_index"], a["env_index"])
    assert np.array_equal(a["counters"], env.counters()) and np.array_equal(a["services"], env.services())
    assert np.array_equal(a["observation"], env.observation()) and np.array_equal(a["link_stats"], env.link_stats_all())
    assert np.array_equal(a["slots"][7], env.slots(7))
    # a budget below the batch: a sorted sample, the slot maps of a subset of it, the same draw every time
    rows, sample = s["env_index"].astype(int) - 100, s["sample_env_index"].astype(int) - 100
    assert 0 < len(sample) < len(rows) < 40 and set(sample) <= set(rows) and (np.diff(rows) > 0).all()
    assert np.array_equal(s["counters"], env.counters()[rows]) and np.array_equal(s["slots"][-1], env.slots(int(sample[-1])))
    assert sum(v.nbytes for v in s.values()) <= 40_000
    assert sorted(again) == sorted(s) and all(np.array_equal(again[k], s[k]) for k in s)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_dump_is_reproducible_and_is_the_oracle_state(tmp_path):
    from bench import WORKLOADS
    from oracle.oracle import OracleBatch

    args = ["--gpus", "1", "--batch", "4096", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"]
    dumps = []
    for r in range(2):
        d = str(tmp_path / ("run%d" % r))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", d],
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        assert out["steps"] == 20 and out["timing"]["blocks"] == 1
        assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(d, "*.npy"))) <= 64 << 20
        dumps.append(_load(d))
    a, b = dumps
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert np.array_equal(a["env_index"], np.arange(4096))  # (4 096 envs fit the budget whole)
    # the state after the preparation (1 500 + 5 steps, then 50 runs of 20) and the 20 timed steps, on the CPU, for a few of the
    # sampled envs
    assert out["timing"]["state_preparation_steps"] == 2505
    fam, topo, kw, policy = WORKLOADS["cfg2"]
    pick = np.arange(0, len(a["sample_env_index"]), 97)
    envs = a["sample_env_index"][pick].astype(int)
    ora = OracleBatch(fam, topo, [10 + int(e) for e in envs], **kw)
    ora.run(policy, 2505 + 20)
    assert np.array_equal(a["counters"][envs], ora.counters()) and np.array_equal(a["services"][envs], ora.services())
    assert np.array_equal(a["net_stats"][envs], ora.net_stats_all()) and np.array_equal(a["active"][envs], ora.active())
    assert np.array_equal(a["link_stats"][pick], ora.link_stats_all())
    for i, e in enumerate(pick):
        assert np.array_equal(a["slots"][e], ora.slots(i))
