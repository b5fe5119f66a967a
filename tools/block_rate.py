#!/usr/bin/env python3
"""Cost of the block actions (include/orl.h, orl_batch_block_table / orl_batch_select_blocks; k_block_table and k_select_blocks in
csrc/orl_blocks.h) at steady state, beside the calls of the same batch that read the same rows.

On cfg2 (RMSA) and cfg1 (RWA) of bench.py at 65 536 envs and cfg4n (RMCSA, 7 cores x 320 slots) at 16 384 envs, after 300 warm-up steps
of the family's heuristic on the device, in the same command: block_table(j) for j = 1 and 4, select_blocks(j) with the index in the
actions buffer, path_features(j) for the same j, route_spectrum("first") / route_cores("first") and the family's mask ("joint" /
"path_modulation"):
  * us per launch from HIP events over a window, back to back: launches replayed from a captured graph of 50 of them (no host launch
    cost), the cases alternated over two rounds, the minimum kept.  Nothing touches the slot maps in between, so they can stay in the
    256 MB MALL (Infinity Cache) where they fit: a lower bound, not an HBM figure;
  * bytes each launch writes per env, from the row shapes;
  * the device's table, mask and selection against the restatement (tests/block_restate.py) on the first --check envs.
Writes one JSON line per workload to --out (default: stdout only).

    python tools/block_rate.py [--envs 65536] [--rmcsa-envs 16384] [--warmup 300] [--window 0.3] [--check 64] [--only cfg2,cfg1,cfg4n] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402
from bench import WORKLOADS  # noqa: E402
from mask_rate import time_window  # noqa: E402
from path_obs_rate import graph_of  # noqa: E402
from tests import block_restate as br  # noqa: E402
from tests import path_features_restate as pf  # noqa: E402
from tests import rmcsa_mask_restate as mr  # noqa: E402

JS = (1, 4)


def measure(name, n, args):
    fam, topo, kw, pol = WORKLOADS[name]
    env = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
    env.run(pol, args.warmup)
    rmcsa = fam == "RMCSA"
    stream, acts = env.torch_stream(), env.device_tensor("actions")
    R = env.k_paths * env.num_spatial_resources
    # against the restatement
    n_chk = min(args.check, n)
    env_type, avail, services = pf.state_of(env)
    rows = br.Rows(env_type, avail[:n_chk], services[:n_chk], env.topology, mr.tables_of(env) if rmcsa else None)
    rng = np.random.default_rng(0)
    mismatched, index = {}, {}
    for j in JS:
        tab, msk = env.block_table(j)
        bad = (tab[:n_chk] != br.table(rows, j)).any(axis=(1, 2)) | (msk[:n_chk] != br.mask(rows, j, env.allow_rejection)).any(axis=1)
        # an index per env that a masked agent could have drawn: a set column where the env has one
        idx = np.array([rng.choice(np.flatnonzero(m[:-1])) if m[:-1].any() else R * j for m in msk], np.int32)
        got = env.select_blocks(idx, j)
        bad |= (got[:n_chk] != br.select(rows, j, idx[:n_chk])).any(axis=1)
        mismatched["j%d" % j], index[j] = int(bad.sum()), idx
    mask_layout = "path_modulation" if rmcsa else "joint"
    route = (lambda: env.route_cores("first", "ksp", fetch=False)) if rmcsa else (lambda: env.route_spectrum("first", "ksp", fetch=False))
    fns = {"mask_" + mask_layout: lambda: env.action_mask(mask_layout, fetch=False), "route_first": route}
    for j in JS:
        fns["block_table_j%d" % j] = lambda j=j: env.block_table(j, fetch=False)
        fns["path_features_j%d" % j] = lambda j=j: env.path_features(j, fetch=False)
        fns["select_blocks_j%d" % j] = lambda j=j: env.select_blocks(None, j, fetch=False)
    for fn in fns.values():  # (allocates the buffers before the capture)
        fn()
    env.sync()
    us = {k: [] for k in fns}
    for _ in range(2):  # alternated
        for k, fn in fns.items():
            full = np.zeros((n, 4), np.int32)
            full[:, 0] = index[int(k[-1])] if k.startswith("select") else 0
            with torch.cuda.stream(stream):  # (a selection overwrites its index: each window starts from the same indices; the later launches
                acts.copy_(torch.as_tensor(full, device=acts.device))  # of a window read the path it left in column 0, an index in range)
            env.sync()
            graph = graph_of(fn, stream)
            ms, reps = time_window(graph.replay, stream, args.window / 2)
            us[k].append(1e3 * ms / (reps * 50))
            del graph
    written = {"route_first": 16 + 16 * (R if rmcsa else env.k_paths), "mask_" + mask_layout: env.action_mask_shape(mask_layout)[1]}
    for j in JS:
        sh = env.block_table_shape(j)
        written["block_table_j%d" % j] = 4 * sh[2] + sh[4]
        written["path_features_j%d" % j] = 4 * env.path_features_shape(j)[2]
        written["select_blocks_j%d" % j] = 16
    rec = dict(workload=name, family=fam, envs=n, links=int(env.topology.n_links), slots=env.num_spectrum_resources, cores=env.num_spatial_resources,
               k=env.k_paths, rows=R, us_per_launch_back_to_back={k: round(min(v), 2) for k, v in us.items()},
               us_per_launch_back_to_back_all={k: [round(x, 2) for x in v] for k, v in us.items()}, bytes_written_per_env=written,
               device_vs_restatement_mismatched_rows=mismatched, rows_checked=n_chk, device=torch.cuda.get_device_name(env.device_id),
               time=time.strftime("%Y-%m-%d %H:%M:%S"))
    print(json.dumps(rec), flush=True)
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rmcsa-envs", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--only", default="cfg2,cfg1,cfg4n")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [measure(name, args.rmcsa_envs if WORKLOADS[name][0] == "RMCSA" else args.envs, args) for name in args.only.split(",")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
