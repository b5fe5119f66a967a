#!/usr/bin/env python3
"""Cost of the release horizons (include/orl.h, orl_batch_release_horizons; k_release_horizons in csrc/orl_horizon.h) at steady state,
beside the views of the same batch that read the slot maps.

On cfg2 (RMSA) and cfg1 (RWA) of bench.py at 65 536 envs and cfg4n (RMCSA, 7 cores x 320 slots) at 16 384 envs, after a warm-up of the
family's heuristic on the device long enough that the release tables are at steady state (--warmup, 1 500 steps: cfg2 needs about that
many), in the same command: release_horizons("slots"), release_horizons("blocks", j) for j = 1 and 4, block_table(j) and
path_features(j) for the same j, and link_features():
  * us per launch from HIP events over a window, back to back: launches replayed from a captured graph of 50 of them (no host launch
    cost), the cases alternated over two rounds, the minimum kept.  Nothing touches the state in between, so it can stay in the 256 MB
    MALL (Infinity Cache) where it fits: a lower bound, not an HBM figure;
  * the algorithmic bytes of a horizon launch per env — the release table's words up to the mean high-water mark (a time and a record,
    16 bytes per slot, once per round of rows) plus the row bytes written — and the TB/s they make of the time;
  * the device's rows against the restatement (tests/horizon_restate.py) from pending() on the first --check envs.
Writes one JSON line per workload to --out (default: stdout only).

    python tools/horizon_rate.py [--envs 65536] [--rmcsa-envs 16384] [--warmup 1500] [--window 0.3] [--check 16] [--only cfg2,cfg1,cfg4n] [--out FILE]
"""
import argparse
import ctypes
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
from tests import horizon_restate as hr  # noqa: E402
from tests import path_features_restate as pf  # noqa: E402
from tests import rmcsa_mask_restate as mr  # noqa: E402

JS = (1, 4)
SC_EV = 19  # word of the scalar record: high-water mark | count << 32 of the env's release table


def plan_of(env, layout, j):
    cfg, d = env._cfg, env._desc
    out = (ctypes.c_int32 * 10)()
    assert env.lib.orl_debug_horizon_plan(cfg.env_type, env.lib.orl_batch_row_words(env._h), env.num_envs, d.n_nodes, d.n_links, d.k_paths,
                                          cfg.num_spatial_resources, cfg.num_spectrum_resources, d.n_modulations, layout, j, out) == 10
    return dict(zip(("dim", "rows", "width", "pitch", "ok", "waves", "block", "grid", "lds_bytes", "rows_per_round"), out))


def measure(name, n, args):
    fam, topo, kw, pol = WORKLOADS[name]
    env = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
    env.run(pol, args.warmup)
    rmcsa = fam == "RMCSA"
    stream = env.torch_stream()
    C, S = env.num_spatial_resources, env.num_spectrum_resources
    ev = env.get_state()[:n * 256].view(np.uint64).reshape(n, 32)[:, SC_EV]
    hwm, count = float((ev & np.uint64(0xffffffff)).mean()), float((ev >> np.uint64(32)).mean())
    # against the restatement
    n_chk = min(args.check, n)
    env_type, avail, services = pf.state_of(env)
    pending = [env.pending(e) for e in range(n_chk)]
    H = hr.slots_layout(pending, services[:n_chk], env.topology, C, S)
    rows = br.Rows(env_type, avail[:n_chk], services[:n_chk], env.topology, mr.tables_of(env) if rmcsa else None)
    same = lambda a, b: int((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum())
    mismatched = {"slots": same(env.release_horizons("slots")[:n_chk], H)}
    for j in JS:
        mismatched["blocks_j%d" % j] = same(env.release_horizons("blocks", j)[:n_chk], hr.blocks_layout(H, rows, j, services[:n_chk]))
    fns = {"horizons_slots": lambda: env.release_horizons("slots", fetch=False), "link_features": lambda: env.link_features(fetch=False)}
    for j in JS:
        fns["horizons_blocks_j%d" % j] = lambda j=j: env.release_horizons("blocks", j, fetch=False)
        fns["block_table_j%d" % j] = lambda j=j: env.block_table(j, fetch=False)
        fns["path_features_j%d" % j] = lambda j=j: env.path_features(j, fetch=False)
    for fn in fns.values():  # (allocates the buffers before the capture)
        fn()
    env.sync()
    us = {k: [] for k in fns}
    for _ in range(2):  # alternated
        for k, fn in fns.items():
            graph = graph_of(fn, stream)
            ms, reps = time_window(graph.replay, stream, args.window / 2)
            us[k].append(1e3 * ms / (reps * 50))
            del graph
    best = {k: min(v) for k, v in us.items()}
    model, plans = {}, {}
    for k, (layout, j) in {"horizons_slots": (0, 1), "horizons_blocks_j1": (1, 1), "horizons_blocks_j4": (1, 4)}.items():
        pl = plan_of(env, layout, j)
        rounds = -(-pl["rows"] // pl["rows_per_round"])
        per_env = 16.0 * hwm * rounds + 4.0 * pl["pitch"]
        model[k] = dict(bytes_per_env=round(per_env, 1), tb_per_s=round(per_env * n / (best[k] * 1e-6) / 1e12, 3))
        plans[k] = dict(waves=pl["waves"], lds_bytes=pl["lds_bytes"], rows_per_round=pl["rows_per_round"], rounds=rounds)
    rec = dict(workload=name, family=fam, envs=n, links=int(env.topology.n_links), slots=S, cores=C, k=env.k_paths, rows=env.k_paths * C, warmup=args.warmup,
               mean_high_water_mark=round(hwm, 1), mean_pending=round(count, 1), us_per_launch_back_to_back={k: round(v, 2) for k, v in best.items()},
               us_per_launch_back_to_back_all={k: [round(x, 2) for x in v] for k, v in us.items()}, byte_model=model, plan=plans,
               device_vs_restatement_mismatched_rows=mismatched, rows_checked=n_chk, device=torch.cuda.get_device_name(env.device_id),
               time=time.strftime("%Y-%m-%d %H:%M:%S"))
    print(json.dumps(rec), flush=True)
    env.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rmcsa-envs", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=1500)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--check", type=int, default=16)
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
