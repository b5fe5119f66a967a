#!/usr/bin/env python3
"""Cost of the network capacity view (include/orl.h, orl_batch_network_capacity; k_network_capacity in csrc/orl_capacity.h) at steady
state, beside the views of the same batch that read the same slot maps.

On cfg2 (RMSA) and cfg1 (RWA) of bench.py at 65 536 envs, cfg4n (RMCSA, 7 cores x 320 slots) at 16 384 and cfg5 (RMSA on germany50) at
8 192, after a warm-up of the family's heuristic on the device (--warmup, 1 500 steps), in the same command: network_capacity("paths"),
("serviceable") and ("counts"), path_features(1), link_features() and block_table(1):
  * us per launch from HIP events over a window, back to back: launches replayed from a captured graph of --launches of them (no host
    launch cost), the cases alternated over two rounds, the minimum kept.  Nothing touches the state in between, so it can stay in the
    256 MB MALL (Infinity Cache) where it fits: a lower bound, not an HBM figure;
  * per launch and env the bytes of slot map read once (C' E W words) and of rows written (the pitch), and the TB/s they make of the
    time; the LDS bytes of one env from the plan (orl_debug_capacity_plan);
  * the device's rows against the restatement (tests/capacity_restate.py) from slots_packed() on the first --check envs.
Writes one JSON line per workload to --out (default: stdout only).

    python tools/capacity_rate.py [--envs 65536] [--rmcsa-envs 16384] [--ger-envs 8192] [--warmup 1500] [--window 0.3] [--check 8]
                                  [--only cfg2,cfg1,cfg4n,cfg5] [--out FILE]
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
from tests import capacity_restate as cap  # noqa: E402
from tests import rmcsa_mask_restate as mr  # noqa: E402

LAYOUTS = ("paths", "serviceable", "counts")
PLAN_FIELDS = ("dim", "rows", "width", "pitch", "ok", "waves", "block", "grid", "lds_bytes", "staged", "wave_bytes")


def plan_of(env, layout, n_br):
    cfg, d = env._cfg, env._desc
    out = (ctypes.c_int32 * len(PLAN_FIELDS))()
    assert env.lib.orl_debug_capacity_plan(cfg.env_type, env.lib.orl_batch_row_words(env._h), env.num_envs, d.n_nodes, d.n_links, d.k_paths,
                                           cfg.num_spatial_resources, cfg.num_spectrum_resources, d.n_modulations, n_br, layout, out) == len(PLAN_FIELDS)
    return dict(zip(PLAN_FIELDS, out))


def measure(name, n, args):
    fam, topo, kw, pol = WORKLOADS[name]
    env = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
    env.run(pol, args.warmup)
    stream = env.torch_stream()
    C, S = (env.num_spatial_resources if fam == "RMCSA" else 1), env.num_spectrum_resources
    W = env.lib.orl_batch_row_words(env._h)
    n_br = len(env._keep["bit_rates"])
    # against the restatement
    n_chk = min(args.check, n)
    tab = mr.tables_of(env) if fam == "RMCSA" else None
    need = cap.need_table(fam, env.topology, cap.class_rates(fam, kw), tab)
    avail = mr.unpack_cores(env.slots_packed()[:n_chk], C, env.topology.n_links, S)
    want = dict(zip(LAYOUTS, cap.restate(avail, env.topology, need)))
    mismatched = {lay: int((env.network_capacity(lay)[:n_chk] != want[lay]).any(axis=1).sum()) for lay in LAYOUTS}
    n_cls = need.shape[3]
    blocked = want["counts"][:, :n_cls].sum(axis=1)
    fns = {"capacity_" + lay: (lambda lay=lay: env.network_capacity(lay, fetch=False)) for lay in LAYOUTS}
    fns["path_features_j1"] = lambda: env.path_features(1, fetch=False)
    fns["link_features"] = lambda: env.link_features(fetch=False)
    fns["block_table_j1"] = lambda: env.block_table(1, fetch=False)
    for fn in fns.values():  # (allocates the buffers before the capture)
        fn()
    env.sync()
    us = {k: [] for k in fns}
    for _ in range(2):  # alternated
        for k, fn in fns.items():
            graph = graph_of(fn, stream, args.launches)
            ms, reps = time_window(graph.replay, stream, args.window / 2)
            us[k].append(1e3 * ms / (reps * args.launches))
            del graph
    best = {k: min(v) for k, v in us.items()}
    map_bytes = 8 * C * env.topology.n_links * W
    written = {"capacity_" + lay: env.network_capacity_shape(lay)[3] * (1 if lay == "serviceable" else 4) for lay in LAYOUTS}
    written["path_features_j1"] = 4 * env.path_features_shape(1)[2]
    written["link_features"] = 4 * env.link_features_shape()[3]
    bt = env.block_table_shape(1)
    written["block_table_j1"] = 4 * bt[2] + bt[4]
    model = {k: dict(map_bytes_read=map_bytes, row_bytes_written=int(w), tb_per_s=round((map_bytes + w) * n / (best[k] * 1e-6) / 1e12, 3))
             for k, w in written.items()}
    plans = {lay: {f: plan_of(env, i, n_br)[f] for f in ("waves", "lds_bytes", "staged", "wave_bytes")} for i, lay in enumerate(LAYOUTS)}
    rec = dict(workload=name, family=fam, envs=n, nodes=int(env.topology.n_nodes), links=int(env.topology.n_links), slots=S, cores=C, k=env.k_paths,
               classes=n_cls, path_rows=int(env.network_capacity_shape("paths")[0]), warmup=args.warmup,
               blocked_cells_per_env=[int(blocked.min()), int(blocked.max())], cells=int((env.topology.n_paths > 0).sum()) * n_cls,
               us_per_launch_back_to_back={k: round(v, 2) for k, v in best.items()},
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
    ap.add_argument("--ger-envs", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=1500)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--launches", type=int, default=20, help="launches per captured graph")
    ap.add_argument("--check", type=int, default=8)
    ap.add_argument("--only", default="cfg2,cfg1,cfg4n,cfg5")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sizes = lambda name: args.rmcsa_envs if WORKLOADS[name][0] == "RMCSA" else (args.ger_envs if WORKLOADS[name][1] == "germany50" else args.envs)
    lines = [measure(name, sizes(name), args) for name in args.only.split(",")]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
