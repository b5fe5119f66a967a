#!/usr/bin/env python3
"""Cost of the core and spectrum rules and the (path, core) table of RMCSA (include/orl.h, orl_batch_route_cores; k_route_cores in
csrc/orl_route_cores.h) at steady state, beside complete_actions and the "path_modulation" mask of the same batch.

On cfg4n of bench.py (RMCSA, NSFNET, 7 cores x 320 slots), 16 384 envs, after 300 warm-up steps of SAP_BM_FC_FF on the device, for
every rule x route with n_given = 0, for every rule with n_given = 2 (one given pair: k C times that is what the table costs without
this kernel), and for complete_actions(n_given = 0 .. 3) and the mask, in the same command:
  * us per launch from HIP events over a window, back to back: launches replayed from a captured graph of 50 of them (no host launch
    cost).  Nothing touches the slot maps in between, so they can stay in the 256 MB MALL (Infinity Cache) where they fit: a lower
    bound, not an HBM figure;
  * the device's actions and table against the restatement (tests/route_cores_restate.py) on the first --check envs.
The kernel reads the link rows of every path of the pair in every core (complete_actions stops at the first pair that fits) and writes
16 B per pair and 16 B per env.  Writes the result as a JSON line to --out (default: stdout only).

    python tools/route_cores_rate.py [--envs 16384] [--warmup 300] [--window 0.3] [--check 128] [--workload cfg4n] [--out FILE]
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
from tests import rmcsa_mask_restate as mr  # noqa: E402
from tests import route_cores_restate as rc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--check", type=int, default=128)
    ap.add_argument("--workload", default="cfg4n")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fam, topo, kw, pol = WORKLOADS[args.workload]
    assert fam == "RMCSA", fam
    n = args.envs
    env = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
    env.run(pol, args.warmup)
    rng = np.random.default_rng(0)
    stream, acts = env.torch_stream(), env.device_tensor("actions")
    K, C, S, M = env.k_paths, env.num_spatial_resources, env.num_spectrum_resources, len(env.modulation_formats)
    services = env.services()
    n_paths = env.topology.n_paths[services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)]
    prefix = np.zeros((n, 4), np.int32)  # a (path, modulation, core) in range per env, for the calls that read a prefix
    prefix[:, 0], prefix[:, 1], prefix[:, 2] = rng.random(n) * n_paths, rng.integers(M, size=n), rng.integers(C, size=n)
    env.action_mask("path_modulation", fetch=False)  # (allocates the buffers before the capture)
    env.route_cores("first", "ksp", fetch=False)
    env.sync()

    def write_prefix():
        with torch.cuda.stream(stream):
            acts.copy_(torch.as_tensor(prefix, device=acts.device))
        env.sync()

    # actions and table against the restatement
    n_chk = min(args.check, n)
    tab = mr.tables_of(env)
    avail = mr.unpack_cores(env.slots_packed()[:n_chk], C, env.topology.n_links, S)
    prep = rc.Prepared(avail, services[:n_chk], env.topology, tab)
    mismatched, rejects = {}, {}
    for rule in rc.RULES:
        want_tab = rc.table(prep, rule)
        for route in rc.ROUTES:
            got, got_tab = env.route_cores(rule, route, table=True)
            bad = (got[:n_chk] != rc.route(prep, want_tab, route)).any(axis=1) | (got_tab[:n_chk] != want_tab).any(axis=(1, 2))
            mismatched["%s_%s" % (rule, route)] = int(bad.sum())
            rejects["%s_%s" % (rule, route)] = round(float((got[:, 0] == K).mean()), 4)

    fns = {"mask_path_modulation": lambda: env.action_mask("path_modulation", fetch=False)}
    for g in range(4):
        fns["complete_g%d" % g] = lambda g=g: env.complete_actions(n_given=g, fetch=False)
    for rule in rc.RULES:
        for route in rc.ROUTES:
            fns["%s_%s" % (rule, route)] = lambda rule=rule, route=route: env.route_cores(rule, route, fetch=False)
        fns["%s_pair" % rule] = lambda rule=rule: env.route_cores(rule, "ksp", n_given=2, fetch=False)
    us = {k: [] for k in fns}
    for _ in range(2):  # alternated
        for k, fn in fns.items():
            write_prefix()  # (every launch overwrites the row: each window starts from the same prefix again)
            graph = graph_of(fn, stream)
            ms, reps = time_window(graph.replay, stream, args.window / 2)
            us[k].append(1e3 * ms / (reps * 50))
            del graph
    best = {k: round(min(v), 2) for k, v in us.items()}
    # the table without this kernel: k C launches of route_cores(rule, n_given=2)
    over_kc = {rule: round(max(best["%s_%s" % (rule, route)] for route in rc.ROUTES) / (K * C * best["%s_pair" % rule]), 4) for rule in rc.RULES}
    rec = dict(workload=args.workload, family=fam, envs=n, links=int(env.topology.n_links), slots=S, cores=C, k=K, us_per_launch_back_to_back=best,
               us_per_launch_back_to_back_all={k: [round(x, 2) for x in v] for k, v in us.items()}, route_cores_over_kC_times_pair=over_kc,
               device_vs_restatement_mismatched_rows=mismatched, rows_checked=n_chk, reject_share=rejects,
               device=torch.cuda.get_device_name(env.device_id), time=time.strftime("%Y-%m-%d %H:%M:%S"))
    print(json.dumps(rec), flush=True)
    env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
