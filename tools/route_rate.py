#!/usr/bin/env python3
"""Cost of the routing rules and the per-path assignment table (include/orl.h, orl_batch_route_spectrum; k_route_spectrum in
csrc/orl_route.h) at steady state, beside assign_spectrum of the same rule and the "joint" action mask of the same batch.

On cfg2 (RMSA, NSFNET, 320 slots), cfg5 (RMSA, Germany50's 88 links, 320 slots) and cfg1 (RWA, NSFNET, 80 wavelengths) of bench.py,
65 536 envs each, after 300 warm-up steps of the workload's heuristic on the device, for every rule x route, and for
assign_spectrum(rule) with n_given = 0 (the first path that fits) and n_given = 1 (one given path: k times that is what the table costs
without this kernel) and the mask, in the same command:
  * us per launch from HIP events over a window, back to back: launches replayed from a captured graph of 50 of them (no host launch
    cost).  Nothing touches the slot maps in between, so they can stay in the 256 MB MALL (Infinity Cache) where they fit: a lower
    bound, not an HBM figure;
  * the device's actions and table against the restatement (tests/route_restate.py) on the first --check envs.
The route kernel reads the link rows of every path of the pair (assign_spectrum stops at the first that fits) and writes 16 B per
path and 16 B per env.  Writes the results as JSON lines to --out (default: stdout only).

    python tools/route_rate.py [--envs 65536] [--warmup 300] [--window 0.3] [--check 256] [--only cfg2,cfg5,cfg1] [--out FILE]
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
from tests import assign_restate as ar  # noqa: E402
from tests import route_restate as rr  # noqa: E402

CASES = ("cfg2", "cfg5", "cfg1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--check", type=int, default=256)
    ap.add_argument("--only", default=None, help="comma-separated: " + ",".join(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else None
    lines = []
    for wl in CASES:
        if only and wl not in only:
            continue
        fam, topo, kw, pol = WORKLOADS[wl]
        n = args.envs
        env = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
        env.run(pol, args.warmup)
        rng = np.random.default_rng(0)
        stream, acts = env.torch_stream(), env.device_tensor("actions")
        K, S = env.k_paths, env.num_spectrum_resources
        services = env.services()
        n_paths = env.topology.n_paths[services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)]
        paths = (rng.random(n) * n_paths).astype(np.int32)
        env.action_mask("joint", fetch=False)  # (allocates the buffers before the capture)
        env.route_spectrum("first", "ksp", fetch=False)
        env.sync()

        def write_paths():
            with torch.cuda.stream(stream):
                acts[:, 0].copy_(torch.as_tensor(paths, device=acts.device))
            env.sync()

        # actions and table against the restatement
        n_chk = min(args.check, n)
        avail = ar.unpack_slots(env.slots_packed()[:n_chk], env.topology.n_links, S, ar.row_words(S))
        prep = ar.Prepared(env.ENV_TYPE, avail, services[:n_chk], env.topology, K, S)
        links = rr.Links(avail, services[:n_chk], env.topology)
        mismatched, rejects = {}, {}
        for rule in rr.RULES:
            want_tab = rr.table(prep, links, rule)
            for route in rr.ROUTES:
                got, tab = env.route_spectrum(rule, route, table=True)
                bad = (got[:n_chk] != rr.route(want_tab, route, K, S)).any(axis=1) | (tab[:n_chk] != want_tab).any(axis=(1, 2))
                mismatched["%s_%s" % (rule, route)] = int(bad.sum())
                rejects["%s_%s" % (rule, route)] = round(float((got[:, 0] == K).mean()), 4)

        fns = {"mask_joint": lambda: env.action_mask("joint", fetch=False)}
        for rule in rr.RULES:
            for route in rr.ROUTES:
                fns["%s_%s" % (rule, route)] = lambda rule=rule, route=route: env.route_spectrum(rule, route, fetch=False)
            if rule != "min_cuts":
                for g in (0, 1):
                    fns["assign_%s_g%d" % (rule, g)] = lambda rule=rule, g=g: env.assign_spectrum(rule, n_given=g, fetch=False)
        us = {k: [] for k in fns}
        for _ in range(2):  # alternated
            for k, fn in fns.items():
                write_paths()  # (every launch overwrites the row: each window starts from the same paths again)
                graph = graph_of(fn, stream)
                ms, reps = time_window(graph.replay, stream, args.window / 2)
                us[k].append(1e3 * ms / (reps * 50))
                del graph
        best = {k: round(min(v), 2) for k, v in us.items()}
        # the table without this kernel: k launches of assign_spectrum(rule, n_given=1)
        over_k = {rule: round(max(best["%s_%s" % (rule, route)] for route in rr.ROUTES) / (K * best["assign_%s_g1" % rule]), 3) for rule in ar.RULES}
        rec = dict(workload=wl, family=fam, envs=n, links=int(env.topology.n_links), slots=S, k=K, us_per_launch_back_to_back=best,
                   us_per_launch_back_to_back_all={k: [round(x, 2) for x in v] for k, v in us.items()},
                   route_over_k_times_assign_g1=over_k, device_vs_restatement_mismatched_rows=mismatched, rows_checked=n_chk,
                   reject_share=rejects, device=torch.cuda.get_device_name(env.device_id), time=time.strftime("%Y-%m-%d %H:%M:%S"))
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
