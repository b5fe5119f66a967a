#!/usr/bin/env python3
"""Cost of capacity_after (include/orl.h, orl_batch_capacity_after; k_capacity_after in csrc/orl_capacity_after.h) at steady state,
beside network_capacity("counts") on the same batch and beside the fork route that answers the same question without it.

On cfg2 (RMSA) and cfg1 (RWA) of bench.py at 65 536 envs, cfg4n (RMCSA, 7 cores x 320 slots) at 16 384 and cfg5 (RMSA on germany50) at
8 192, after a warm-up of the family's heuristic on the device (--warmup, 1 500 steps), in the same command:
  * capacity_after("route", "total"), ("route", "classes") and ("blocks", j = 4, "total"), and network_capacity("counts"): us per launch
    from HIP events over a window, back to back, replayed from a captured graph of --launches launches (no host launch cost), the cases
    alternated over two rounds, the minimum kept.  Nothing touches the state in between, so it can stay in the 256 MB MALL (Infinity
    Cache) where it fits: a lower bound, not an HBM figure;
  * the fork route on the same candidates, the scratch batch's time counted: copy_envs of every env into k C' children of a scratch
    batch of k C' x --fork-envs envs (--fork-envs roots: a scratch batch of k C' x 65 536 envs does not fit), policy_step on the
    children, network_capacity("counts") on them — wall time per decision of the --fork-envs roots, synchronised, scaled to the batch.
    On the RMSA workloads child p steps PATH_FF on path p; RWA and RMCSA have no per-path policy, so there every child steps the
    family's heuristic: the same launches on as many children, not the same candidates;
  * counted on the host from the restatement (tests/capacity_after_restate.py) on the first --check envs: the share of paths that
    share a link with a present route candidate (those recompute) and of pairs that own one (their cells are what can be re-tested),
    and the device's rows against the restatement.
Writes one JSON line per workload to --out (default: stdout only).

    python tools/capacity_after_rate.py [--envs 65536] [--rmcsa-envs 16384] [--ger-envs 8192] [--warmup 1500] [--window 0.3] [--check 4]
                                        [--fork-envs 1024] [--only cfg2,cfg1,cfg4n,cfg5] [--out FILE]
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
from tests import capacity_after_restate as car  # noqa: E402
from tests import capacity_restate as cap  # noqa: E402
from tests import rmcsa_mask_restate as mr  # noqa: E402


def route(env, fam, **kw):
    return env.route_cores("first", "ksp", **kw) if fam == "RMCSA" else env.route_spectrum("first", "ksp", **kw)


def fork_route(name, n_roots, args, roots):
    """Wall time per decision of n_roots roots through a scratch batch of k C' children each, the way examples/capacity_aware_rmsa.py
    does it: copy_envs + policy_step + network_capacity("counts"), synchronised"""
    fam, topo, kw, pol = WORKLOADS[name]
    R = roots.k_paths * (roots.num_spatial_resources if fam == "RMCSA" else 1)
    scratch = orl.make(fam, topology=topo, num_envs=n_roots * R, seeds=list(range(7, 7 + n_roots * R)), **kw)
    parent, child = np.repeat(np.arange(n_roots), R), np.arange(n_roots * R)
    paths = (np.tile(np.arange(R), n_roots) // (R // roots.k_paths)).astype(np.int32)
    step_pol = "PATH_FF" if fam == "RMSA" else pol  # (elsewhere the family's heuristic stands in for the cost of the children's step)
    times = []
    for i in range(args.fork_reps + 1):
        scratch.sync()
        t0 = time.perf_counter()
        scratch.copy_envs(parent, child, source=roots)
        if step_pol == "PATH_FF":
            scratch.policy_step(step_pol, auto_reset=True, fetch=False, paths=paths)
        else:
            scratch.policy_step(step_pol, auto_reset=True, fetch=False)
        scratch.network_capacity("counts", fetch=False)
        scratch.sync()
        if i:
            times.append(time.perf_counter() - t0)
    scratch.close()
    return 1e6 * min(times), R


def measure(name, n, args):
    fam, topo, kw, pol = WORKLOADS[name]
    env = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
    env.run(pol, args.warmup)
    stream = env.torch_stream()
    C, S = (env.num_spatial_resources if fam == "RMCSA" else 1), env.num_spectrum_resources
    R = env.k_paths * C
    # against the restatement, and the shares the delta scheme rests on
    n_chk = min(args.check, n)
    tab = mr.tables_of(env) if fam == "RMCSA" else None
    need = cap.need_table(fam, env.topology, cap.class_rates(fam, kw), tab)
    n_cls = need.shape[3]
    avail = mr.unpack_cores(env.slots_packed()[:n_chk], C, env.topology.n_links, S)
    table = route(env, fam, table=True)[1]
    cands = car.route_candidates(table[:n_chk], S)
    sv = env.services()[:n_chk]
    src, dst = sv[:, 2].astype(np.int64), sv[:, 3].astype(np.int64)
    want, share = car.after(avail, env.topology, need, src, dst, cands, chunk=1 if topo == "germany50" else car.CHUNK)
    got = env.capacity_after("route", "classes")[:n_chk].reshape(n_chk, R + 1, n_cls)
    mismatched = int((got != want).any(axis=(1, 2)).sum())
    tot = car.total(want)
    loss = np.where(tot[:, :-1] >= 0, tot[:, :-1] - tot[:, -1:], 0)
    fns = {"after_route_total": lambda: env.capacity_after("route", "total", fetch=False),
           "after_route_classes": lambda: env.capacity_after("route", "classes", fetch=False),
           "after_blocks_j4_total": lambda: env.capacity_after("blocks", "total", j=4, fetch=False),
           "capacity_counts": lambda: env.network_capacity("counts", fetch=False),
           "route_table": lambda: route(env, fam, fetch=False)}
    env.block_table(4, fetch=False)
    for fn in fns.values():  # (allocates the buffers before the capture)
        fn()
    env.sync()
    present = {"route": float((env.capacity_after("route", "total")[:, :-1] >= 0).mean()),
               "blocks_j4": float((env.capacity_after("blocks", "total", j=4)[:, :-1] >= 0).mean())}
    us = {k: [] for k in fns}
    for _ in range(2):  # alternated
        for k, fn in fns.items():
            graph = graph_of(fn, stream, args.launches)
            ms, reps = time_window(graph.replay, stream, args.window / 2)
            us[k].append(1e3 * ms / (reps * args.launches))
            del graph
    best = {k: min(v) for k, v in us.items()}
    n_fork = min(args.fork_envs, n)
    fork_us, _ = fork_route(name, n_fork, args, env)
    rec = dict(workload=name, family=fam, envs=n, nodes=int(env.topology.n_nodes), links=int(env.topology.n_links), slots=S, cores=C, k=env.k_paths,
               classes=n_cls, candidates=dict(route=R, blocks_j4=4 * R), present_share=present, warmup=args.warmup,
               us_per_launch_back_to_back={k: round(v, 2) for k, v in best.items()},
               us_per_launch_back_to_back_all={k: [round(x, 2) for x in v] for k, v in us.items()},
               counts_passes_equivalent=round(best["after_route_total"] / best["capacity_counts"], 2), counts_passes_of_a_full_recount=R + 1,
               fork_route=dict(roots=n_fork, children=n_fork * R, us_per_decision=round(fork_us, 1), us_scaled_to_the_batch=round(fork_us * n / n_fork, 1)),
               share_of_paths_that_recompute=round(share[0] / max(1, share[1]), 4), share_of_pairs_re_tested_at_most=round(share[2] / max(1, share[3]), 4),
               largest_loss_per_env_checked=[int(x) for x in loss.max(axis=1)], device_vs_restatement_mismatched_envs=mismatched, envs_checked=n_chk,
               device=torch.cuda.get_device_name(env.device_id), time=time.strftime("%Y-%m-%d %H:%M:%S"))
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
    ap.add_argument("--launches", type=int, default=10, help="launches per captured graph")
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--fork-envs", type=int, default=1024, help="roots of the fork route's measurement (its scratch batch has k C' times as many envs)")
    ap.add_argument("--fork-reps", type=int, default=3)
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
