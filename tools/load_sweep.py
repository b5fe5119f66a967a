#!/usr/bin/env python3
"""A blocking-against-load curve from ONE batch: L loads x R seeds, env i at load i % L (per-env traffic load, include/orl.h
orl_batch_create_with_rates).  Default: cfg2 of bench.py's WORKLOADS, 16 loads from 100 to 400 Erlang x 4 096 seeds under the
workload's heuristic.  Prints the service blocking per load (a host reduction of counters()) and env-steps/s; with --compare the
same sweep as L consecutive R-env batches, one load each.

usage: tools/load_sweep.py [--workload cfg2] [--loads 16] [--lo 100] [--hi 400] [--seeds 4096] [--steps 1000] [--warmup 300]
                           [--compare] [--uniform]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def blocking(counters):
    """service blocking over the batch's envs: 1 - accepted / processed (counters() columns 1 and 0)."""
    c = np.asarray(counters, np.float64)
    return 1.0 - c[:, 1].sum() / c[:, 0].sum()


def timed_run(env, policy, warmup, steps):
    env.run(policy, warmup)
    c0 = env.counters()
    t0 = time.perf_counter()
    env.run(policy, steps)
    dt = time.perf_counter() - t0
    return env.counters() - c0, dt


def main():
    import optical_rl_gym_amd as orl
    from bench import WORKLOADS

    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS))
    ap.add_argument("--loads", type=int, default=16)
    ap.add_argument("--lo", type=float, default=100.0)
    ap.add_argument("--hi", type=float, default=400.0)
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--compare", action="store_true", help="also run the sweep as one batch per load, one after the other")
    ap.add_argument("--uniform", action="store_true", help="also time a uniform batch of the same size at the mean load")
    args = ap.parse_args()
    fam, topo, kw, policy = WORKLOADS[args.workload]
    kw = {k: v for k, v in kw.items() if k != "load"}
    if fam == "DeepRMSA":
        raise SystemExit("DeepRMSA takes mean_service_inter_arrival_time instead of load: sweep it through that argument")
    L, R = args.loads, args.seeds
    loads = np.linspace(args.lo, args.hi, L)
    # one pending-release capacity — the one the largest load needs — for every batch of both variants: the capacity is part of
    # the specialisation's key, so the one-batch-per-load variant would otherwise build a specialised kernel per load
    kw["event_capacity"] = int(loads.max() + 10.0 * np.sqrt(loads.max()) + 64.0)
    n = L * R
    seeds = [10 + i for i in range(n)]
    out = dict(workload=args.workload, loads=[float(x) for x in loads], seeds_per_load=R, steps=args.steps, warmup=args.warmup)

    t0 = time.perf_counter()
    env = orl.make(fam, topology=topo, num_envs=n, seeds=seeds, load=loads[np.arange(n) % L], **kw)
    t_make = time.perf_counter() - t0
    d, dt = timed_run(env, policy, args.warmup, args.steps)
    env.close()
    curve = [blocking(d[li::L]) for li in range(L)]
    out["one_batch"] = dict(envs=n, create_s=round(t_make, 3), run_s=round(dt, 4), env_steps_per_s=round(n * args.steps / dt, 1),
                            wall_s=round(time.perf_counter() - t0, 3), blocking=[round(float(b), 6) for b in curve])
    print("load  service blocking")
    for ld, b in zip(loads, curve):
        print("%6.1f  %.5f" % (ld, b))
    print("one batch of %d envs: %.3e env-steps/s (%.3f s for %d steps; %.2f s with construction and warm-up)"
          % (n, n * args.steps / dt, dt, args.steps, out["one_batch"]["wall_s"]))

    if args.uniform:
        env = orl.make(fam, topology=topo, num_envs=n, seeds=seeds, load=float(loads.mean()), **kw)
        _d, dtu = timed_run(env, policy, args.warmup, args.steps)
        env.close()
        out["uniform_mean_load"] = dict(load=float(loads.mean()), run_s=round(dtu, 4), env_steps_per_s=round(n * args.steps / dtu, 1))
        print("uniform batch at the mean load %.1f: %.3e env-steps/s (the mixed-load batch takes %.3f of its time)"
              % (loads.mean(), n * args.steps / dtu, dt / dtu))

    if args.compare:
        t0 = time.perf_counter()
        run_s, curve2 = 0.0, []
        for li in range(L):
            env = orl.make(fam, topology=topo, num_envs=R, seeds=seeds[li::L], load=float(loads[li]), **kw)
            d, dt1 = timed_run(env, policy, args.warmup, args.steps)
            env.close()
            run_s += dt1
            curve2.append(blocking(d))
        wall = time.perf_counter() - t0
        out["batch_per_load"] = dict(envs=R, run_s=round(run_s, 4), env_steps_per_s=round(n * args.steps / run_s, 1), wall_s=round(wall, 3),
                                     blocking=[round(float(b), 6) for b in curve2])
        same = [float(a) == float(b) for a, b in zip(curve, curve2)]
        print("%d batches of %d envs, one after the other: %.3e env-steps/s (%.3f s for the timed steps, %.2f s in all); curves %s"
              % (L, R, n * args.steps / run_s, run_s, wall, "identical" if all(same) else "DIFFER"))
        print("one batch is %.2fx faster on the timed steps, %.2fx on the whole sweep"
              % (run_s / out["one_batch"]["run_s"], wall / out["one_batch"]["wall_s"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
