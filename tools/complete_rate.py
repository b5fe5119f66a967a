#!/usr/bin/env python3
"""Cost of the first-fit completion of partial RMCSA actions (include/orl.h, orl_batch_complete_actions; k_rmcsa_complete in
csrc/orl_rmcsa_complete.h) at steady state, beside the "path_modulation" action mask of the same batch.

On cfg4n (NSFNET, 7 cores x 320 slots; 16 384 envs, the batch its benchmark runs), after 300 warm-up steps of SAP_BM_FC_FF on the
device, for g = 0, 1, 2, 3 given columns (a prefix within reach where the pending service has one, read from the actions buffer) and
for the mask, alternated in the same command:
  * us per launch from HIP events over a window of >= 1 s, back to back: launches replayed from a captured graph of 50 of them (no
    host launch cost).  Nothing touches the slot maps in between, so they can stay in the 256 MB MALL (Infinity Cache): a lower
    bound, not an HBM figure;
  * in the loop, the cost where an agent uses them, after a step kernel that rewrote slot maps and records: the mask +
    `policy_step("SAP_BM_FC_FF", fetch=False)` against policy_step alone; the g = 0 completion + `step(None, fetch=False)` against
    policy_step (the step with the heuristic's slot scan as its first phase) and against the step of actions already in the buffer;
    for g = 1, 2, 3 the g = 0 completion, then the completion of its own first g columns, then the step, against the g = 0 loop;
  * the device's rows against the restatement (tests/complete_restate.py) on the first --check envs.
The expectation: the completion reads at most the link rows the "path_modulation" mask reads and writes 16 B per env, so
its launch should not exceed the mask's.  Writes the results as JSON lines to --out (default: stdout only).

    python tools/complete_rate.py [--envs 16384] [--warmup 300] [--window 1.0] [--check 1024] [--out FILE]
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
from tests import complete_restate as cr  # noqa: E402
from tests import rmcsa_mask_restate as rr  # noqa: E402


def prefix_in_reach(env, tab, rng):
    """[n, 3]: per env a (path, modulation) within reach where the pending service has one (else (0, 0)) and a core"""
    reach = cr.reach_of(env.services(), env.topology, tab)
    n, K, M = reach.shape
    score = np.where(reach.reshape(n, K * M), rng.random((n, K * M)), -1.0)
    col = score.argmax(axis=1)
    return np.stack([col // M, col % M, rng.integers(0, env.num_spatial_resources, n)], axis=1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--check", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    fam, topo, kw, pol = WORKLOADS["cfg4n"]
    n = args.envs
    env = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
    env.run(pol, args.warmup)
    tab = rr.tables_of(env)
    rng = np.random.default_rng(0)
    stream = env.torch_stream()
    acts = env.device_tensor("actions")
    env.action_mask("path_modulation", fetch=False)  # (allocates the buffer before the capture)
    env.complete_actions(n_given=0, fetch=False)
    env.sync()

    def write_prefix():
        pre = prefix_in_reach(env, tab, rng)
        with torch.cuda.stream(stream):
            acts[:, :3].copy_(torch.as_tensor(pre, device=acts.device))
        env.sync()
        return pre

    # the rows against the restatement
    n_chk = min(args.check, n)
    pre = write_prefix()
    avail = rr.unpack_cores(env.slots_packed()[:n_chk], env.num_spatial_resources, env.topology.n_links, env.num_spectrum_resources)
    pv = rr.prov_all(avail, env.services()[:n_chk], env.topology, tab)
    mismatched, rejects = {}, {}
    for g in range(4):
        got = env.complete_actions(given=pre[:, :g] if g else None, n_given=g)
        want = cr.complete(pv, env.services()[:n_chk], env.topology, tab, g, pre[:n_chk])
        mismatched[g] = int((got[:n_chk] != want).any(axis=1).sum())
        rejects[g] = round(float((got[:, 0] == env.k_paths).mean()), 4)
    write_prefix()

    def mask():
        env.action_mask("path_modulation", fetch=False)

    def complete(g):
        return lambda: env.complete_actions(n_given=g, fetch=False)

    keys = ["mask"] + ["g%d" % g for g in range(4)]
    fns = dict(mask=mask, **{"g%d" % g: complete(g) for g in range(4)})
    graphs = {k: graph_of(fns[k], stream) for k in keys}
    us = {k: [] for k in keys}
    for _ in range(2):  # alternated
        for k in keys:
            write_prefix()  # (a completion overwrites the row: each window starts from a prefix within reach again)
            ms, reps = time_window(graphs[k].replay, stream, args.window / 2)
            us[k].append(1e3 * ms / (reps * 50))
    del graphs

    def step_only():
        env.step(None, auto_reset=True, fetch=False)

    def policy_step():
        env.policy_step(pol, auto_reset=True, fetch=False)

    def step_mask():
        env.policy_step(pol, auto_reset=True, fetch=False)
        env.action_mask("path_modulation", fetch=False)

    def step_complete(g):
        def fn():
            env.complete_actions(n_given=0, fetch=False)  # (g >= 1: the prefix of the launch under test is this completion's)
            if g:
                env.complete_actions(n_given=g, fetch=False)
            env.step(None, auto_reset=True, fetch=False)
        return fn

    loop_fns = dict(policy_step=policy_step, mask=step_mask, **{"g%d" % g: step_complete(g) for g in range(4)})
    loop = {k: [] for k in loop_fns}
    for _ in range(2):
        for k, fn in loop_fns.items():
            ms, reps = time_window(fn, stream, args.window / 2)
            loop[k].append(1e3 * ms / reps)
    # the step of actions that are already in the buffer (whatever the last loop left, stepped again: mostly refused, so a lower
    # bound of the step the completions are followed by)
    ms, reps = time_window(step_only, stream, args.window / 2)
    us_step_only = 1e3 * ms / reps
    us_pstep = min(loop["policy_step"])
    rec = dict(workload="cfg4n", family=fam, envs=n, cores=env.num_spatial_resources, slots=env.num_spectrum_resources,
               us_per_launch_back_to_back={k: round(min(v), 2) for k, v in us.items()},
               us_per_launch_back_to_back_all={k: [round(x, 2) for x in v] for k, v in us.items()},
               us_per_step_policy_step=round(us_pstep, 2), us_per_step_step_only=round(us_step_only, 2),
               us_per_step_in_loop={k: round(min(v), 2) for k, v in loop.items()},
               mask_us_added_per_step_in_loop=round(min(loop["mask"]) - us_pstep, 2),
               complete_g0_plus_step_minus_policy_step_us=round(min(loop["g0"]) - us_pstep, 2),
               complete_g0_us_added_per_step_in_loop=round(min(loop["g0"]) - us_step_only, 2),
               complete_us_added_per_step_in_loop={"g%d" % g: round(min(loop["g%d" % g]) - min(loop["g0"]), 2) for g in (1, 2, 3)},
               completion_not_slower_than_mask={"g%d" % g: bool(min(us["g%d" % g]) <= min(us["mask"])) for g in range(4)},
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
