#!/usr/bin/env python3
"""Cost of the path-feature observation (include/orl.h, orl_batch_path_features; k_path_features in csrc/orl_path_obs.h) at steady
state, beside the action mask of the same batch.

For each configuration (cfg2 and cfg3: 65 536 envs; cfg4n: 16 384, the batch its benchmark runs, at j = 1), after 300 warm-up steps
of the family's heuristic on the device:
  * us per launch from HIP events over a window of >= 1 s, for k_path_features and for the action mask ("joint"; RMCSA, which has
    no joint mask: "path_modulation"), alternated in the same command:
      - back to back: launches replayed from a captured graph of 50 of them (no host launch cost).  Nothing touches the slot maps in
        between, so slot maps and rows can stay in the 256 MB MALL (Infinity Cache): a lower bound, not an HBM figure;
      - in the loop: `policy_step(fetch=False)` + the launch per step against `policy_step` alone — the cost where an agent uses
        it, after a step kernel that rewrote slot maps, records and the step's other outputs;
  * DeepRMSA (cfg3): the other device route to the same numbers — the float64 observation the step kernel keeps current, cast to
    float32 by torch (`obs.float()` into a preallocated tensor), back to back; `observation()` is called --obs-calls times so that
    a kernel trace (rocprofv3 --kernel-trace --stats) of this command shows k_obs8's own time, which this tool cannot launch alone;
  * bytes written, from shapes: n_envs x pitch x 4; a bound on the bytes read: block rows x hops x row words x 8 (every core's rows
    of every path of the pending pair; the path records and slot tables are L2-resident and not counted);
  * the device's rows against the restatement (tests/path_features_restate.py) on the first --check envs.
Writes the results as JSON lines to --out (default: stdout only).

    python tools/path_obs_rate.py [--envs 65536] [--rmcsa-envs 16384] [--j 1] [--warmup 300] [--window 1.0] [--out FILE] [--only cfg2,cfg3,cfg4n]
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
from tests import path_features_restate as pf  # noqa: E402
from tests import rmcsa_mask_restate as rr  # noqa: E402

CASES = ("cfg2", "cfg3", "cfg4n")


def bytes_model(env, j):
    dim, rows, pitch = env.path_features_shape(j)
    svc, t = env.services(), env.topology
    src, dst = svc[:, 2].astype(int), svc[:, 3].astype(int)
    hops = np.where(np.arange(env.k_paths)[None, :] < t.n_paths[src, dst][:, None], t.path_hops[src, dst], 0).sum()
    cores = env.num_spatial_resources if env.ENV_TYPE == 3 else 1
    return env.num_envs * pitch * 4, int(hops) * cores * env.lib.orl_batch_row_words(env._h) * 8


def graph_of(fn, stream, n=50):
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(n):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rmcsa-envs", type=int, default=16384)
    ap.add_argument("--j", type=int, default=1, help="blocks per row (cfg3: the batch's own j, so that the rows are its observation)")
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--check", type=int, default=2048)
    ap.add_argument("--obs-calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated: " + ",".join(CASES))
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else None
    lines = []
    for wl in CASES:
        if only and wl not in only:
            continue
        fam, topo, kw, pol = WORKLOADS[wl]
        n_envs = args.rmcsa_envs if fam == "RMCSA" else args.envs
        env = orl.make(fam, topology=topo, num_envs=n_envs, seeds=list(range(1, 1 + n_envs)), **kw)
        env.run(pol, args.warmup)
        j = env.j if fam == "DeepRMSA" else args.j
        layout = "path_modulation" if fam == "RMCSA" else "joint"
        dim, rows, pitch = env.path_features_shape(j)
        got = env.path_features(j)  # (also allocates the buffer before the capture)
        env.action_mask(layout, fetch=False)
        n_chk = min(args.check, n_envs)
        env_type, avail, services = env.ENV_TYPE, rr.unpack_cores(env.slots_packed()[:n_chk], env.num_spatial_resources, env.topology.n_links,
                                                                  env.num_spectrum_resources), env.services()[:n_chk]
        want = np.float32(pf.restate_fast(env_type, avail, services, env.topology, j, rr.tables_of(env) if fam == "RMCSA" else None))
        mismatched = int((got[:n_chk].view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())
        stream = env.torch_stream()

        def feat():
            env.path_features(j, fetch=False)

        def mask():
            env.action_mask(layout, fetch=False)

        def step_only():
            env.policy_step(pol, auto_reset=True, fetch=False)

        def step_feat():
            env.policy_step(pol, auto_reset=True, fetch=False)
            env.path_features(j, fetch=False)

        def step_mask():
            env.policy_step(pol, auto_reset=True, fetch=False)
            env.action_mask(layout, fetch=False)

        g_feat, g_mask = graph_of(feat, stream), graph_of(mask, stream)
        us = {"feat": [], "mask": []}
        for _ in range(2):  # alternated
            for key, g in (("feat", g_feat), ("mask", g_mask)):
                ms, reps = time_window(g.replay, stream, args.window / 2)
                us[key].append(1e3 * ms / (reps * 50))
        del g_feat, g_mask
        loop = {"step": [], "feat": [], "mask": []}
        for _ in range(2):
            for key, fn in (("step", step_only), ("feat", step_feat), ("mask", step_mask)):
                ms, reps = time_window(fn, stream, args.window / 2)
                loop[key].append(1e3 * ms / reps)
        us_step = min(loop["step"])
        rec = dict(workload=wl, family=fam, envs=n_envs, j=j, dim=dim, rows=rows, pitch_floats=pitch, mask_layout=layout,
                   us_per_launch_back_to_back=round(min(us["feat"]), 2), us_per_launch_back_to_back_all=[round(x, 2) for x in us["feat"]],
                   mask_us_per_launch_back_to_back=round(min(us["mask"]), 2), mask_us_per_launch_back_to_back_all=[round(x, 2) for x in us["mask"]],
                   us_per_step_policy_step=round(us_step, 2), us_added_per_step_in_loop=round(min(loop["feat"]) - us_step, 2),
                   mask_us_added_per_step_in_loop=round(min(loop["mask"]) - us_step, 2))
        written, read_bound = bytes_model(env, j)
        rec.update(bytes_written=written, bytes_read_bound=read_bound,
                   tb_per_s_back_to_back=round((written + read_bound) / (min(us["feat"]) * 1e-6) / 1e12, 3),
                   device_vs_restatement_mismatched_rows=mismatched, rows_checked=n_chk)
        if fam == "DeepRMSA":
            obs = env.device_tensor("obs")
            f32 = torch.empty(obs.shape, dtype=torch.float32, device=obs.device)
            with torch.cuda.stream(stream):
                f32.copy_(obs)
            g_cast = graph_of(lambda: f32.copy_(obs), stream)
            ms, reps = time_window(g_cast.replay, stream, args.window / 2)
            rec["f32_cast_of_obs_us_back_to_back"] = round(1e3 * ms / (reps * 50), 2)
            del g_cast
            for _ in range(args.obs_calls):
                env.observation()
        rec.update(device=torch.cuda.get_device_name(env.device_id), time=time.strftime("%Y-%m-%d %H:%M:%S"))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        env.check()
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
