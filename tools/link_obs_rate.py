#!/usr/bin/env python3
"""Cost of the per-link feature observation (include/orl.h, orl_batch_link_features; k_link_features in csrc/orl_link_obs.h) at
steady state, beside the path features (j = 1) and the action mask of the same batch.

For each configuration (cfg2 and cfg3: 65 536 envs; cfg4n: 16 384, the batch its benchmark runs), after 300 warm-up steps of the
family's heuristic on the device:
  * us per launch from HIP events over windows of >= 0.25 s, for k_link_features, k_path_features (j = 1) and the action mask
    ("joint"; RMCSA, which has no joint mask: "path_modulation"), alternated in the same command:
      - back to back: launches replayed from a captured graph of 50 of them (no host launch cost).  Nothing touches the slot maps in
        between, so slot maps, link records and rows can stay in the 256 MB MALL (Infinity Cache): a lower bound, not an HBM figure;
      - in the loop: `policy_step(fetch=False)` + the launch per step against `policy_step` alone — the cost where an agent uses
        it, after a step kernel that rewrote slot maps, link records and the step's other outputs;
  * the bytes model beside each time: n_envs x pitch x 4 written; n_envs x (C E W 8 + 32 E) — every slot row and every link record,
    once — plus 32 bytes per path record of the pending pairs read;
  * the device's rows against the restatement (tests/link_features_restate.py) on the first --check envs.
Writes the results as JSON lines to --out (default: stdout only).

    python tools/link_obs_rate.py [--envs 65536] [--rmcsa-envs 16384] [--warmup 300] [--window 0.25] [--out FILE] [--only cfg2,cfg3,cfg4n]
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
from tests import link_features_restate as lf  # noqa: E402
from tests import rmcsa_mask_restate as rr  # noqa: E402

CASES = ("cfg2", "cfg3", "cfg4n")


def bytes_model(env):
    dim, rows, width, pitch = env.link_features_shape()
    svc, t = env.services(), env.topology
    n_paths = int(t.n_paths[svc[:, 2].astype(int), svc[:, 3].astype(int)].sum())
    per_env = rows * env.lib.orl_batch_row_words(env._h) * 8 + 32 * t.n_links
    return env.num_envs * pitch * 4, env.num_envs * per_env + 32 * n_paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rmcsa-envs", type=int, default=16384)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--check", type=int, default=2048)
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
        layout = "path_modulation" if fam == "RMCSA" else "joint"
        dim, rows, width, pitch = env.link_features_shape()
        got = env.link_features()  # (also allocates the buffer before the capture)
        env.path_features(1, fetch=False)
        env.action_mask(layout, fetch=False)
        n_chk = min(args.check, n_envs)
        avail = rr.unpack_cores(env.slots_packed()[:n_chk], env.num_spatial_resources, env.topology.n_links, env.num_spectrum_resources)
        want = np.float32(lf.restate_fast(env.ENV_TYPE, avail, env.services()[:n_chk], env.topology, env.link_stats_all()[:n_chk]))
        mismatched = int((got[:n_chk].view(np.uint32) != want.view(np.uint32)).any(axis=1).sum())
        stream = env.torch_stream()
        views = {"link": lambda: env.link_features(fetch=False), "path": lambda: env.path_features(1, fetch=False),
                 "mask": lambda: env.action_mask(layout, fetch=False)}

        def step_and(view):
            def fn():
                env.policy_step(pol, auto_reset=True, fetch=False)
                if view:
                    view()
            return fn

        graphs = {key: graph_of(fn, stream) for key, fn in views.items()}
        us = {key: [] for key in views}
        for _ in range(2):  # alternated
            for key, g in graphs.items():
                ms, reps = time_window(g.replay, stream, args.window)
                us[key].append(1e3 * ms / (reps * 50))
        del graphs
        loop = {key: [] for key in ("step", "link", "path", "mask")}
        for _ in range(2):
            for key in loop:
                ms, reps = time_window(step_and(views.get(key)), stream, args.window)
                loop[key].append(1e3 * ms / reps)
        us_step = min(loop["step"])
        written, read = bytes_model(env)
        rec = dict(workload=wl, family=fam, envs=n_envs, dim=dim, rows=rows, width=width, pitch_floats=pitch, mask_layout=layout,
                   us_per_launch_back_to_back=round(min(us["link"]), 2), us_per_launch_back_to_back_all=[round(x, 2) for x in us["link"]],
                   path_features_j1_us_per_launch_back_to_back=round(min(us["path"]), 2),
                   mask_us_per_launch_back_to_back=round(min(us["mask"]), 2),
                   us_per_step_policy_step=round(us_step, 2), us_added_per_step_in_loop=round(min(loop["link"]) - us_step, 2),
                   path_features_j1_us_added_per_step_in_loop=round(min(loop["path"]) - us_step, 2),
                   mask_us_added_per_step_in_loop=round(min(loop["mask"]) - us_step, 2),
                   bytes_written=written, bytes_read=read,
                   tb_per_s_back_to_back=round((written + read) / (min(us["link"]) * 1e-6) / 1e12, 3),
                   tb_per_s_in_loop=round((written + read) / (max(min(loop["link"]) - us_step, 1e-3) * 1e-6) / 1e12, 3),
                   device_vs_restatement_mismatched_rows=mismatched, rows_checked=n_chk,
                   build_flags=os.environ.get("ORL_HIPCC_EXTRA", ""), device=torch.cuda.get_device_name(env.device_id),
                   time=time.strftime("%Y-%m-%d %H:%M:%S"))
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
