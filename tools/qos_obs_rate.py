#!/usr/bin/env python3
"""Cost of MatrixObservationWithPaths on the device (include/orl.h, orl_batch_matrix_paths_observation; k_qos_matrix_obs in
csrc/orl_qos_obs.h) for QoSConstrainedRA at steady state.

For each configuration: 65 536 envs on NSFNET (22 links, k = 5), 300 warm-up steps of SAP-FF on the device, then
  * us per launch from HIP events over a window of >= 1 s:
      - back to back: launches replayed from a captured graph of 50 of them (no host launch cost);
      - in the loop: `policy_step(fetch=False)` + `matrix_observation_with_paths(fetch=False)` per step against `policy_step`
        alone — what the observation adds to a step of an agent on the device;
  * the bytes model of one launch: the rows written (n_envs x pitch) + per env the link counters and the two service-record
    words read (n_envs x (8 E + 16); path records and tables are L2-resident and not counted), and the TB/s it gives against
    6.3 TB/s (what a streaming kernel achieves on MI355X);
  * a check of 256 sampled envs against the numpy restatement (tests/qos_obs_restate.py).
Configurations: A = the reference notebook's (examples/stable_baselines3/QoSConstrainedRA.ipynb: S = 16, classes [0.5, 0.5],
rewards [10, 1], load 50, episodes of 100), rows of 139 MB, which may stay in the 256 MB MALL between launches; B =
tools/qos_step_rate.py's (S = 64, three classes, load 300), rows of 555 MB, more than the MALL holds: an HBM figure.
Writes the results as JSON lines to --out (default: stdout only).

    python tools/qos_obs_rate.py [--envs 65536] [--warmup 300] [--window 1.0] [--out profiles/qos_obs_rate.jsonl] [--only A,B]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o qobs -- python tools/qos_obs_rate.py --window 0.2
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402
from tests.qos_obs_restate import restate_fast  # noqa: E402

ACHIEVABLE_TBS = 6.3
CONFIGS = {
    "A": dict(load=50, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=16, num_service_classes=2,
              classes_arrival_probabilities=[0.5, 0.5], classes_reward=[10.0, 1.0], allow_rejection=True),
    "B": dict(load=300, mean_service_holding_time=25, episode_length=50, num_spectrum_resources=64, num_service_classes=3,
              classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[4.0, 2.0, 1.0], allow_rejection=True),
}


def time_window(fn, stream, window):
    """ms of `reps` calls of fn (each queues work on `stream`) from HIP events, repeated until the window is >= `window` seconds."""
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 8
    while True:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ev0.record(stream)
            for _ in range(reps):
                fn()
            ev1.record(stream)
        ev1.synchronize()
        ms = ev0.elapsed_time(ev1)
        if ms >= 1e3 * window:
            return ms, reps
        reps = max(reps * 2, int(reps * 1.2e3 * window / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names: " + ",".join(CONFIGS))
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else None
    lines = []
    for name, kw in CONFIGS.items():
        if only and name not in only:
            continue
        env = orl.make("QoSConstrainedRA", topology="nsfnet_chen", num_envs=args.envs, seeds=list(range(1, 1 + args.envs)), **kw)
        env.run("SAP_FF", args.warmup)
        dim, pitch = env.matrix_paths_obs_shape()
        env.matrix_observation_with_paths(fetch=False)  # (allocates the buffer before the capture)
        view = env.device_tensor("matrix_paths_obs")
        sample = np.sort(np.random.default_rng(0).choice(args.envs, 256, replace=False))
        spectrum = np.stack([env.spectrum(int(e)) for e in sample])
        pending = env.services()[sample, 2:5].astype(np.int64)
        want = restate_fast(spectrum, pending, env.topology, env.num_spectrum_resources, env.k_paths)
        mismatched = int((view[torch.as_tensor(sample, device=view.device)].cpu().numpy() != want).any(axis=1).sum())
        stream = env.torch_stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(50):
                env.matrix_observation_with_paths(fetch=False)
        ms_g, reps_g = time_window(g.replay, stream, args.window)
        us_graph = 1e3 * ms_g / (reps_g * 50)
        del g

        def step_only():
            env.policy_step("SAP_FF", auto_reset=True, fetch=False)

        def step_obs():
            env.policy_step("SAP_FF", auto_reset=True, fetch=False)
            env.matrix_observation_with_paths(fetch=False)

        ms_s, reps_s = time_window(step_only, stream, args.window)
        ms_so, reps_so = time_window(step_obs, stream, args.window)
        us_step = 1e3 * ms_s / reps_s
        us_loop = 1e3 * ms_so / reps_so - us_step
        E = env.topology.n_links
        written, read = args.envs * pitch, args.envs * (8 * E + 16)
        total = written + read
        tbs = total / (us_graph * 1e-6) / 1e12
        tbs_loop = total / (us_loop * 1e-6) / 1e12 if us_loop > 0 else None
        rec = dict(config=name, kwargs=kw, envs=args.envs, warmup_steps=args.warmup, links=E, k_paths=env.k_paths, dim=dim,
                   pitch=pitch, us_per_launch_back_to_back=round(us_graph, 2), us_per_step_policy_step=round(us_step, 2),
                   us_added_per_step_in_loop=round(us_loop, 2), window_s=[round(x / 1e3, 3) for x in (ms_g, ms_s, ms_so)],
                   bytes_written=written, bytes_read=read, bytes_total=total, tb_per_s_back_to_back=round(tbs, 3),
                   share_of_achievable_back_to_back=round(tbs / ACHIEVABLE_TBS, 3),
                   tb_per_s_in_loop=None if tbs_loop is None else round(tbs_loop, 3),
                   sampled_envs_checked=len(sample), device_vs_restatement_mismatched_rows=mismatched,
                   device=torch.cuda.get_device_name(env.device_id), time=time.strftime("%Y-%m-%d %H:%M:%S"))
        print("%s dim %5d pitch %5d: %7.2f us/launch back to back, +%7.2f us per step in the loop (policy_step alone %.1f us); "
              "%.1f MB written + %.1f MB read = %.2f TB/s back to back (%.2f of %.1f), %s TB/s in the loop; %d of %d sampled rows "
              "differ from the restatement"
              % (name, dim, pitch, us_graph, us_loop, us_step, written / 1e6, read / 1e6, tbs, tbs / ACHIEVABLE_TBS, ACHIEVABLE_TBS,
                 "%.2f" % tbs_loop if tbs_loop else "-", mismatched, len(sample)), flush=True)
        lines.append(rec)
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
