#!/usr/bin/env python3
"""Cost and content of the action masks (include/orl.h, orl_batch_action_mask; k_action_mask in csrc/orl_mask.h, k_rmcsa_mask in
csrc/orl_rmcsa_mask.h) at steady state.

For each configuration: 65 536 envs (RMCSA's two-stage layouts: 16 384, the batch its benchmark runs), 300 warm-up steps of the
family's heuristic on the device, then
  * us per mask launch from HIP events over a window of >= 1 s, three ways:
      - back to back: launches replayed from a captured graph of 50 of them (no host launch cost).  Nothing touches the slot maps in
        between, so a cfg2 batch's ~115 MB of slot maps and the 106 MB of rows can stay in the 256 MB MALL (Infinity Cache): this
        is a lower bound, not an HBM figure;
      - eager: launches issued one by one from Python (what `action_mask(fetch=False)` costs an eager loop);
      - in the loop: `policy_step(fetch=False)` + `action_mask(fetch=False)` per step against `policy_step` alone — the mask's
        cost where an agent uses it, after a step kernel that rewrote slot maps, records and the step's other outputs;
  * the bytes model of one launch: the mask rows written (n_envs x pitch) + the two service-record words read per env + the link
    rows of every path of the pending pair (hops x row words x 8 B; the path records and slot tables are L2-resident and not
    counted; RMCSA: every core's rows of every path for "path_modulation", every core's rows of the one given path for "core_slot",
    whose pairs are the heuristic's: columns 0 and 1 of the actions buffer as policy_step left them), and the TB/s it gives at the back-to-back and the in-loop time, against 6.3 TB/s (what a streaming kernel achieves
    on MI355X) and the 8 TB/s spec;
  * the valid-action fraction: provisioning columns per row, from a host restatement of the read-back state WITHOUT the fallback
    (tests/mask_restate.py) — a mask row of all ones is either a fallback row or a row where every action provisions, and only
    the state tells them apart — and the share of rows with no provisioning action.  The device's mask is checked against the
    restatement (with the fallback) on every env.
Writes the results as JSON lines to --out (default: stdout only).

    python tools/mask_rate.py [--envs 65536] [--rmcsa-envs 16384] [--warmup 300] [--window 1.0] [--out profiles/mask_rate.jsonl] [--only cfg2_joint,...]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o mask -- python tools/mask_rate.py --window 0.2
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
from bench import WORKLOADS  # noqa: E402
from tests import rmcsa_mask_restate as rr  # noqa: E402
from tests.mask_restate import restate_fast, row_words, unpack_slots  # noqa: E402

ACHIEVABLE_TBS, SPEC_TBS = 6.3, 8.0
RMCSA_ENVS = 16384
CASES = [("cfg2_joint", "cfg2", "joint"), ("cfg2_path", "cfg2", "path"), ("cfg3_joint", "cfg3", "joint"), ("cfg1_joint", "cfg1", "joint"),
         ("cfg4n_path_modulation", "cfg4n", "path_modulation"), ("cfg4n_core_slot", "cfg4n", "core_slot")]


def given_pairs(env):
    """What "core_slot" reads with given=None: columns 0 and 1 of the actions buffer."""
    return env.device_tensor("actions")[:, :2].cpu().numpy().copy()


def bytes_model(env, pitch, layout):
    svc = env.services()
    t = env.topology
    src, dst = svc[:, 2].astype(int), svc[:, 3].astype(int)
    row_bytes = env.lib.orl_batch_row_words(env._h) * 8
    hops = np.where(np.arange(env.k_paths)[None, :] < t.n_paths[src, dst][:, None], t.path_hops[src, dst], 0)
    if layout == "core_slot":  # the given path alone, where it exists (a pair beyond reach loads nothing: not modelled, an upper bound)
        g = given_pairs(env)
        ok = (g[:, 0] >= 0) & (g[:, 0] < env.k_paths)
        hops = np.where(ok, hops[np.arange(len(g)), np.clip(g[:, 0], 0, env.k_paths - 1)], 0)
    hops = hops.sum() * env.num_spatial_resources
    written, records, rows = env.num_envs * pitch, env.num_envs * 16, int(hops) * row_bytes
    return written, records, rows


def restated(env, layout, fallback, chunk=8192):
    """The mask of the read-back state, restated on the host (with or without the fallback rows)."""
    packed, svc = env.slots_packed(), env.services()
    S = env.num_spectrum_resources
    cw = 50.0 if env.ENV_TYPE == 2 else 12.5
    parts = []
    if env.ENV_TYPE == 3:
        tab, given, C = rr.tables_of(env), given_pairs(env), env.num_spatial_resources
        for lo in range(0, env.num_envs, 512):
            avail = rr.unpack_cores(packed[lo:lo + 512], C, env.topology.n_links, S)
            parts.append(rr.restate_rmcsa_fast(avail, svc[lo:lo + 512], env.topology, tab, layout, given=given[lo:lo + 512],
                                               allow_rejection=env.allow_rejection, fallback=fallback))
        return np.concatenate(parts)
    for lo in range(0, env.num_envs, chunk):
        avail = unpack_slots(packed[lo:lo + chunk], env.topology.n_links, S, row_words(S))
        parts.append(restate_fast(env.ENV_TYPE, avail, svc[lo:lo + chunk], env.topology, env.k_paths, S, env.j, cw, env.allow_rejection,
                                  layout, fallback=fallback))
    return np.concatenate(parts)


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
    ap.add_argument("--rmcsa-envs", type=int, default=RMCSA_ENVS, help="envs of the RMCSA cases")
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated case names: " + ",".join(c[0] for c in CASES))
    args = ap.parse_args()
    only = set(args.only.split(",")) if args.only else None
    lines = []
    for name, wl, layout in CASES:
        if only and name not in only:
            continue
        fam, topo, kw, pol = WORKLOADS[wl]
        n_envs = args.rmcsa_envs if fam == "RMCSA" else args.envs
        env = orl.make(fam, topology=topo, num_envs=n_envs, seeds=list(range(1, 1 + n_envs)), **kw)
        env.run(pol, args.warmup)
        if fam == "RMCSA":
            env.policy(pol, fetch=False)  # the heuristic's (path, modulation) of the pending service into the actions buffer
        dim, pitch = env.action_mask_shape(layout)
        mask = env.action_mask(layout)  # (also allocates the buffer before the capture)
        raw = restated(env, layout, fallback=False)
        want = raw.copy()
        if not env.allow_rejection:
            want[~raw[:, :-1].any(axis=1), :-1] = True
        mismatched = int((mask != want).any(axis=1).sum())
        raw = raw[:, :-1]
        valid = float(raw.mean())
        none_row = float((~raw.any(axis=1)).mean())
        all_row = float(raw.all(axis=1).mean())
        stream = env.torch_stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(50):
                env.action_mask(layout, fetch=False)
        ms_g, reps_g = time_window(g.replay, stream, args.window)
        us_graph = 1e3 * ms_g / (reps_g * 50)
        del g
        ms_e, reps_e = time_window(lambda: env.action_mask(layout, fetch=False), stream, args.window)
        us_eager = 1e3 * ms_e / reps_e

        def step_only():
            env.policy_step(pol, auto_reset=True, fetch=False)

        def step_mask():
            env.policy_step(pol, auto_reset=True, fetch=False)
            env.action_mask(layout, fetch=False)

        ms_s, reps_s = time_window(step_only, stream, args.window)
        ms_sm, reps_sm = time_window(step_mask, stream, args.window)
        us_step = 1e3 * ms_s / reps_s
        us_loop = 1e3 * ms_sm / reps_sm - us_step
        written, records, rows = bytes_model(env, pitch, layout)
        total = written + records + rows
        tbs = total / (us_graph * 1e-6) / 1e12
        tbs_loop = total / (us_loop * 1e-6) / 1e12 if us_loop > 0 else None
        rec = dict(case=name, workload=wl, layout=layout, envs=n_envs, warmup_steps=args.warmup, dim=dim, pitch=pitch,
                   us_per_launch_back_to_back=round(us_graph, 2), us_per_launch_eager=round(us_eager, 2),
                   us_per_step_policy_step=round(us_step, 2), us_added_per_step_in_loop=round(us_loop, 2),
                   window_s=[round(x / 1e3, 3) for x in (ms_g, ms_e, ms_s, ms_sm)],
                   bytes_written=written, bytes_service_records=records, bytes_path_rows=rows, bytes_total=total,
                   tb_per_s_back_to_back=round(tbs, 3), share_of_achievable_back_to_back=round(tbs / ACHIEVABLE_TBS, 3),
                   tb_per_s_in_loop=None if tbs_loop is None else round(tbs_loop, 3),
                   share_of_achievable_in_loop=None if tbs_loop is None else round(tbs_loop / ACHIEVABLE_TBS, 3),
                   valid_action_fraction=round(valid, 5), rows_without_provisioning_action=round(none_row, 5),
                   rows_all_actions_provision=round(all_row, 5), device_vs_restatement_mismatched_rows=mismatched,
                   device=torch.cuda.get_device_name(env.device_id), time=time.strftime("%Y-%m-%d %H:%M:%S"))
        print("%-11s dim %5d: %6.2f us/launch back to back, %6.2f eager, +%6.2f us per step in the loop (step alone %.1f us); "
              "%.1f MB written + %.2f MB records + %.1f MB path rows = %.2f TB/s back to back (%.2f of %.1f), %s TB/s in the loop; "
              "valid actions %.4f, rows with none %.4f, rows with all %.4f; %d rows differ from the restatement"
              % (name, dim, us_graph, us_eager, us_loop, us_step, written / 1e6, records / 1e6, rows / 1e6, tbs, tbs / ACHIEVABLE_TBS,
                 ACHIEVABLE_TBS, "%.2f" % tbs_loop if tbs_loop else "-", valid, none_row, all_row, mismatched), flush=True)
        lines.append(rec)
        env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
