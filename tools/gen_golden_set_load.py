#!/usr/bin/env python3
"""Fixtures of set_load (optical_network_env.py:76-94), captured by running the reference's own envs where the reference is
importable (test infrastructure, data only; never runs on a GPU machine).

One trace per env family on NSFNET under the family's shortest-available-path first-fit heuristic, recorded by the recorders
of oracle/gen_golden.py (run_trace) and oracle/gen_golden_qos.py (record), unchanged and by import.  The policy handed to them
is a closure that counts its calls, calls env.set_load(**schedule[t]) when step t is in the schedule, and then returns the
reference heuristic's action: both recorders note the pending service before they ask for the action, and set_load does not
touch it, so the services drawn from step t on are the first to see the new rates.  The schedule is stored beside `meta` as a
JSON string ({step: {load / mean_service_holding_time}}).  Every trace is checked to differ from the same run without the
schedule from the first change on (arrival times), so that a fixture cannot be reproduced by ignoring set_load.

  tests/golden/s1_rmsa_set_load.npz       seed 10, S = 320, load 150 -> 400 -> (250, holding time 10) -> 60, 1 500 steps
  tests/golden/s1_deeprmsa_set_load.npz   the g4 configuration (j = 1), 600 steps
  tests/golden/s1_rwa_set_load.npz        the g5 configuration, 600 steps
  tests/golden/s1_rmcsa_set_load.npz      the g6 test configuration, 600 steps
  tests/golden/s1_qos_set_load.npz        the q1 configuration, 600 steps

Usage:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python3 -W ignore <repo>/tools/gen_golden_set_load.py
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_qos as gq  # noqa: E402  (the reference, repaired at import time)

qos, gg = gq.qos, gq.gg
gym, rmsa_env, deeprmsa_env, rwa_env, rmcsa_env = gg.gym, gg.rmsa_env, gg.deeprmsa_env, gg.rwa_env, gg.rmcsa_env


def scheduled(heuristic, schedule, seen):
    """The policy of run_trace: set_load at the scheduled steps, then the reference heuristic.  `seen` collects, per change,
    what the env holds afterwards (load, mean_service_holding_time, mean_service_inter_arrival_time)."""
    calls = [0]

    def policy(env):
        t = calls[0]
        calls[0] += 1
        if t in schedule:
            env.set_load(**schedule[t])
            seen[t] = (float(env.load), float(env.mean_service_holding_time), float(env.mean_service_inter_arrival_time))
        return heuristic(env)

    return policy


def with_schedule(name, schedule, record_one):
    """record_one(name, schedule, seen) writes <GOLD>/<name>.npz; the same run without the schedule goes to a scratch directory
    and must differ from the first change on.  The schedule and what the env held after each change are added to the file."""
    gold = gg.GOLD
    seen = {}
    record_one(name, schedule, seen)
    with tempfile.TemporaryDirectory() as tmp:
        gg.GOLD = tmp
        try:
            record_one(name, {}, {})
        finally:
            gg.GOLD = gold
        plain = dict(np.load(os.path.join(tmp, name + ".npz")))
    path = os.path.join(gold, name + ".npz")
    got = dict(np.load(path))
    first = min(schedule)
    # svc[t] is the service pending before step t; the one drawn by step `first` is the first to use the new rates
    assert np.array_equal(got["svc"][: first + 1], plain["svc"][: first + 1]), name
    assert got["svc"][first + 1, 0] != plain["svc"][first + 1, 0], name
    assert not np.array_equal(got["svc"][first + 1:, 0], plain["svc"][first + 1:, 0]), name
    assert sorted(seen) == sorted(schedule), name
    got["schedule"] = np.array(json.dumps({str(t): schedule[t] for t in sorted(schedule)}))
    got["after_change"] = np.array([[t] + list(seen[t]) for t in sorted(seen)], np.float64)
    np.savez_compressed(path, **got)
    print("%-24s %6d bytes  max pending %4d  changes %s" % (name, os.path.getsize(path), int(got["n_active"].max()), sorted(schedule)))


def main():
    nsf = gg.load_topology("nsfnet_chen")

    kw = dict(seed=10, load=150, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=320, allow_rejection=True)
    sched = {300: dict(load=400), 700: dict(load=250, mean_service_holding_time=10.0), 1100: dict(load=60)}
    with_schedule("s1_rmsa_set_load", sched, lambda name, sc, seen, kw=kw: gg.run_trace(
        name, gym.make("RMSA-v0", topology=nsf, **kw), policy=scheduled(rmsa_env.shortest_available_path_first_fit, sc, seen),
        n_steps=1500, info_keys=gg.RMSA_INFO, meta=dict(env="RMSA", topology="nsfnet_chen", kwargs=kw, policy="SAP_FF")))

    kw = dict(seed=10, allow_rejection=False, mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=1,
              episode_length=50, node_request_probabilities=gg.DEEPRMSA_NODE_PROBS)
    sched = {150: dict(load=140), 300: dict(mean_service_holding_time=10.0), 450: dict(load=60)}
    with_schedule("s1_deeprmsa_set_load", sched, lambda name, sc, seen, kw=kw: gg.run_trace(
        name, gym.make("DeepRMSA-v0", topology=nsf, **dict(kw, node_request_probabilities=np.array(gg.DEEPRMSA_NODE_PROBS))),
        policy=scheduled(deeprmsa_env.shortest_available_path_first_fit, sc, seen), n_steps=600, info_keys=gg.RMSA_INFO,
        obs_fn=lambda e: e.observation(), meta=dict(env="DeepRMSA", topology="nsfnet_chen", kwargs=kw, policy="SAP")))

    kw = dict(seed=10, allow_rejection=True, load=450, mean_service_holding_time=25, episode_length=1000)
    sched = {150: dict(load=600), 300: dict(mean_service_holding_time=12.5), 450: dict(load=200)}
    with_schedule("s1_rwa_set_load", sched, lambda name, sc, seen, kw=kw: gg.run_trace(
        name, gym.make("RWA-v0", topology=nsf, **kw), policy=scheduled(rwa_env.shortest_available_path_first_fit, sc, seen),
        n_steps=600, info_keys=gg.RWA_INFO, snapshot_every=300,
        vec_info_keys=("path_action_probability", "wavelength_action_probability"),
        meta=dict(env="RWA", topology="nsfnet_chen", kwargs=kw, policy="SAP_FF")))

    kw = dict(seed=10, allow_rejection=True, load=250, mean_service_holding_time=25, episode_length=1000,
              num_spectrum_resources=64, num_spatial_resources=7, worst_xt=-84.7)
    sched = {150: dict(load=400), 300: dict(mean_service_holding_time=40.0), 450: dict(load=120)}
    # (RMCSAEnv.__init__ changes the Modulation objects of the topology it is given: a freshly loaded one per env)
    with_schedule("s1_rmcsa_set_load", sched, lambda name, sc, seen, kw=kw: gg.run_trace(
        name, gym.make("RMCSA-v0", topology=gg.load_topology("nsfnet_chen"), **kw),
        policy=scheduled(rmcsa_env.shortest_available_path_best_modulation_first_core_first_fit, sc, seen), n_steps=600,
        info_keys=gg.RMCSA_INFO, snapshot_every=300,
        meta=dict(env="RMCSA", topology="nsfnet_chen", kwargs=kw, policy="SAP_BM_FC_FF")))

    kw = dict(seed=31, load=1000, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=40,
              num_service_classes=3, classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0],
              allow_rejection=True)
    sched = {150: dict(load=1400), 300: dict(mean_service_holding_time=20.0), 450: dict(load=500)}

    def record_qos(name, sc, seen, kw=kw):
        pol = scheduled(qos.shortest_available_path, sc, seen)
        gq.record(name, dict(kw), lambda env, t: pol(env), 600, "SAP_FF")

    with_schedule("s1_qos_set_load", sched, record_qos)


if __name__ == "__main__":
    main()
