#!/usr/bin/env python3
"""Fixture of MatrixObservationWithPaths (qos_constrained_ra.py:440-493), captured by running the reference's own wrapper where
the reference is importable (test infrastructure, data only; never runs on a GPU machine).

QoSConstrainedRA cannot be constructed as shipped; importing oracle/gen_golden_qos.py applies its two import-time repairs (the
module's main() does not run on import).  At the q1 configuration (seed 31, load 1000, S = 40, three classes, rejection
allowed) two action streams are recorded, each from a fresh env:
  sapff   300 steps of shortest_available_path
  random  300 seeded random actions in [0, k] (the reject action and paths a class-0 service may not take included)
After every reset and step: the counters (available_spectrum, int32 [E]), the pending (source, destination, class), and the
observation as np.packbits of its first dim - 1 columns plus the class column; the actions and the reset points.

  tests/golden/m1_qos_matrix_paths.npz

Usage:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python3 -W ignore <repo>/tools/gen_golden_qos_obs.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden_qos as gq  # noqa: E402  (the reference, repaired at import time)

qos, gg = gq.qos, gq.gg

KW = dict(seed=31, load=1000, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=40, num_service_classes=3,
          classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0], allow_rejection=True)
N_STEPS = 300
OUT = os.path.join(gg.GOLD, "m1_qos_matrix_paths.npz")


def _spill(env):
    """The observation has a column set only by the slice of a path running into the next block: a link without a free unit on
    allowed path p <= k - 2 that the next path does not use."""
    s, topo = env.service, env.topology
    paths = topo.graph["ksp"][s.source, s.destination]
    allowed = paths[:1] if s.service_class == 0 else paths

    def links(path):
        return {topo.edges[path.node_list[i], path.node_list[i + 1]]["index"] for i in range(len(path.node_list) - 1)}

    avail = topo.graph["available_spectrum"]
    for p, path in enumerate(allowed):
        if p + 2 > env.k_paths:
            break
        nxt = links(allowed[p + 1]) if p + 1 < len(allowed) else set()
        if any(avail[e] == 0 and e not in nxt for e in links(path)):
            return True
    return False


def record(chooser):
    env = qos.QoSConstrainedRA(topology=gg.load_topology("nsfnet_chen"), **KW)
    wrap = qos.MatrixObservationWithPaths(env)
    rec = dict(actions=[], reset_before=[], spectrum=[], pending=[], obs_bits=[], obs_class=[])
    n_spill = n_class0 = 0

    def snap():
        nonlocal n_spill, n_class0
        o = np.asarray(wrap.observation(None), np.float64).reshape(-1)
        body = o[:-1]
        assert np.isin(body, (0.0, 1.0)).all()
        s = env.service
        assert o[-1] == s.service_class
        rec["spectrum"].append(gq.spectrum(env))
        rec["pending"].append((s.source_id, s.destination_id, s.service_class))
        rec["obs_bits"].append(np.packbits(body.astype(np.uint8)))
        rec["obs_class"].append(int(o[-1]))
        n_spill += _spill(env)
        n_class0 += s.service_class == 0

    done = True
    for t in range(N_STEPS):
        first = done
        if done:
            env.reset()
            done = False
        snap()
        a = int(chooser(env, t))
        _, _r, done, _info = env.step(a)
        rec["actions"].append(a)
        rec["reset_before"].append(first)
    snap()
    dim = env.topology.number_of_edges() * env.num_spectrum_resources * (env.k_paths + 1) + 1
    out = dict(actions=np.array(rec["actions"], np.int64), reset_before=np.array(rec["reset_before"], np.uint8),
               spectrum=np.array(rec["spectrum"], np.int32), pending=np.array(rec["pending"], np.int32),
               obs_bits=np.array(rec["obs_bits"], np.uint8), obs_class=np.array(rec["obs_class"], np.uint8))
    return out, dim, env.k_paths, n_spill, n_class0


def main():
    rs = np.random.RandomState(9)
    acts = rs.randint(0, 6, size=N_STEPS)  # k = 5 paths + the reject action
    streams = (("sapff", lambda env, t: qos.shortest_available_path(env)), ("random", lambda env, t: acts[t]))
    arrays, meta = {}, dict(env="QoSConstrainedRA", topology="nsfnet_chen", kwargs=KW, n_steps=N_STEPS, streams={})
    for name, chooser in streams:
        out, dim, k, n_spill, n_class0 = record(chooser)
        for key, v in out.items():
            arrays["%s_%s" % (name, key)] = v
        meta["dim"], meta["k_paths"] = dim, k
        meta["streams"][name] = dict(n_obs=len(out["obs_class"]), n_spill=n_spill, n_class0=n_class0)
        print("%-7s observations %d  with a spill %d  class 0 %d  resets %d" % (name, len(out["obs_class"]), n_spill, n_class0,
                                                                             int(out["reset_before"].sum())))
    meta["n_spill"] = sum(s["n_spill"] for s in meta["streams"].values())
    meta["n_class0"] = sum(s["n_class0"] for s in meta["streams"].values())
    np.savez_compressed(OUT, meta=np.array(json.dumps(meta)), **arrays)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
