#!/usr/bin/env python3
"""A blocking-against-load curve from one batch: 8 loads x 512 seeds of RMSA-v0 on NSFNET, every env at its own load, then the
upper half of the curve moved up on the live batch with set_load (what a curriculum callback does through
`venv.env_method("set_load", load=..., indices=...)`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import optical_rl_gym_amd as orl  # noqa: E402

loads = np.linspace(100, 400, 8)
L, R = len(loads), 512
n = L * R
# (event_capacity: room for the pending releases of the largest load set_load will ask for, 500 Erlang -> 787)
batch = orl.make("RMSA-v0", topology="nsfnet_chen", num_envs=n, seeds=10, load=loads[np.arange(n) % L], mean_service_holding_time=25,
                 episode_length=1000, num_spectrum_resources=320, event_capacity=orl.BatchedRMSAEnv.capacity_needed(500))


def curve():
    c0 = batch.counters()
    batch.run("SAP_FF", 1000)
    d = (batch.counters() - c0).astype(float)
    return [1 - d[i::L, 1].sum() / d[i::L, 0].sum() for i in range(L)]


batch.run("SAP_FF", 500)  # warm-up: the networks fill
for ld, b in zip(batch.load[:L], curve()):
    print("load %5.1f  service blocking %.4f" % (ld, b))
batch.set_load(load=batch.load * 1.25, mask=batch.load >= 250)  # services drawn from now on; nothing else changes
batch.run("SAP_FF", 500)
for ld, b in zip(batch.load[:L], curve()):
    print("load %5.1f  service blocking %.4f" % (ld, b))
batch.close()
