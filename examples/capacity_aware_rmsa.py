#!/usr/bin/env python3
"""Capacity-loss-minimising routing for RMSA on the device: try every path on a fork of the env, ask network_capacity("counts") what
each choice leaves the network able to carry, keep the path that blocks the fewest (pair, class) cells.

RMSA on NSFNET with the sizes of the benchmark's cfg2 (320 slots, 300 Erlang) and the seeds of examples/lookahead_rmsa.py.  R root
envs, and a scratch batch of R x k envs of the same configuration.  Per step of the roots:
  1. root i is forked into the children i*k .. i*k + k - 1 of the scratch batch (one copy_envs call);
  2. child p provisions the pending service first-fit on path p (policy "PATH_FF");
  3. network_capacity("counts", fetch=False) on the children: per class the node pairs that could no longer be served — every pair and
     every bit rate of the network, not the pending service's alone; the rows are read in place as a torch tensor;
  4. root i takes the first-fit action on the path whose child has the fewest blocked (pair, class) cells, the lowest p on ties; a child
     whose own service was refused loses to every child that accepted it.
Printed: the service blocking rate of the roots beside that of plain SAP_FF and of route_spectrum("first", "ksp") (first fit on the
first path with room, in k-shortest-path order) on the same seeds over the same steps — whichever way it falls.

    python examples/capacity_aware_rmsa.py [--roots 256] [--steps 1000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import numpy as np  # noqa: E402
import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--roots", type=int, default=256)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=1500, help="SAP_FF steps of every batch before the comparison starts (5 x load)")
args = ap.parse_args()

kw = dict(topology="nsfnet_chen", load=300, mean_service_holding_time=25, episode_length=10 ** 9, num_spectrum_resources=320,
          allow_rejection=False)
R = args.roots
roots = orl.make("RMSA-v0", num_envs=R, seeds=10, **kw)
plain = orl.make("RMSA-v0", num_envs=R, seeds=10, **kw)
ksp = orl.make("RMSA-v0", num_envs=R, seeds=10, **kw)
k = roots.k_paths
scratch = orl.make("RMSA-v0", num_envs=R * k, seeds=10 + R, **kw)
for b in (roots, plain, ksp, scratch):
    b.run("SAP_FF", args.warmup)

parent = np.repeat(np.arange(R), k)
child = np.arange(R * k)
path_of_child = np.tile(np.arange(k), R).astype(np.int32)
n_cls = scratch.network_capacity_shape("serviceable")[1]
cells = int((scratch.topology.n_paths > 0).sum()) * n_cls
scratch.network_capacity("counts", fetch=False)  # (allocates the rows)
counts = scratch.device_tensor("capacity_counts")
p0, a0 = roots.totals()
q0, b0 = plain.totals()
r0, c0 = ksp.totals()
blocked_sum = taken = 0
t0 = time.time()
for _ in range(args.steps):
    scratch.copy_envs(parent, child, source=roots)
    before = scratch.counters()[:, 1]  # services accepted so far (the source's count)
    scratch.policy_step("PATH_FF", auto_reset=True, fetch=False, paths=path_of_child)
    scratch.network_capacity("counts", fetch=False)
    refused = torch.as_tensor(scratch.counters()[:, 1] == before, device=counts.device)  # (counters() has synchronised)
    blocked = counts[:, :n_cls].sum(dim=1) + refused * (cells + 1)
    best = torch.argmin(blocked.reshape(R, k), dim=1)  # (the first of equal minima: the lowest p)
    blocked_sum += float(blocked.reshape(R, k).gather(1, best[:, None]).clamp(max=cells).sum())
    roots.policy_step("PATH_FF", auto_reset=True, fetch=False, paths=best.to(torch.int32).cpu().numpy())
    taken += R
roots.sync()
dt = time.time() - t0
plain.run("SAP_FF", args.steps)
for _ in range(args.steps):
    ksp.route_spectrum("first", "ksp", fetch=False)
    ksp.step(None, auto_reset=True, fetch=False)
ksp.sync()
p1, a1 = roots.totals()
q1, b1 = plain.totals()
r1, c1 = ksp.totals()
print("%d roots x %d steps, %d children each: %.1f s; %.1f of %d (pair, class) cells blocked after the chosen action, on average"
      % (R, args.steps, k, dt, blocked_sum / taken, cells))
print("service blocking rate: capacity-aware %.4f, plain SAP_FF %.4f, first fit in k-shortest-path order %.4f"
      % (1 - (a1 - a0) / (p1 - p0), 1 - (b1 - b0) / (q1 - q0), 1 - (c1 - c0) / (r1 - r0)))
for b in (roots, plain, ksp, scratch):
    b.check()
    b.close()
