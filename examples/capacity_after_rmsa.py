#!/usr/bin/env python3
"""Capacity-loss-minimising routing for RMSA without a fork: capacity_after() says what every candidate path would leave the network
able to carry, and the env takes the one that blocks the fewest (pair, class) cells.

RMSA on NSFNET with the sizes, load and seeds of examples/capacity_aware_rmsa.py (320 slots, 300 Erlang).  Per step, all on the device
and captured in ONE graph — no scratch batch, no copy of the env states, no extra step, no round trip to the host:
  1. route_spectrum("first", "ksp", table=True, fetch=False): the first-fit window of every path, as the assignment table;
  2. capacity_after("route", "total", fetch=False): per path the (pair, class) cells that would be blocked with the service placed there
     — every pair and every bit rate of the network — and -1 for a path without room;
  3. torch.argmin over the present candidates, the lowest path on ties; (path, its slot) written into the actions buffer — the reject
     action where no path has room;
  4. step(None).
Unlike capacity_aware_rmsa.py this scores the slot map right after the placement, not a forked child after its step, which has also run
the releases that fall due before the next arrival; the two need not choose alike.
Printed: the service blocking rate beside that of plain SAP_FF and of route_spectrum("first", "ksp") on the same seeds over the same
steps — whichever way it falls.

    python examples/capacity_after_rmsa.py [--roots 256] [--steps 1000]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

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
for b in (roots, plain, ksp):
    b.run("SAP_FF", args.warmup)
k, S = roots.k_paths, roots.num_spectrum_resources
stream = roots.torch_stream()
roots.route_spectrum("first", "ksp", fetch=False)   # (the first calls allocate the table and the rows: before the capture)
roots.capacity_after("route", "total", fetch=False)
roots.sync()
total = roots.device_tensor("capacity_after_total")
table = roots.device_tensor("assign_table").view(R, k, 4)
actions = roots.device_tensor("actions")
env_index = torch.arange(R, device=total.device)
huge = torch.full((R, k), 2 ** 30, dtype=torch.int32, device=total.device)
blocked_sum = torch.zeros((), dtype=torch.float64, device=total.device)


def one_step():
    roots.route_spectrum("first", "ksp", fetch=False)
    roots.capacity_after("route", "total", fetch=False)
    t = total[:, :k]
    best = torch.argmin(torch.where(t >= 0, t, huge), dim=1)  # (the first of equal minima: the lowest path)
    fits = (t >= 0).any(dim=1)
    actions[:, 0] = torch.where(fits, best, torch.full_like(best, k)).to(torch.int32)
    actions[:, 1] = table[env_index, best, 0]  # (S where nothing fits: the reject action)
    blocked_sum.add_(torch.where(fits, t[env_index, best], total[:, k]).sum())
    roots.step(None, auto_reset=True, fetch=False)


p0, a0 = roots.totals()
q0, b0 = plain.totals()
r0, c0 = ksp.totals()
with torch.cuda.stream(stream):
    one_step()  # (the first step runs eagerly: it warms torch's kernels up outside the capture, and counts like the others)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
stream.wait_stream(torch.cuda.current_stream())
with torch.cuda.graph(graph, stream=stream):
    one_step()  # (captured, not run)
torch.cuda.synchronize()
t0 = time.time()
for _ in range(args.steps - 1):
    graph.replay()
torch.cuda.synchronize()
dt = time.time() - t0
plain.run("SAP_FF", args.steps)
for _ in range(args.steps):
    ksp.route_spectrum("first", "ksp", fetch=False)
    ksp.step(None, auto_reset=True, fetch=False)
ksp.sync()
p1, a1 = roots.totals()
q1, b1 = plain.totals()
r1, c1 = ksp.totals()
n_cls = roots.network_capacity_shape("serviceable")[1]
cells = int((roots.topology.n_paths > 0).sum()) * n_cls
print("%d envs x %d steps in one captured graph, no scratch batch: %.2f s (%.0f us per step); %.1f of %d (pair, class) cells blocked after "
      "the chosen placement, on average" % (R, args.steps, dt, 1e6 * dt / max(1, args.steps - 1), float(blocked_sum) / (R * args.steps), cells))
print("service blocking rate: capacity_after %.4f, plain SAP_FF %.4f, first fit in k-shortest-path order %.4f"
      % (1 - (a1 - a0) / (p1 - p0), 1 - (b1 - b0) / (q1 - q0), 1 - (c1 - c0) / (r1 - r0)))
for b in (roots, plain, ksp):
    b.check()
    b.close()
