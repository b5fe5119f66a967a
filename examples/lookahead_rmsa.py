#!/usr/bin/env python3
"""A one-step lookahead (rollout) policy for RMSA on the device, built on copy_envs: fork, try every path, roll the heuristic
forward, keep the best.

RMSA on NSFNET with the sizes of the benchmark's cfg2 (320 slots, 300 Erlang).  R root envs, and a scratch batch of R x k envs of the
same configuration.  Per step of the roots:
  1. root i is forked into the children i*k .. i*k + k - 1 of the scratch batch (one copy_envs call);
  2. child p provisions the pending service first-fit on path p (policy "PATH_FF");
  3. every child runs the shortest-available-path first-fit heuristic ("SAP_FF") for H steps;
  4. root i takes the first-fit action on the path whose child accepted the most services, the lowest p on ties.
Printed: the service blocking rate of the roots beside that of plain SAP_FF on the same seeds over the same steps.

--shared-streams forks WITH the random streams (keep_rng=False): every child then draws exactly the arrivals its root is going to
see, so the lookahead is CLAIRVOYANT — an upper bound, not a policy anyone could run.  The default (keep_rng=True) leaves each
child the stream it has: it sees the root's network and pending service, and a future of its own.  Measured on an MI355X with the
defaults below: plain SAP_FF blocks 0.0398 of the services, the clairvoyant lookahead 0.0315, the lookahead on the children's own
streams 0.1199 — five children with five different futures compare the paths on noise, and a 20-step rollout of one sample each
is worse than the heuristic it rolls out.  (Children that share ONE future different from the root's — common random numbers —
are the obvious next step; they need nothing from the library beyond keep_rng and equal seeds.)

    python examples/lookahead_rmsa.py [--roots 256] [--steps 1000] [--horizon 20] [--shared-streams]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import numpy as np  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--roots", type=int, default=256)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--warmup", type=int, default=1500, help="SAP_FF steps of every batch before the comparison starts (5 x load)")
ap.add_argument("--horizon", type=int, default=20)
ap.add_argument("--shared-streams", action="store_true")
args = ap.parse_args()

kw = dict(topology="nsfnet_chen", load=300, mean_service_holding_time=25, episode_length=10 ** 9, num_spectrum_resources=320,
          allow_rejection=False)
R = args.roots
roots = orl.make("RMSA-v0", num_envs=R, seeds=10, **kw)
plain = orl.make("RMSA-v0", num_envs=R, seeds=10, **kw)
k = roots.k_paths
scratch = orl.make("RMSA-v0", num_envs=R * k, seeds=10 + R, **kw)
for b in (roots, plain, scratch):
    b.run("SAP_FF", args.warmup)

parent = np.repeat(np.arange(R), k)
child = np.arange(R * k)
path_of_child = np.tile(np.arange(k), R).astype(np.int32)
p0, a0 = roots.totals()
q0, b0 = plain.totals()
t0 = time.time()
for _ in range(args.steps):
    scratch.copy_envs(parent, child, source=roots, keep_rng=not args.shared_streams)
    before = scratch.counters()[:, 1]  # services accepted so far (the source's count)
    scratch.policy_step("PATH_FF", auto_reset=True, fetch=False, paths=path_of_child)
    scratch.run("SAP_FF", args.horizon)
    gain = (scratch.counters()[:, 1] - before).reshape(R, k)
    roots.policy_step("PATH_FF", auto_reset=True, fetch=False, paths=np.argmax(gain, axis=1).astype(np.int32))
roots.sync()
dt = time.time() - t0
plain.run("SAP_FF", args.steps)
p1, a1 = roots.totals()
q1, b1 = plain.totals()
print("%d roots x %d steps, %d children each, horizon %d, %s: %.1f s" % (R, args.steps, k, args.horizon,
      "streams shared with the root (clairvoyant)" if args.shared_streams else "children on their own streams", dt))
print("service blocking rate: lookahead %.4f, plain SAP_FF %.4f" % (1 - (a1 - a0) / (p1 - p0), 1 - (b1 - b0) / (q1 - q0)))
for b in (roots, plain, scratch):
    b.check()
    b.close()
