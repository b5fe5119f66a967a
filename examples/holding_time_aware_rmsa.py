#!/usr/bin/env python3
"""Holding-time-aware spectrum assignment for RMSA, entirely on the device: put a service next to a neighbour that leaves when it does,
so that the hole the two leave is one hole.  Per step `block_table(j)` lists every candidate path's first j free blocks that fit the
pending service and `release_horizons("blocks", j)` says, for each of them, in how long the slot below and the slot above the block
free up (+inf at the spectrum's edge) and how long the service itself will stay.  A few torch operations pick, among the listed blocks,
the one whose nearer-in-time finite neighbour horizon is closest to the service's own holding time — ties to the lower index, blocks
with only the spectrum's edge for neighbours last — and `select_blocks` places the service against that neighbour: at the block's
lower end ("first") for the left one, at its upper end ("last") for the right one.  Then `step(None)`.  The loop is captured in one
graph and replayed; nothing crosses PCIe.  Seeds, sizes and load are those of examples/routing_rules_rmsa.py; its KSP-FF
(`route_spectrum("first", "ksp")`) and the reference's SAP_FF run beside it.

    python examples/holding_time_aware_rmsa.py [num_envs] [steps] [j]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 400
J = int(sys.argv[3]) if len(sys.argv) > 3 else 4
kw = dict(topology="nsfnet_chen", load=300, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=64,
          allow_rejection=True)


def blocking(env):
    processed, accepted = env.totals()
    return 1.0 - accepted / processed


def make():
    return orl.make("RMSA-v0", num_envs=B, seeds=1, **kw)


def replayed(env, one_step):
    """one_step() once eagerly (every launch has run, every buffer exists), then captured and replayed STEPS - 1 times"""
    stream = env.torch_stream()
    with torch.cuda.stream(stream):
        one_step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=stream):
        one_step()
    with torch.cuda.stream(stream):
        for _ in range(STEPS - 1):
            graph.replay()
    env.sync()
    env.check()
    del graph
    return blocking(env)


env = make()
env.block_table(J, fetch=False)
env.release_horizons("blocks", J, fetch=False)
env.sync()
acts, mask, horizons = env.device_tensor("actions"), env.device_tensor("block_mask"), env.device_tensor("release_horizons")
R = env.k_paths
first = torch.empty_like(acts)


def aware_step():
    env.block_table(J, fetch=False)
    env.release_horizons("blocks", J, fetch=False)
    near = horizons[:, :-1].reshape(B, R * J, 2)
    gap = (near - horizons[:, -1].reshape(B, 1, 1)).abs()                     # |neighbour's remaining time - own holding time|; inf at an edge
    gap = torch.where(torch.isfinite(near), gap, torch.full_like(gap, 1e30))  # edge-only blocks last, yet before none at all
    score, side = gap.min(dim=2)                                              # the nearer neighbour of each block: 0 left, 1 right
    score = torch.where(mask[:, :-1], score, torch.full_like(score, float("inf")))
    best = score.argmin(dim=1)
    index = torch.where(mask[:, :-1].any(dim=1), best, torch.full_like(best, R * J)).to(torch.int32)  # no block at all: the reject action
    right = side.gather(1, best.reshape(B, 1)) == 1
    acts[:, 0].copy_(index)
    env.select_blocks(None, J, placement="first", fetch=False)
    first.copy_(acts)
    acts[:, 0].copy_(index)
    env.select_blocks(None, J, placement="last", fetch=False)
    acts.copy_(torch.where(right, acts, first))
    env.step(None, auto_reset=True, fetch=False)


aware = replayed(env, aware_step)
env.close()

env = make()


def ksp_ff_step():
    env.route_spectrum("first", "ksp", fetch=False)
    env.step(None, auto_reset=True, fetch=False)


ksp_ff = replayed(env, ksp_ff_step)
env.close()
env = make()
env.run("SAP_FF", STEPS)
sap = blocking(env)
env.close()
print("service blocking, %d envs x %d steps, j = %d" % (B, STEPS, J))
print("holding-time-aware blocks %.4f   route_spectrum(first, ksp) %.4f   SAP_FF %.4f" % (aware, ksp_ff, sap))
