#!/usr/bin/env python3
"""The standard spectrum-assignment baselines for RMSA, entirely on the device: k-shortest-path routing — the first path on which
the service fits — with the first slot chosen by first fit, last fit, best fit, exact fit, most used or least used
(`assign_spectrum(rule)` with no path given), beside the reference's SAP_FF heuristic on the same seeds (those of
examples/first_fit_rmcsa_agent.py).  One step is two launches — the rule, then `step(None)` on the device-resident action — captured
in one graph and replayed; no slot map crosses PCIe.

Unlike SAP_FF, whose first fit searches range(0, S - n), every rule here may start a service on s = S - n.

    python examples/spectrum_rules_rmsa.py [num_envs] [steps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 400
kw = dict(topology="nsfnet_chen", load=300, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=64,
          allow_rejection=True)


def blocking(env):
    processed, accepted = env.totals()
    return 1.0 - accepted / processed


def make():
    return orl.make("RMSA-v0", num_envs=B, seeds=1, **kw)


for rule in ("first", "last", "best", "exact", "most_used", "least_used"):
    env = make()
    stream = env.torch_stream()

    def one_step():
        env.assign_spectrum(rule, fetch=False)  # n_given = 0: the first path with room, the slot under the rule
        env.step(None, auto_reset=True, fetch=False)

    with torch.cuda.stream(stream):
        one_step()  # (warm: every launch of the loop has run once)
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
    print("%-10s k-shortest-path + rule on the device:  service blocking %.4f" % (rule, blocking(env)))
    del graph
    env.close()

env = make()
env.run("SAP_FF", STEPS)
print("%-10s the reference's heuristic:             service blocking %.4f" % ("SAP_FF", blocking(env)))
env.close()
