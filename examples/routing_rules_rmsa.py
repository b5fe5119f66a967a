#!/usr/bin/env python3
"""Routing x spectrum-assignment baselines for RMSA, entirely on the device: `route_spectrum(rule, route)` computes the rule's winning
slot and its cost on every candidate path and picks the path under a routing order — "ksp" the first path that fits (KSP-FF with
"first"), "best" the cheapest winner over all paths (FF-KSP with "first": the lowest slot anywhere), "least_loaded" the path with the
most free slots (the reference's least_loaded_path_first_fit with "first") — for the rules first fit, best fit and min_cuts (the start
that splits the fewest free runs of the path's links).  The seeds and sizes are those of examples/spectrum_rules_rmsa.py.  One step
is two launches — the route, then `step(None)` on the device-resident action — captured in one graph and replayed; no slot map
crosses PCIe.

    python examples/routing_rules_rmsa.py [num_envs] [steps]
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


print("service blocking, %d envs x %d steps        %s" % (B, STEPS, "  ".join("%-12s" % r for r in ("first", "best", "min_cuts"))))
for route in ("ksp", "best", "least_loaded"):
    row = []
    for rule in ("first", "best", "min_cuts"):
        env = make()
        stream = env.torch_stream()

        def one_step():
            env.route_spectrum(rule, route, fetch=False)
            env.step(None, auto_reset=True, fetch=False)

        with torch.cuda.stream(stream):
            one_step()  # (warm: every launch of the loop has run once, the table is allocated)
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
        row.append(blocking(env))
        del graph
        env.close()
    print("route %-12s rule on the device:         %s" % (route, "  ".join("%-12.4f" % v for v in row)))

env = make()
env.run("SAP_FF", STEPS)
sap = blocking(env)
env.close()
env = make()
env.run("LLP_FF", STEPS)
print("the reference's heuristics:                   SAP_FF %.4f  LLP_FF %.4f" % (sap, blocking(env)))
env.close()
