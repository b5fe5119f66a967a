#!/usr/bin/env python3
"""Core selection x spectrum-assignment baselines for RMCSA, entirely on the device: `route_cores(rule, route)` computes the rule's
winning slot and its cost on every (path, core) pair and picks the pair under a route — "ksp" the first path and its first core that
fit (with "first": complete_actions' first fit), "best" the cheapest winner over all pairs, "least_loaded" the pair with the most free
slots, "ksp_best_core" / "ksp_least_loaded_core" the first path that fits and on it the cheapest / the least-loaded core — for the
rules first fit, best fit, exact fit and min_cuts (the start that splits the fewest free runs of the path's links in that core).  One
step is two launches — the route, then `step(None)` on the device-resident action — captured in one graph and replayed; no slot map
crosses PCIe.

At the load of examples/masked_rmcsa_agent.py (300 Erlang on 7 cores x 64 slots) the maps never fill and a service is blocked exactly
when no modulation is within reach, whichever provisioning action is taken (31.9 %); here the 7 cores have 32 slots each and carry
700 Erlang, so that the maps fill and the choice of core and slot shows in the blocking.

    python examples/core_rules_rmcsa.py [num_envs] [steps] [load]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 1200
LOAD = float(sys.argv[3]) if len(sys.argv) > 3 else 700
kw = dict(topology="nsfnet_chen", load=LOAD, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=32,
          num_spatial_resources=7, allow_rejection=True)
RULES = ("first", "best", "exact", "min_cuts")
ROUTES = ("ksp", "best", "least_loaded", "ksp_best_core", "ksp_least_loaded_core")


def blocking(env):
    processed, accepted = env.totals()
    return 1.0 - accepted / processed


def make():
    return orl.make("RMCSA-v0", num_envs=B, seeds=1, **kw)


print("service blocking, %d envs x %d steps, load %g   %s" % (B, STEPS, LOAD, "  ".join("%-10s" % r for r in RULES)))
for route in ROUTES:
    row = []
    for rule in RULES:
        env = make()
        stream = env.torch_stream()

        def one_step():
            env.route_cores(rule, route, fetch=False)
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
    print("route %-22s rule on the device:   %s" % (route, "  ".join("%-10.4f" % v for v in row)))

env = make()
with torch.cuda.stream(env.torch_stream()):
    for _ in range(STEPS):
        env.complete_actions(n_given=0, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
env.sync()
first_fit = blocking(env)
env.close()
env = make()
env.run("SAP_BM_FC_FF", STEPS)
print("complete_actions(n_given=0) %.4f   SAP_BM_FC_FF %.4f" % (first_fit, blocking(env)))
env.close()
