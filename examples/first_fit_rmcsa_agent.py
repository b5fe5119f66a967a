#!/usr/bin/env python3
"""One-head agents for RMCSA: the agent fixes a prefix of the (path, modulation, core, first slot) action and the device completes
it first-fit (`complete_actions`), under the validity rule of the two-stage masks.  The "path_modulation" row is then the whole
mask of the agent — no second head of C * S + 1 logits, no second mask launch, no second sampling pass per step.

Printed on the same seeds (those of examples/masked_rmcsa_agent.py), service blocking of:
  (a) the empty prefix as a heuristic: a reach-aware k-shortest-path first fit — the first path with room under the modulation within
      reach that needs the fewest slots;
  (b) a uniformly random agent over the "path_modulation" mask whose pair the device completes (g = 2), the whole loop — mask,
      sampling, completion, step — captured in one graph and replayed;
  (c) the two-stage uniformly random masked agent (both heads sampled);
  (d) SAP_BM_FC_FF, which takes each path's best modulation by length alone and walks into the reach limits of step().

    python examples/first_fit_rmcsa_agent.py [num_envs] [steps]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 400
kw = dict(topology="nsfnet_chen", load=300, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=64,
          num_spatial_resources=7, allow_rejection=True)


def blocking(env):
    processed, accepted = env.totals()
    return 1.0 - accepted / processed


def sample(mask, noise):
    """One uniformly drawn provisioning column per row (the largest noise among the set ones); rows without one: the last column,
    the reject action (set, as allow_rejection is on, but never preferred)."""
    score = torch.where(mask, noise, torch.full_like(noise, -1.0))
    score[:, -1] = -0.5
    return score.argmax(dim=1)


def make():
    return orl.make("RMCSA-v0", num_envs=B, seeds=1, **kw)


# (a) the empty prefix: completion and step per step, nothing else
env = make()
with torch.cuda.stream(env.torch_stream()):
    for _ in range(STEPS):
        env.complete_actions(n_given=0, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
env.sync()
env.check()
print("(a) first-fit completion of the empty prefix:   service blocking %.4f" % blocking(env))
env.close()

# (b) one head: the path-modulation mask, a uniform draw, the device completes the pair; one captured graph per step
env = make()
dev = "cuda:%d" % env.device_id
K, M, C, S = env.k_paths, len(env.modulation_formats), env.num_spatial_resources, env.num_spectrum_resources
acts = env.device_tensor("actions")
gen = torch.Generator(device=dev).manual_seed(3)
stream = env.torch_stream()
env.action_mask("path_modulation", fetch=False)  # (the first call allocates the buffer: before the capture)
pm = env.device_tensor("action_mask")            # bool [B, K * M + 1] at the device pitch, no copy
noise = torch.empty((B, K * M + 1), device=dev)


def one_head_step():
    env.action_mask("path_modulation", fetch=False)
    col = sample(pm, noise)
    rej = col == K * M                           # (the reject column decodes to path K: no completion)
    acts[:, 0] = torch.where(rej, torch.full_like(col, K), col // M).int()
    acts[:, 1] = (col % M).int()
    env.complete_actions(n_given=2, fetch=False)  # reads the pair where the agent just wrote it, writes all four columns
    env.step(None, auto_reset=True, fetch=False)


with torch.cuda.stream(stream):
    noise.copy_(torch.rand(noise.shape, device=dev, generator=gen))
    one_head_step()                              # (warm: every launch of the loop has run once)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
stream.wait_stream(torch.cuda.current_stream())
with torch.cuda.graph(graph, stream=stream):
    one_head_step()
with torch.cuda.stream(stream):
    for _ in range(STEPS - 1):
        noise.copy_(torch.rand(noise.shape, device=dev, generator=gen))
        graph.replay()
env.sync()
env.check()
print("(b) one-head masked random agent, g = 2:        service blocking %.4f" % blocking(env))
env.close()

# (c) both heads sampled: examples/masked_rmcsa_agent.py
env = make()
acts = env.device_tensor("actions")
gen = torch.Generator(device=dev).manual_seed(3)
env.action_mask("path_modulation", fetch=False)
pm = env.device_tensor("action_mask")
env.action_mask("core_slot", fetch=False)
cs = env.device_tensor("action_mask")
with torch.cuda.stream(env.torch_stream()):
    for _ in range(STEPS):
        env.action_mask("path_modulation", fetch=False)
        col = sample(pm, torch.rand((B, K * M + 1), device=dev, generator=gen))
        acts[:, 0] = (col // M).int()
        acts[:, 1] = (col % M).int()
        env.action_mask("core_slot", fetch=False)
        col = sample(cs, torch.rand((B, C * S + 1), device=dev, generator=gen))
        reject = col == C * S
        acts[:, 2] = (col // S).int()
        acts[:, 3] = torch.where(reject, torch.full_like(col, S), col % S).int()
        acts[:, 0] = torch.where(reject, torch.full_like(col, K), acts[:, 0].long()).int()
        acts[:, 1] = torch.where(reject, torch.full_like(col, M), acts[:, 1].long()).int()
        env.step(None, auto_reset=True, fetch=False)
env.sync()
env.check()
print("(c) two-stage masked random agent:              service blocking %.4f" % blocking(env))
env.close()

# (d) the heuristic, entirely on the device
env = make()
env.run("SAP_BM_FC_FF", STEPS)
print("(d) SAP_BM_FC_FF heuristic:                     service blocking %.4f" % blocking(env))
env.close()
