#!/usr/bin/env python3
"""A two-stage masked agent for RMCSA on the same GPU as the envs.  An RMCSA action is (path, modulation, core, first slot), and
nearly all of that space cannot provision the pending service: most (path, modulation) pairs are beyond one of the two reach
limits, and most (core, slot) pairs of a reachable one are busy or too close to the end of the spectrum.  The batch's two mask
layouts factorise validity exactly: "path_modulation" says which pairs provision on some core and slot, "core_slot" which (core,
slot) provision under the pair the agent wrote into columns 0 and 1 of the actions buffer.  Sampling stage 1, then stage 2, never
yields a blocked action while a provisioning one exists.

Here the agent is uniformly random over the set columns of both rows (the place of a two-head policy's masked logits); everything
stays on the device: the masks are torch views of the batch's own arrays, the actions are written into the batch's action array,
and all launches are queued on the batch's stream (`env.torch_stream()`).  Printed beside it on the same seeds: a uniformly random
agent without masks and the SAP_BM_FC_FF heuristic.

    python examples/masked_rmcsa_agent.py [num_envs] [steps]
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


# the heuristic, entirely on the device
env = orl.make("RMCSA-v0", num_envs=B, seeds=1, **kw)
env.run("SAP_BM_FC_FF", STEPS)
print("SAP_BM_FC_FF heuristic:        service blocking %.4f" % blocking(env))
env.close()

for masked in (False, True):
    env = orl.make("RMCSA-v0", num_envs=B, seeds=1, **kw)
    dev = "cuda:%d" % env.device_id
    K, M, C, S = env.k_paths, len(env.modulation_formats), env.num_spatial_resources, env.num_spectrum_resources
    acts = env.device_tensor("actions")
    gen = torch.Generator(device=dev).manual_seed(3)
    if masked:
        env.action_mask("path_modulation", fetch=False)  # (the first call of a layout allocates its buffer)
        pm = env.device_tensor("action_mask")            # bool [B, K * M + 1] at the device pitch, no copy
        env.action_mask("core_slot", fetch=False)
        cs = env.device_tensor("action_mask")            # bool [B, C * S + 1]; each view keeps showing its own layout
    with torch.cuda.stream(env.torch_stream()):
        for _ in range(STEPS):
            if masked:
                env.action_mask("path_modulation", fetch=False)
                col = sample(pm, torch.rand((B, K * M + 1), device=dev, generator=gen))
                # stage 1 into columns 0 and 1 (the reject column decodes to path K: no (core, slot) provisions under it)
                acts[:, 0] = (col // M).int()
                acts[:, 1] = (col % M).int()
                env.action_mask("core_slot", fetch=False)  # reads the pairs where the agent just wrote them
                col = sample(cs, torch.rand((B, C * S + 1), device=dev, generator=gen))
                reject = col == C * S
                acts[:, 2] = (col // S).int()
                acts[:, 3] = torch.where(reject, torch.full_like(col, S), col % S).int()
                acts[:, 0] = torch.where(reject, torch.full_like(col, K), acts[:, 0].long()).int()
                acts[:, 1] = torch.where(reject, torch.full_like(col, M), acts[:, 1].long()).int()
            else:
                hi = torch.tensor([K, M, C, S], device=dev)
                acts.copy_((torch.rand((B, 4), device=dev, generator=gen) * hi).int())
            env.step(None, auto_reset=True, fetch=False)
    env.sync()
    env.check()
    print("%s service blocking %.4f" % ("two-stage masked random agent:" if masked else "unmasked random agent:        ", blocking(env)))
    env.close()
