#!/usr/bin/env python3
"""A learning agent on the same GPU as RMCSA-v0 envs that acts in DeepRMSA's terms: it sees the batch's path features
(`path_features(j, fetch=False)`: per (path, core) row the first j free blocks that fit the pending service) and chooses "row r, block
b" — one head over Discrete(k * cores * j + 1), masked with `device_tensor("block_mask")`, every set column of which provisions.  The
agent writes its index into column 0 of the actions array, `select_blocks(fetch=False)` decodes it on the device into (path,
modulation, core, first slot) and `step(None, fetch=False)` takes it.  Nothing crosses PCIe in the rollout, and the whole rollout of T
steps is captured once in a `torch.cuda.CUDAGraph` on the batch's stream.

The configuration is that of examples/core_rules_rmcsa.py — 7 cores x 32 slots under 700 Erlang, so that the maps fill and the choice
of core and block shows in the blocking.  The policy is a small MLP trained with a plain policy-gradient update (reward-to-go,
batch-mean baseline, entropy bonus); the point is the data path, not the algorithm.  Service blocking is printed beside
route_cores("first", "ksp") and the SAP_BM_FC_FF heuristic on the same seeds: measured, no threshold.

    python examples/block_actions_rmcsa_agent.py [num_envs] [updates] [--eager] [--j N] [--last]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
EAGER = "--eager" in sys.argv
PLACEMENT = "last" if "--last" in sys.argv else "first"
J = int(sys.argv[sys.argv.index("--j") + 1]) if "--j" in sys.argv else 2
if "--j" in sys.argv:
    args.remove(str(J))
B = int(args[0]) if len(args) > 0 else 4096
UPDATES = int(args[1]) if len(args) > 1 else 60
T = 32  # steps per rollout
kw = dict(topology="nsfnet_chen", load=700, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=32,
          num_spatial_resources=7, allow_rejection=True)
STEPS = UPDATES * T + T  # (the warm rollout included)


def blocking(env):
    processed, accepted = env.totals()
    return 1.0 - accepted / processed


# the baselines on the same seeds and as many steps, entirely on the device
ref = orl.make("RMCSA-v0", num_envs=B, seeds=1, **kw)
with torch.cuda.stream(ref.torch_stream()):
    for _ in range(STEPS):
        ref.route_cores("first", "ksp", fetch=False)
        ref.step(None, auto_reset=True, fetch=False)
ref.sync()
first_ksp = blocking(ref)
ref.close()
ref = orl.make("RMCSA-v0", num_envs=B, seeds=1, **kw)
ref.run("SAP_BM_FC_FF", STEPS)
print("service blocking over %d steps of %d envs: route_cores(first, ksp) %.4f   SAP_BM_FC_FF %.4f" % (STEPS, B, first_ksp, blocking(ref)))
ref.close()

env = orl.make("RMCSA-v0", num_envs=B, seeds=1, **kw)
dev = "cuda:%d" % env.device_id
env.reset()
env.path_features(J, fetch=False)  # (the first calls allocate the device buffers: outside the capture)
env.block_table(J, fetch=False)
feat = env.device_tensor("path_features")  # float32 [B, dim] at the device pitch, no copy
mask = env.device_tensor("block_mask")     # bool [B, rows * j + 1]: the last column is the reject action
acts, rew = env.device_tensor("actions"), env.device_tensor("reward")
dim, n_actions = feat.shape[1], mask.shape[1]
net = torch.nn.Sequential(torch.nn.Linear(dim, 256), torch.nn.ELU(), torch.nn.Linear(256, 256), torch.nn.ELU(), torch.nn.Linear(256, n_actions)).to(dev)
opt = torch.optim.Adam(net.parameters(), lr=3e-4)
obs_buf = torch.zeros((T, B, dim), device=dev)
act_buf = torch.zeros((T, B), dtype=torch.long, device=dev)
rew_buf = torch.zeros((T, B), device=dev)
mask_buf = torch.ones((T, B, n_actions), dtype=torch.bool, device=dev)
stream = env.torch_stream()


def rollout():
    for t in range(T):
        with torch.no_grad():
            obs_buf[t].copy_(feat)
            mask_buf[t].copy_(mask)
            logits = net(obs_buf[t]).masked_fill(~mask, float("-inf"))
            u = torch.rand_like(logits).clamp_(1e-7, 1 - 1e-7)
            a = (logits - torch.log(-torch.log(u))).argmax(dim=1)  # Gumbel-max = a sample of Categorical(logits)
            act_buf[t].copy_(a)
            acts[:, 0].copy_(a.int())                              # the index; the reject column is an index beyond the blocks
        env.select_blocks(None, J, placement=PLACEMENT, fetch=False)  # (row, block) -> (path, modulation, core, slot) in the actions array
        env.step(None, auto_reset=True, fetch=False)               # one launch; reward / done are rewritten in place
        env.path_features(J, fetch=False)                          # what the agent sees next
        env.block_table(J, fetch=False)                            # what it may do next
        rew_buf[t].copy_(rew)


with torch.cuda.stream(stream):  # (libraries' workspaces are set up outside the capture)
    rollout()
torch.cuda.synchronize()
graph = None
if not EAGER:
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        rollout()
main = torch.cuda.current_stream()


def update():
    logits = net(obs_buf.view(T * B, -1)).masked_fill(~mask_buf.view(T * B, -1), -1e9)
    logp_all = torch.log_softmax(logits, dim=1)
    logp = logp_all.gather(1, act_buf.view(-1, 1)).view(T, B)
    entropy = -(logp_all.exp() * logp_all).sum(dim=1).mean()
    ret = torch.zeros(B, device=dev)
    rets = []
    for t in reversed(range(T)):  # reward-to-go, discounted
        ret = rew_buf[t] + 0.95 * ret
        rets.append(ret)
    rets = torch.stack(rets[::-1])
    adv = rets - rets.mean(dim=1, keepdim=True)
    loss = -(logp * adv).mean() - 0.01 * entropy
    opt.zero_grad()
    loss.backward()
    opt.step()


torch.cuda.synchronize()
p0, a0 = env.totals()  # (the warm rollout above)
t0 = time.time()
for u_ in range(UPDATES):
    stream.wait_stream(main)
    with torch.cuda.stream(stream):
        if EAGER:
            rollout()
        else:
            graph.replay()
    main.wait_stream(stream)
    update()
    if u_ % 10 == 9 or u_ == UPDATES - 1:
        torch.cuda.synchronize()
        p1, a1 = env.totals()
        print("update %3d: blocking %.4f over the last %d steps, %.2f M env-steps/s incl. the network and the update"
              % (u_ + 1, 1 - (a1 - a0) / max(p1 - p0, 1), (p1 - p0) // B, (u_ + 1) * T * B / (time.time() - t0) / 1e6))
        p0, a0 = p1, a1
torch.cuda.synchronize()
print("agent on path features under the block mask (j = %d, placement %s): service blocking %.4f over %d steps of %d envs"
      % (J, PLACEMENT, blocking(env), env.totals()[0] // B, B))
env.check()
env.close()
