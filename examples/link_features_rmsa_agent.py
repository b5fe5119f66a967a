#!/usr/bin/env python3
"""A graph-style agent on the same GPU as RMSA-v0 envs — the loop of examples/path_features_rmsa_agent.py with the state seen per
LINK: what the agent sees is the batch's link features (`link_features(fetch=False)`: float32 rows built on the device, one block
of 10 + k values per link), what it may do the "path" action mask, and what it chooses a path — PathOnlyFirstFitAction's
Discrete(k + 1): the agent writes its path into the batch's "paths" array, `policy("PATH_FF", fetch=False)` finds the first fit on
that path on the device and `step(None, fetch=False)` takes it.  Nothing crosses PCIe in the rollout, and the whole rollout of T
steps is captured once in a `torch.cuda.CUDAGraph` on the batch's stream.

The network is the smallest one that uses the topology: one MLP shared by all links over a link's 10 + k columns (and the service's
bit rate), its outputs mean-pooled along each candidate path with the block's on-path columns, one linear head per pooled path
and a learned logit for the reject action; a softmax over the paths under the mask.  It is trained with a plain policy-gradient
update (reward-to-go, batch-mean baseline, entropy bonus); the point is the data path, not the algorithm.  Blocking is printed
beside the SAP-FF heuristic's on the same seeds: measured, no threshold.

    python examples/link_features_rmsa_agent.py [num_envs] [updates] [--eager]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # run from a source checkout

import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
EAGER = "--eager" in sys.argv
B = int(args[0]) if len(args) > 0 else 4096
UPDATES = int(args[1]) if len(args) > 1 else 60
T = 32  # steps per rollout
EPISODE = 50
kw = dict(topology="nsfnet_chen", load=300, mean_service_holding_time=25, episode_length=EPISODE, num_spectrum_resources=100,
          allow_rejection=True)
STEPS = UPDATES * T

# the heuristic on the same seeds and as many steps, entirely on the device
ref = orl.make("RMSA-v0", num_envs=B, seeds=1, **kw)
ref.run("SAP_FF", STEPS)
processed, accepted = ref.totals()
print("SAP_FF heuristic: blocking %.4f over %d steps of %d envs" % (1 - accepted / processed, STEPS, B))
ref.close()

env = orl.make("RMSA-v0", num_envs=B, seeds=1, **kw)
dev = "cuda:%d" % env.device_id
K = env.k_paths
n_actions = K + 1  # a path, or reject
env.reset()
env.link_features(fetch=False)  # (the first calls allocate the device buffers: outside the capture)
env.action_mask("path", fetch=False)
feat = env.device_tensor("link_features")                   # float32 [B, dim] at the device pitch, no copy
mask = env.device_tensor("action_mask")[:, :n_actions]      # bool
paths, rew = env.device_tensor("paths"), env.device_tensor("reward")
dim, R, F, _pitch = env.link_features_shape()
HEAD = dim - R * F  # the header: bit rate, source and destination one-hots


class LinkNet(torch.nn.Module):
    def __init__(self, hidden=64, out=32):
        super().__init__()
        self.link = torch.nn.Sequential(torch.nn.Linear(F + 1, hidden), torch.nn.ELU(), torch.nn.Linear(hidden, hidden), torch.nn.ELU(),
                                        torch.nn.Linear(hidden, out), torch.nn.ELU())
        self.head = torch.nn.Linear(out, 1)
        self.reject = torch.nn.Parameter(torch.zeros(1))

    def forward(self, rows):  # [n, dim] -> logits [n, k + 1]
        n = rows.shape[0]
        blocks = rows[:, HEAD:].reshape(n, R, F)
        rate = rows[:, :1, None].expand(n, R, 1)
        h = self.link(torch.cat([blocks, rate], dim=2))                  # [n, links, out]
        on_path = blocks[:, :, F - K:]                                   # [n, links, k]: 1.0 where the link is on path p
        pooled = torch.einsum("nlp,nlo->npo", on_path, h) / on_path.sum(dim=1).clamp_(min=1.0)[:, :, None]
        return torch.cat([self.head(pooled).squeeze(2), self.reject.expand(n, 1)], dim=1)


net = LinkNet().to(dev)
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
            paths.copy_(a.int())
        env.policy("PATH_FF", fetch=False)                 # first fit on the chosen path -> the actions array
        env.step(None, auto_reset=True, fetch=False)       # one launch; reward / done are rewritten in place
        env.link_features(fetch=False)                     # what the agent sees next
        env.action_mask("path", fetch=False)               # what it may do next
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
processed, accepted = env.totals()
print("agent on link features (%d links x %d values) under the path mask: blocking %.4f over %d steps of %d envs"
      % (R, F, 1 - accepted / processed, processed // B, B))
env.check()
env.close()
