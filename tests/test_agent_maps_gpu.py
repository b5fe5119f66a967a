"""Agent-made slot maps through every step implementation, then handed to the device loop (tests/slot_agent.py holds the agent, the
cases and the oracle's walk; tests/test_agent_maps.py checks on the CPU that the walk reaches the 64-slot edges): 120 steps of a
boundary-seeking agent — provisions that end at S, start or end on a word boundary, lie across one —, run() of the loop's heuristic
for 100 steps on the map they left, 40 agent steps more.  Every step's reward, done and info (DeepRMSA: the observation too) equal
the oracle's; at every 10th step so do the heuristics' answers and both action masks; after each phase EVERY env equals the oracle
in counters, pending service, pending releases, packed slot maps, link and network statistics.  The host phases run under k_step,
k_agent and the two-kernel form, the loop under every form of the persistent kernel."""
import numpy as np
import pytest

from tests import slot_agent
from tests.helpers import _exact, _ran_pair_form, force_impl
from tests.slot_agent import CASES, LOOP_POLICY, PAIR_CASES, PHASES, TOPOLOGY

pytestmark = pytest.mark.gpu

HOST_IMPLS = ("wave64", "agent8", "split2")
LOOP_IMPLS = ("persist", "persist_global", "persist_lds", "persist_rd")


def _params():
    out = []
    for c in CASES:
        for impl in HOST_IMPLS + LOOP_IMPLS + (("persist_pair",) if c.name in PAIR_CASES else ()):
            out.append(pytest.param(c, impl, id="%s-%s" % (c.name, impl)))
    return out


@pytest.mark.parametrize("case,impl", _params())
def test_walk_on_the_device_equals_the_oracle(case, impl, monkeypatch):
    import optical_rl_gym_amd as orl

    w = slot_agent.walk(case.name)
    force_impl(monkeypatch, impl)
    dev = orl.make(case.fam, topology=TOPOLOGY, num_envs=case.batch, seeds=slot_agent.seeds_of(case), **case.kw)
    chk = _exact("%s %s" % (case.name, impl))
    steps = iter(w["steps"])
    for phase, (kind, length) in enumerate(PHASES):
        if kind == "run":
            st = dev.run(LOOP_POLICY[case.fam], length)
            names = [n for n, _ in st.kernels()]
            form = int(dev.lib.orl_batch_debug_persist_form(dev._h))
            if impl in ("wave64", "split2"):
                assert names == [] and form == -1, (case.name, impl, names, form)
            else:
                assert names == ["k_persist"] and form >= 0, (case.name, impl, names, form)
            if impl == "persist_pair":
                assert _ran_pair_form(dev), (case.name, form)
            if impl == "persist_rd":
                assert form == 7, (case.name, form)  # rows deferred: the map is changed in the loop, k_rowstats replays the statistics
        else:
            for _ in range(length):
                rec = next(steps)
                t = rec["t"]
                chk(t, "pending service", dev.services(), rec["services"])
                if "masks" in rec:  # (every 10th step; neither query steps the batch)
                    for name, want in rec["policies"].items():
                        chk(t, "policy " + name, dev.policy(name), want)
                    for layout, want in rec["masks"].items():
                        got = dev.action_mask(layout)
                        assert got.shape == want.shape, (case.name, layout, got.shape, want.shape)
                        bad = np.flatnonzero((got != want).any(axis=1))
                        assert len(bad) == 0, "%s %s step %d, %s mask: %d envs differ, first %d" % (case.name, impl, t, layout, len(bad), bad[0])
                obs, reward, done, info = dev.step(rec["actions"], auto_reset=True)
                chk(t, "reward", reward, rec["reward"])
                chk(t, "done", done, rec["done"])
                chk(t, "info", info, rec["info"])
                if rec["obs"] is not None:
                    chk(t, "obs", obs, rec["obs"])
        want = w["states"][phase]
        chk(phase, "counters", dev.counters(), want["counters"])
        chk(phase, "services", dev.services(), want["services"])
        chk(phase, "active", dev.active(), want["active"])
        chk(phase, "slot maps", dev.slots_packed(), want["slots_packed"])
        chk(phase, "link statistics", dev.link_stats_all(), want["link_stats_all"])
        chk(phase, "network statistics", dev.net_stats_all(), want["net_stats_all"])
    assert not dev.flags().any()
    dev.check()
    dev.close()
