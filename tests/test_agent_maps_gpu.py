"""Agent-made slot maps through every step implementation, then handed to the device loop (tests/slot_agent.py holds the agents, the
cases and the oracle's walk; tests/test_agent_maps.py checks on the CPU that the walk reaches what it exists for).  RMSA: 120 steps
of a boundary-seeking agent — provisions that end at S, start or end on a word boundary, lie across one —, run() of the loop's
heuristic for 100 steps on the map they left, 40 agent steps more.  RMCSA: an agent that chooses (path, modulation, core, slot) —
high cores, modulations other than the best, the word edges of every core, every kind of refused and partly rejecting action —, three
launches of one step on the prev_core values it left, agent, a run of 60 steps, agent.  RWA: wavelengths in every word of rows up to
8 words wide, busy pairs, a run of SAP_LF.  Every step's reward, done and info (DeepRMSA: the observation too) equal the oracle's;
at every 10th step so do the heuristics' answers and the action masks the family has; after each phase EVERY env equals the oracle
in counters, pending service, pending releases, packed slot maps of all cores, link and network statistics.  The host phases run
under k_step, k_agent and the two-kernel form, the loop under every form of the persistent kernel the family has."""
import numpy as np
import pytest

from tests import slot_agent
from tests.helpers import _exact, _ran_pair_form, force_impl
from tests.run_plans import expected_form, forms_of_family
from tests.slot_agent import CASES, LOOP_POLICY, PAIR_CASES, TOPOLOGY

pytestmark = pytest.mark.gpu

HOST_IMPLS = ("wave64", "agent8", "split2")
LOOP_IMPLS = ("persist", "persist_global", "persist_lds", "persist_rd")


def loop_impls_of(case):
    """the forms of the persistent kernel the family has (tests/run_plans.py, FAMILY_FORMS: RMCSA is built in neither the LDS-resident
    nor the rows-deferred form)"""
    return tuple(f for f in LOOP_IMPLS if f in forms_of_family(case.fam))


def _params():
    out = []
    for c in CASES:
        for impl in HOST_IMPLS + loop_impls_of(c) + (("persist_pair",) if c.name in PAIR_CASES else ()):
            out.append(pytest.param(c, impl, id="%s-%s" % (c.name, impl)))
    return out


@pytest.mark.parametrize("case,impl", _params())
def test_walk_on_the_device_equals_the_oracle(case, impl, monkeypatch):
    import optical_rl_gym_amd as orl

    w = slot_agent.walk(case.name)
    force_impl(monkeypatch, impl)
    dev = orl.make(case.fam, topology=TOPOLOGY, num_envs=case.batch, seeds=slot_agent.seeds_of(case), **dict(case.kw, **case.dev_kw))
    chk = _exact("%s %s" % (case.name, impl))
    steps = iter(w["steps"])
    for phase, (kind, length) in enumerate(slot_agent.phases_of(case)):
        if kind == "run":
            st = dev.run(LOOP_POLICY[case.fam], length)
            names = [n for n, _ in st.kernels()]
            form = int(dev.lib.orl_batch_debug_persist_form(dev._h))
            if impl in ("wave64", "split2"):
                assert names == [] and form == -1, (case.name, impl, names, form)
            else:
                assert names == ["k_persist"] and form >= 0, (case.name, impl, names, form)
            if impl == "persist_pair":  # (RMCSA: the one-wavefront kernel, specialised)
                assert dev.specialised and _ran_pair_form(dev) == (case.fam != "RMCSA"), (case.name, form)
            # global state: 0, RMCSA 1; rows deferred 7: the map is changed in the loop, k_rowstats replays the statistics.  Not
            # "persist_lds": where the LDS-resident form does not fit the configuration, the library's default form runs
            if impl in ("persist_global", "persist_rd"):
                assert form == expected_form(case, impl), (case.name, impl, form)
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
    assert not dev.flags().any()  # (refused and partly rejecting actions are legal: no bad-action flag)
    dev.check()
    for e, want in w.get("histograms", {}).items():  # cells [path][mod][C][slot], [path][M][core][slot], [path][mod][core][S] among them
        got = dev.action_histograms_of(e)
        chk(e, "actions_output", got[0], want[0])
        chk(e, "actions_taken", got[1], want[1])
    dev.close()
