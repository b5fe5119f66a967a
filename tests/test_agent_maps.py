"""The oracle's walk of every case of tests/slot_agent.py meets the conditions the case exists for — judged here, on the CPU, so
that a scenario that stopped reaching the 64-slot edges (RMCSA: the high cores, the other modulations, every kind of refused
action; RWA: every word of the row) cannot pass as a green GPU test (tests/test_agent_maps_gpu.py replays
the same cached walks on the device) — and the specialisation libraries of the two-wavefront form that the GPU test asserts
are built here, where no hipcc run costs GPU time."""
import os
import shutil

import numpy as np
import pytest

from tests import slot_agent
from tests.slot_agent import CASES, PAIR_CASES

RMSA_CASES = [c for c in CASES if c.fam == "RMSA"]
RMCSA_CASES = [c for c in CASES if c.fam == "RMCSA"]
RWA_CASES = [c for c in CASES if c.fam == "RWA"]


@pytest.mark.parametrize("case", RMSA_CASES, ids=lambda c: c.name)
def test_agent_walk_reaches_the_word_edges(case):
    w = slot_agent.walk(case.name)
    S = case.S
    got = slot_agent.row_classes(w["samples"], S)
    rate = slot_agent.acceptance(w)
    print("%s: %d sampled rows, %r, acceptance %.3f" % (case.name, len(w["samples"]), got, rate))
    for what, count in got.items():
        assert count >= 1, "%s: no sampled row with %s" % (case.name, what)
    dones = np.array([s["done"] for s in w["steps"]]).sum(axis=0)
    assert (dones >= 2).all(), "%s: an env passed fewer than two episode boundaries" % case.name
    # a slot some agent-placed service held when the loop took over is free when it hands back: only a release frees a slot
    released = ((~w["before_run"]) & w["after_run"]).any(axis=(1, 2))
    assert released.all(), "%s: envs %r released no agent-placed service in the loop" % (case.name, np.flatnonzero(~released).tolist())
    if S <= 129:
        assert 0.5 < rate < 1.0, (case.name, rate)
    else:
        assert rate >= 0.5, (case.name, rate)
    # the agent's provisions themselves: one ends at S, one starts and one ends on a word boundary, one lies across one
    need = np.array([slot_agent.slots_needed(s["services"], slot_agent.topology()) for s in w["steps"]])
    acts = np.array([s["actions"] for s in w["steps"]]).astype(np.int64)
    ok = np.array([s["accepted"] for s in w["steps"]])
    start = acts[..., 1]
    end = start + np.take_along_axis(need, np.minimum(acts[..., 0], slot_agent.K - 1)[..., None], axis=2)[..., 0]
    assert (ok & (end == S)).any() and (S <= 65 or (ok & (start % 64 == 0) & (start > 0)).any())  # (S = 65: a start at 64 leaves one slot)
    assert (ok & (end % 64 == 0) & (end < S)).any() or S <= 65
    assert (ok & (start // 64 != (end - 1) // 64)).any()


@pytest.mark.parametrize("case", RMSA_CASES, ids=lambda c: c.name)
def test_first_fit_alone_never_uses_the_last_slot(case):
    """The control: the same configuration, seeds and length with SAP-FF at every step shows no row with slot S - 1 used."""
    w = slot_agent.control_walk(case.name)
    assert slot_agent.row_classes(w["samples"], case.S)["last_slot_used"] == 0
    assert w["after_run"][:, :, case.S - 1].all()
    assert not (w["samples"] == 1).all(), "the control's network is empty"


def test_random_deeprmsa_actions_take_late_blocks():
    case = slot_agent.CASE_BY_NAME["deep_s129_j4"]
    w = slot_agent.walk(case.name)
    j = case.kw["j"]
    acts = np.array([s["actions"][:, 0] for s in w["steps"]])
    ok = np.array([s["accepted"] for s in w["steps"]])
    late = ok & (acts < slot_agent.K * j) & (acts % j >= 2)
    print("%s: %d of %d provisions on a block of index >= 2, acceptance %.3f" % (case.name, late.sum(), ok.sum(), ok.mean()))
    assert late.any()
    assert (np.array([s["done"] for s in w["steps"]]).sum(axis=0) >= 2).all()
    assert all(s["obs"] is not None for s in w["steps"])


def _agent_arrays(w):
    acts = np.array([s["actions"] for s in w["steps"]]).astype(np.int64)
    meta = np.array([s["meta"] for s in w["steps"]])
    ok = np.array([s["accepted"] for s in w["steps"]])
    return acts, meta, ok


def _common_conditions(case, w):
    """(a) and (b) of every RMCSA and RWA case -> the acceptance over the agent steps"""
    rate = slot_agent.acceptance(w)
    assert 0.3 <= rate <= 0.9, (case.name, rate)
    assert abs(rate - case.acc) < 5e-4, "%s: the case table says %.3f, the walk gives %.3f" % (case.name, case.acc, rate)
    dones = np.array([s["done"] for s in w["steps"]]).sum(axis=0)
    assert (dones >= 2).all(), "%s: an env passed fewer than two episode boundaries" % case.name
    # a slot of some core that an agent-placed service (not one the heuristic placed in an earlier run) held when a run began is free
    # when it hands back: only a release frees a slot
    released = np.zeros(case.batch, bool)
    for r in w["runs"]:
        released |= r["agent_released"]
    assert released.all(), "%s: envs %r released no agent-placed service in a run" % (case.name, np.flatnonzero(~released).tolist())
    return rate


@pytest.mark.parametrize("case", RMCSA_CASES, ids=lambda c: c.name)
def test_rmcsa_agent_walk_reaches_core_modulation_and_word_edges(case):
    w = slot_agent.walk(case.name)
    S, C, E = case.S, slot_agent.cores_of(case), slot_agent.topology().n_links
    rate = _common_conditions(case, w)
    acts, meta, ok = _agent_arrays(w)
    kind, width = meta[..., 0], meta[..., 1]
    start, core = acts[..., 3], acts[..., 2]
    end = start + width
    prov = ok & (kind == slot_agent.PROVISION)
    assert (ok == prov).all(), "%s: an action meant to be refused was accepted" % case.name
    # every candidate the agent made out of the tables envs.py hands to the ABI (widths, both reach limits) is one to the oracle
    assert ok[kind == slot_agent.PROVISION].all(), "%s: a candidate from the batch's tables was refused by the oracle" % case.name
    got = dict(ends_at_S=int((prov & (end == S)).sum()), starts_on_word=int((prov & (start % 64 == 0) & (start > 0)).sum()),
               straddles=int((prov & (start // 64 != (end - 1) // 64)).sum()),
               top_core_with_room_below=int((prov & (core == C - 1) & (meta[..., 2] == 1)).sum()), non_best_mod=int((prov & (meta[..., 3] == 1)).sum()),
               widest=int(width[prov].max()))
    refused = {name: int((kind == i).sum()) for i, name in enumerate(slot_agent.KINDS)}
    # per run phase: the envs in which some core c > 0 holds more used slots than core 0 when the run begins
    fuller = [int(((~r["before"]).reshape(case.batch, C, E * S).sum(axis=2)[:, 1:].max(axis=1)
                   > (~r["before"]).reshape(case.batch, C, E * S).sum(axis=2)[:, 0]).sum()) for r in w["runs"]]
    # before a one-step launch: an env whose last action was accepted on a core >= 1 next to one whose last action carries the
    # reject index C as its core (the first launch follows the agent's step, the second and third the heuristic's own)
    mixed = [(int((r["last_accepted"] & (r["last_actions"][:, 2] >= 1)).sum()), int((r["last_actions"][:, 2] == C).sum()))
             for r in w["runs"] if r["length"] == 1]
    print("%s: load %g, acceptance %.3f, %r, refused %r, envs with a fuller core > 0 per run %r, (accepted on a core >= 1, core == C) before each one-step launch %r"
          % (case.name, case.load, rate, got, refused, fuller, mixed))
    assert got["ends_at_S"] >= 1 and got["top_core_with_room_below"] >= 1 and got["non_best_mod"] >= 1, (case.name, got)
    assert got["starts_on_word"] >= 1 or S <= 65, (case.name, got)
    assert got["straddles"] >= 1 or S <= 64, (case.name, got)
    assert all(f >= 1 for f in fuller), (case.name, fuller)
    assert len(mixed) == 3 and mixed[0][0] >= 1 and mixed[0][1] >= 1, (case.name, mixed)
    for name, count in refused.items():  # (d)
        if name == "beyond lmax_xt only":
            assert (count >= 1) == (case.name == slot_agent.WXT_CASE), (case.name, name, count)
        else:
            assert count >= 1, "%s: no refused action of kind %r" % (case.name, name)
    if case.name == slot_agent.RATES_CASE:
        assert got["widest"] >= slot_agent.WIDE, (case.name, got)
    if case.name == slot_agent.HIST_CASE:  # the cells of the 4-D histograms that only a partly rejecting action counts in
        M = len(slot_agent.topology().modulations)
        out = sum(w["histograms"][e][0] for e in slot_agent.HIST_ENVS)
        cells = dict(core_C=int(out[:slot_agent.K, :M, C, :S].sum()), mod_M=int(out[:slot_agent.K, M, :C, :S].sum()),
                     slot_S=int(out[:slot_agent.K, :M, :C, S].sum()))
        print("%s: envs %r, actions_output in the partly rejecting cells %r" % (case.name, slot_agent.HIST_ENVS, cells))
        assert all(v >= 1 for v in cells.values()), cells


@pytest.mark.parametrize("case", RMCSA_CASES, ids=lambda c: c.name)
def test_rmcsa_heuristic_alone_never_uses_the_last_slot(case):
    """(f) the control: SAP_BM_FC_FF at every step leaves slot S - 1 of every sampled row of every core free."""
    w = slot_agent.control_walk(case.name)
    assert (w["samples"][:, case.S - 1] == 1).all()
    assert all(r["after"][:, :, case.S - 1].all() for r in w["runs"])
    assert not (w["samples"] == 1).all(), "the control's network is empty"


@pytest.mark.parametrize("case", RWA_CASES, ids=lambda c: c.name)
def test_rwa_agent_walk_reaches_every_word(case):
    w = slot_agent.walk(case.name)
    S = case.S
    rate = _common_conditions(case, w)
    acts, meta, ok = _agent_arrays(w)
    wl = acts[..., 1]
    assert (ok <= (meta[..., 0] == slot_agent.PROVISION)).all(), "%s: a busy pair was accepted" % case.name
    per_word = np.bincount(wl[ok] // 64, minlength=(S + 63) // 64)
    sides = {b: (int((ok & (wl == b - 1)).sum()), int((ok & (wl == b)).sum())) for b in range(64, S, 64)}
    top, busy = int((ok & (wl == S - 1)).sum()), int(((meta[..., 0] == slot_agent.BUSY_PAIR) & ~ok).sum())
    print("%s: load %g, acceptance %.3f, accepted per word %r, on S - 1 %d, below / on each word boundary %r, refused busy pairs %d"
          % (case.name, case.load, rate, per_word.tolist(), top, sides, busy))
    assert (per_word >= 1).all() and top >= 1 and busy >= 1, case.name
    assert all(lo >= 1 and hi >= 1 for lo, hi in sides.values()), (case.name, sides)
    assert all(s["masks"].keys() == {"joint", "path"} for s in w["steps"] if "masks" in s)


def test_reference_fixtures_hold_the_refused_kinds():
    """The g11 fixtures (oracle/gen_golden_agent.py: one env of three walks replayed in the reference) still hold what they were
    recorded for: every kind of refused RMCSA action, beyond lmax_xt alone in the worst_xt fixture, refused busy RWA pairs, and
    the stored stream is the walk's."""
    from tests.helpers import load_golden

    for name, _case, kinds in slot_agent.REFERENCE_FIXTURES:
        g = load_golden(name)
        meta = g["meta"]
        got = np.array(meta["kinds"])
        assert kinds <= set(got.tolist()), (name, sorted(set(got.tolist())))
        refused = np.isin(got, sorted(kinds))
        assert (g["reward"][refused] == 0).all(), name
        w = slot_agent.walk(meta["case"])
        width = g["actions"].shape[1]
        agent_steps = np.flatnonzero(got != slot_agent.RUN_STEP)
        assert np.array_equal(g["actions"][agent_steps], np.array([s["actions"][meta["env_index"], :width] for s in w["steps"]])), name


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_form_specialisations_are_built(name, monkeypatch):
    from optical_rl_gym_amd import _build
    from tests.helpers import force_impl

    force_impl(monkeypatch, "persist_pair")
    case = slot_agent.CASE_BY_NAME[name]
    flags = slot_agent.spec_flags_of(case)
    # (RMCSA's specialisation is the one-wavefront kernel: no row wavefront to ask for)
    assert flags and ("-DORL_SPEC_RW=1" in flags or case.fam == "RMCSA"), flags
    path = _build.build_spec(flags)
    assert os.path.exists(path) and path == _build.spec_path(flags)
