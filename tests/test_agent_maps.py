"""The oracle's walk of every case of tests/slot_agent.py meets the conditions the case exists for — judged here, on the CPU, so
that a scenario that stopped reaching the 64-slot edges cannot pass as a green GPU test (tests/test_agent_maps_gpu.py replays
the same cached walks on the device) — and the specialisation libraries of the two-wavefront form that the GPU test asserts
are built here, where no hipcc run costs GPU time."""
import os
import shutil

import numpy as np
import pytest

from tests import slot_agent
from tests.slot_agent import CASES, PAIR_CASES

RMSA_CASES = [c for c in CASES if c.fam == "RMSA"]


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


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_form_specialisations_are_built(name, monkeypatch):
    from optical_rl_gym_amd import _build
    from tests.helpers import force_impl

    force_impl(monkeypatch, "persist_pair")
    flags = slot_agent.spec_flags_of(slot_agent.CASE_BY_NAME[name])
    assert flags and "-DORL_SPEC_RW=1" in flags, flags
    path = _build.build_spec(flags)
    assert os.path.exists(path) and path == _build.spec_path(flags)
