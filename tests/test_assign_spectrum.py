"""Spectrum-assignment rules for RMSA and RWA actions (include/orl.h, orl_batch_assign_spectrum) without a GPU: the ABI surface, the
kernel in the code object, the facades, and the numpy restatement the GPU tests compare with (tests/assign_restate.py) — pinned to
the oracle's own step on agent-made states, to the joint mask's restatement and to a brute-force loop per rule — with the
preconditions of the GPU test established on the states that test uses (tests/assign_cases.py walks either backend)."""
import functools
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from tests import assign_cases as ac
from tests import assign_restate as ar
from tests import mask_restate
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = ac.K
STATE_SEEDS = tuple(range(300, 316))  # one walked state per seed and point
POINTS = (30, 90)                     # agent steps before the probe
PROBES = [(rule, g) for rule in ar.RULES for g in (0, 1)]


def test_header_and_binding_declare_the_rules():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_assign_spectrum\(orl_batch\* b, int rule, int n_given,\s*const int32_t\* given[^;]*,\s*int32_t\* actions_out[^;]*\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    assert len(_lib.EXPORTS["orl_batch_assign_spectrum"][1]) == 5
    from optical_rl_gym_amd.envs import BatchedOpticalEnv

    for name, rid in BatchedOpticalEnv.ASSIGN_RULES.items():
        const = {"first": "FIRST_FIT", "last": "LAST_FIT", "best": "BEST_FIT", "exact": "EXACT_FIT"}.get(name, name.upper())
        assert re.search(r"#define ORL_ASSIGN_%s %d\b" % (const, rid), h), name
    assert tuple(BatchedOpticalEnv.ASSIGN_RULES) == ar.RULES
    for word in ("s = S - n is tried", r"reject action \(k, S\)", "all of them, not only those on the path"):
        assert re.search(word, h), word


def test_facades_offer_the_rules_to_rmsa_and_rwa_only():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd import gym_api
    from optical_rl_gym_amd.sharding import MultiDeviceBatch
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    assert hasattr(gym_api.RMSAEnv, "assign_spectrum") and hasattr(gym_api.RWAEnv, "assign_spectrum")
    assert not hasattr(gym_api.DeepRMSAEnv, "assign_spectrum") and not hasattr(gym_api.RMCSAEnv, "assign_spectrum")
    assert hasattr(orl.envs.BatchedOpticalEnv, "assign_spectrum") and hasattr(MultiDeviceBatch, "assign_spectrum")
    with pytest.raises(ValueError):
        orl.envs.BatchedOpticalEnv.assignment_rule("worst")
    p, n = orl.envs.BatchedOpticalEnv.assignment_paths(np.arange(4), None, 4)
    assert p.dtype == np.int32 and n == 1 and orl.envs.BatchedOpticalEnv.assignment_paths(None, None, 4) == (None, 0)
    for bad in (np.zeros((4, 1), np.int32), np.zeros(3, np.int32), np.zeros(4, np.float64)):
        with pytest.raises(ValueError):
            orl.envs.BatchedOpticalEnv.assignment_paths(bad, None, 4)
    rmcsa = OracleBackend("RMCSA", "nsfnet_chen", [1, 2], load=100, num_spectrum_resources=64, num_spatial_resources=7)
    with pytest.raises(ValueError, match="RMSA and RWA"):
        OpticalVecEnv(rmcsa, spectrum_assignment="best")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernels_exist_for_every_row_width_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    lib = _build.build()
    found = {}
    for k in kernel_regs.kernels(lib):
        m = re.match(r"(?:void )?k_assign_spectrum<(\d+), (true|false)>", kernel_regs.demangle(k["name"]))
        if m:
            found[int(m.group(1)), m.group(2)] = k
    assert sorted(found) == sorted((w, c) for w in _build.ROW_WIDTHS for c in ("false", "true"))
    for key, k in found.items():
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, (key, k)


def _joint(shape, avail, services):
    topo = ac.topology(shape.topology)
    rows = mask_restate.restate_fast(ac.ENV_TYPE[shape.fam], avail, services, topo, K, shape.S, allow_rejection=True, fallback=False)[:, :-1]
    return rows.reshape(len(services), K, shape.S)


def check_state(shape, avail, services, rng, seen):
    """The restated answers of one state against the joint mask's restatement (every returned column is set; the reject action
    exactly when the row, or the given path's columns, are empty) and each rule against the brute-force loop; returns them"""
    joint = _joint(shape, avail, services)
    done, prep = ac.expected(shape, avail, services, rng, seen)
    n = len(services)
    for rule, g, given, want in done:
        rej = (want[:, :2] == (K, shape.S)).all(axis=1)
        assert (want[:, 2:] == 0).all() and ((want[:, 0] == K) == rej).all()
        ok = np.flatnonzero(~rej)
        assert joint[ok, want[ok, 0], want[ok, 1]].all(), (rule, g)
        if g:
            inside = (given >= 0) & (given < K)
            room = np.zeros(n, bool)
            room[inside] = joint[np.flatnonzero(inside), given[inside]].any(axis=1)
            assert (want[ok, 0] == given[ok]).all()
        else:
            room = joint.any(axis=(1, 2))
            assert (want[ok, 0] == joint[ok].any(axis=2).argmax(axis=1)).all()  # the first path that fits
        assert np.array_equal(rej, ~room), (rule, g)
        for i in ok[:48]:  # (the loop over all s per env: on a part of the larger batches)
            assert ar.brute(prep, int(i), int(want[i, 0]), rule) == int(want[i, 1]), (rule, g, int(i))
    return done


@functools.lru_cache(maxsize=None)
def _probe(name, steps):
    """One oracle state per seed after `steps` agent steps, each held by one env per probe (the oracle has no snapshot: the envs of
    a seed take identical actions until the probe), then every probe's restated action stepped."""
    shape = ac.SHAPE_BY_NAME[name]
    R, G = len(PROBES), len(STATE_SEEDS)
    lead = np.arange(G) * R
    ora = OracleBackend(shape.fam, shape.topology, list(np.repeat(STATE_SEEDS, R)), **shape.kw)
    small = shape._replace(envs=G)
    rng = np.random.RandomState(steps + shape.S)

    class Lead:  # the lead envs as a backend of their own; a step repeats their actions over the replicas
        def slots_packed(self):
            return ora.slots_packed()[lead]

        def services(self):
            return ora.services()[lead]

        def policy(self, name):
            return np.array(ora.policy(name))[lead]

        def step(self, acts, auto_reset):
            ora.step(np.repeat(acts, R, axis=0), auto_reset=auto_reset)

    ac.agent_steps(Lead(), small, steps, rng)
    avail, services = ac.state_of(Lead(), small)
    assert (ora.services() == np.repeat(services, R, axis=0)).all()
    seen = {}
    done = check_state(small, avail, services, np.random.default_rng(steps), seen)
    actions = np.zeros((G * R, 4), np.int32)
    for j, (rule, g, given, want) in enumerate(done):
        assert (rule, g) == PROBES[j]
        actions[lead + j] = want
    before = ora.counters()[:, 1].copy()
    ora.step(actions, auto_reset=False)
    accepted = ora.counters()[:, 1] - before
    # the oracle provisions the service exactly when the answer is not the reject action
    assert np.array_equal(accepted == 1, actions[:, 0] < K) and set(np.unique(accepted)) <= {0, 1}
    return seen


@pytest.mark.parametrize("name", ac.CPU_SHAPES)
@pytest.mark.parametrize("steps", POINTS)
def test_restated_choice_is_what_the_oracle_provisions(name, steps):
    print(name, steps, _probe(name, steps))


@functools.lru_cache(maxsize=None)
def _kinds(name):
    """What the states of the GPU test hold for a shape, here from the oracle: the walked state and its crowded maps"""
    shape = ac.SHAPE_BY_NAME[name]
    ora = OracleBackend(shape.fam, shape.topology, ac.seeds_of(shape), **shape.kw)
    ac.agent_steps(ora, shape, ac.AGENT_STEPS, np.random.RandomState(shape.S))
    avail, services = ac.state_of(ora, shape)
    seen = {}
    rng = np.random.default_rng(shape.S)
    check_state(shape, avail, services, rng, seen)
    check_state(shape, ac.crowd(shape, avail, services), services, rng, seen)
    return seen


@pytest.mark.parametrize("fam", ["RMSA", "RWA"])
def test_the_states_hold_every_kind_the_gpu_test_needs(fam):
    """Per family, over the states tests/test_assign_spectrum_gpu.py checks for the shapes walked here too: no completion, s* = S - n,
    a chosen free run across a word edge (RMSA: the chosen window too), a best-fit tie, a most- / least-used tie, a given path >=
    n_paths and a negative one, n_given = 0 on a path other than 0, and for every rule but first fit an answer that differs from
    first fit's."""
    total = {}
    for name in ac.CPU_SHAPES:
        if ac.SHAPE_BY_NAME[name].fam == fam:
            for kind, c in _kinds(name).items():
                total[kind] = total.get(kind, 0) + c
    print(fam, total)
    missing = [kind for kind in (ar.RMSA_KINDS if fam == "RMSA" else ar.KINDS) if total.get(kind, 0) == 0]
    assert not missing, (missing, total)
