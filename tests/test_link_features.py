"""The per-link feature observation (include/orl.h, orl_batch_link_features) without a GPU: the ABI surface, the kernel in the code
object, the numpy restatement the GPU tests compare with — its vectorised form against the slow one for every family, its two
statistics columns against the oracle's own running averages, bit for bit —, the walks of the GPU suite over the oracle (what
their states hold), and OpticalVecEnv's "link_features" observation over the oracle."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from optical_rl_gym_amd.vec_env import OpticalVecEnv
from tests import link_features_restate as lf
from tests import path_features_restate as pf
from tests import slot_agent
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPOLOGY = slot_agent.TOPOLOGY
K, N, E = 5, 14, 22


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_header_and_binding_declare_the_link_features():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"#define ORL_BUF_LINK_FEATURES 10\b", h)
    assert re.search(r"int orl_batch_link_features_shape\(const orl_batch\* b, int32_t\* dim, int32_t\* rows, int32_t\* width, int32_t\* pitch\);", h)
    assert re.search(r"int orl_batch_link_features\(orl_batch\* b, float\* out[^;]*\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    assert len(_lib.EXPORTS["orl_batch_link_features_shape"][1]) == 5 and len(_lib.EXPORTS["orl_batch_link_features"][1]) == 2


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_link_feature_kernels_exist_for_every_row_width_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    lib = _build.build()
    found = {}
    for k in kernel_regs.kernels(lib):
        m = re.match(r"(?:void )?k_link_features<(\d+)>", kernel_regs.demangle(k["name"]))
        if m:
            found[int(m.group(1))] = k
    assert sorted(found) == list(_build.ROW_WIDTHS)
    for w, k in found.items():
        assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, (w, k)


def test_slow_and_fast_restatement_agree():
    for fam, kw in (("RMSA", pf.RMSA_S64_KW), ("RMSA", slot_agent.CASE_BY_NAME["rmsa_s65"].kw), ("RWA", pf.RWA_S16_KW)):
        ora = OracleBackend(fam, TOPOLOGY, list(range(20, 36)), **kw)
        rng = np.random.default_rng(1)
        for _ in range(3):
            pf.walk(ora, rng, 40)
            env_type, avail, services = pf.state_of(ora)
            lstat = ora.link_stats_all()
            slow = lf.restate(env_type, avail, services, ora.topology, lstat)
            assert slow.shape == (16, 1 + 2 * N + E * (10 + K)) and lf.shape_of(ora.topology, 1) == (slow.shape[1], E, 10 + K)
            assert np.array_equal(_bits(slow), _bits(lf.restate_fast(env_type, avail, services, ora.topology, lstat))), fam
            assert np.array_equal(slow[:, 0], np.zeros(16) if fam == "RWA" else services[:, 4] / 100)
            assert (slow[:, 1:1 + 2 * N].sum(axis=1) == 2).all()
            blk = lf.blocks_of(slow, ora.topology, 1)
            assert np.array_equal(blk[:, 0, :, 7:10], np.transpose(lstat[:, 0:3, :], (0, 2, 1)))
            src, dst = services[:, 2].astype(int), services[:, 3].astype(int)
            hops = np.where(np.arange(K)[None, :] < ora.topology.n_paths[src, dst][:, None], ora.topology.path_hops[src, dst], 0)
            assert np.array_equal(blk[:, 0, :, 10:].sum(axis=1), hops)  # a path's column holds one 1 per hop
    from tests.test_path_features import _rmcsa_oracle

    C, S = 3, 40
    ora, _tab = _rmcsa_oracle(C, S, 12, 60)
    env_type, avail, services = pf.state_of(ora)
    lstat = ora.link_stats_all()
    slow = lf.restate(env_type, avail, services, ora.topology, lstat)
    assert slow.shape == (12, 1 + 2 * N + C * E * (10 + K))
    assert np.array_equal(_bits(slow), _bits(lf.restate_fast(env_type, avail, services, ora.topology, lstat)))
    blk = lf.blocks_of(slow, ora.topology, C)
    assert (blk[:, :1, :, :7] != blk[:, :, :, :7]).any()  # two cores of one link differ somewhere ...
    assert np.array_equal(blk[:, :1, :, 7:].repeat(C, axis=1), blk[:, :, :, 7:])  # ... but for the link's own columns


def test_statistics_columns_equal_what_the_oracle_feeds_its_averages():
    """Columns 5 and 6 are cur_external_fragmentation and cur_link_compactness of _update_link_stats: on every step of an env in
    which nothing was released (its active count rose by one with the accepted service, or stayed with a refused one), for every
    link whose last_update changed, the oracle's new averages are ((old * last_update) + (cur * time_diff)) / now with `cur` from
    the restatement of the map after the step, bit for bit."""
    ora = OracleBackend("RMSA", TOPOLOGY, list(range(64)), **slot_agent.CASE_BY_NAME["rmsa_s65"].kw)
    rng = np.random.default_rng(65)
    checked = two_edge = fragmented = loose = 0
    for _ in range(150):
        old, act0, acc0 = ora.link_stats_all(), ora.active().astype(np.int64), ora.counters()[:, 1].copy()
        ora.step(pf.random_actions(ora, rng), auto_reset=True)
        new, act1, accepted = ora.link_stats_all(), ora.active().astype(np.int64), (ora.counters()[:, 1] - acc0) == 1
        quiet = np.where(accepted, act1 - act0 == 1, act1 == act0)
        env, link = np.nonzero(quiet[:, None] & (new[:, 3, :] != old[:, 3, :]))
        if not len(env):
            continue
        env_type, avail, services = pf.state_of(ora)
        blk = lf.blocks_of(lf.restate_fast(env_type, avail, services, ora.topology, new), ora.topology, 1)[env, 0, link]
        now, last_update = new[env, 3, link], old[env, 3, link]
        time_diff = now - last_update
        assert (now > 0).all() and (time_diff > 0).all()
        for col, cur in ((1, blk[:, 5]), (2, blk[:, 6])):
            want = ((old[env, col, link] * last_update) + (cur * time_diff)) / now
            assert np.array_equal(_bits(want), _bits(new[env, col, link])), col
        q = lf.row_facts(avail[env, 0, link])
        checked += len(env)
        two_edge += int(((q["runs"] == 2) & (q["ends"] == 2) & (blk[:, 5] == 1.0)).sum())  # max_empty = 0 with two edge runs
        fragmented += int(((q["runs"] >= 3) & (blk[:, 5] > 0.0) & (blk[:, 5] < 1.0)).sum())
        loose += int((blk[:, 6] < 1.0).sum())
    print("checked %d (step, link) pairs: %d with two edge runs, %d with three or more free runs, %d with compactness < 1"
          % (checked, two_edge, fragmented, loose))
    assert checked >= 1000 and two_edge >= 1 and fragmented >= 1 and loose >= 1


def _walk_case(name):
    fam = "RWA" if name.startswith("rwa") else "RMSA"
    if name == "rmsa_s64":
        return fam, pf.RMSA_S64_KW, 64
    if name == "rwa_s16":
        return fam, pf.RWA_S16_KW, 16
    case = slot_agent.CASE_BY_NAME[name]
    return fam, case.kw, case.S


def test_the_gpu_walks_hold_their_rows_on_the_oracle():
    """What tests/test_link_features_gpu.py relies on (lf.WALK_HOLDS): together the checked states hold entirely free rows, rows
    without a free slot, longest free runs that cross a 64-slot word boundary at S = 129 and S = 512, and a free slot S - 1 at
    S = 65."""
    for name, holds in lf.WALK_HOLDS.items():
        fam, kw, S = _walk_case(name)
        ora = OracleBackend(fam, TOPOLOGY, pf.walk_seeds(S), **kw)
        rng, seen = np.random.default_rng(S), lf.Seen()
        for _point in pf.WALK_POINTS:
            pf.walk(ora, rng, 60)
            seen.add(pf.state_of(ora)[1])
        print(name, vars(seen))
        for what in holds:
            assert getattr(seen, what) >= 1, (name, what)
    held = {what for holds in lf.WALK_HOLDS.values() for what in holds}
    assert held == {"free_rows", "full_rows", "crossing", "top_free"}
    assert "crossing" in lf.WALK_HOLDS["rmsa_s129"] and "crossing" in lf.WALK_HOLDS["rmsa_s512"] and "top_free" in lf.WALK_HOLDS["rmsa_s65"]


class LinkOracle(OracleBackend):
    """The oracle stand-in with a `link_features` of its own: the numpy restatement on its read-back state."""

    def link_features_shape(self):
        dim, R, F = lf.shape_of(self.topology, self.C)
        return dim, R, F, (dim + 3) // 4 * 4

    def link_features(self, fetch=True, out=None):
        rows = np.float32(lf.of_batch(self, fast=False))
        if out is None:
            return rows
        out[...] = rows
        return out


@pytest.mark.parametrize("fam,kw", [("RMSA", pf.RMSA_S64_KW), ("DeepRMSA", dict(pf.RMSA_S64_KW, j=2)), ("RWA", pf.RWA_S16_KW)])
def test_vecenv_hands_out_the_link_features(fam, kw):
    batch = LinkOracle(fam, TOPOLOGY, list(range(30, 38)), **dict(kw, episode_length=10))
    venv = OpticalVecEnv(batch, observation="link_features")
    dim = 1 + 2 * N + E * (10 + K)
    sp = venv.observation_space
    assert sp.shape == (dim,) and sp.dtype == np.float32 and float(np.min(sp.low)) == -2.0 ** 30 and float(np.max(sp.high)) == 2.0 ** 30
    obs = venv.reset()
    assert obs.shape == (8, dim) and obs.dtype == np.float32
    assert np.array_equal(obs.view(np.uint32), np.float32(lf.of_batch(batch)).view(np.uint32))
    rng = np.random.default_rng(1)
    finished = 0
    for _ in range(24):
        held = obs
        before = held.copy()
        obs, _reward, done, infos = venv.step(pf.random_actions(batch, rng))
        assert obs.shape == (8, dim) and obs.dtype == np.float32 and np.abs(obs).max() <= 2.0 ** 30
        assert np.array_equal(obs.view(np.uint32), np.float32(lf.of_batch(batch)).view(np.uint32))
        assert np.array_equal(held, before)  # the rows a step handed out stay as they were over the next step
        for i in np.flatnonzero(done):  # the soft reset keeps the pending service, the maps and the links' averages
            assert np.array_equal(infos[i]["terminal_observation"], obs[i])
            finished += 1
    assert finished >= 8
