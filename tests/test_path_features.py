"""The path-feature observation (include/orl.h, orl_batch_path_features) without a GPU: the ABI surface, the kernel in the code
object, the numpy restatement the GPU tests compare with — checked against the oracle's own DeepRMSA observation, bit for bit —
its vectorised form against the slow one for every family, the walks of the GPU suite over the oracle (what their states hold),
and OpticalVecEnv's "path_features" observation over the oracle."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from optical_rl_gym_amd.vec_env import OpticalVecEnv
from tests import path_features_restate as pf
from tests import rmcsa_mask_restate as rr
from tests import slot_agent
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_header_and_binding_declare_the_path_features():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"#define ORL_BUF_PATH_FEATURES 9\b", h)
    assert re.search(r"int orl_batch_path_features_shape\(const orl_batch\* b, int j, int32_t\* dim, int32_t\* rows, int32_t\* pitch\);", h)
    assert re.search(r"int orl_batch_path_features\(orl_batch\* b, int j, int modulation, float\* out[^;]*\);", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h) and _lib.ABI_VERSION == 2
    assert len(_lib.EXPORTS["orl_batch_path_features_shape"][1]) == 5 and len(_lib.EXPORTS["orl_batch_path_features"][1]) == 4


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_path_feature_kernels_exist_for_every_row_width_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    lib = _build.build()
    found = {}
    for k in kernel_regs.kernels(lib):
        m = re.match(r"(?:void )?k_path_features<(\d+)>", kernel_regs.demangle(k["name"]))
        if m:
            found[int(m.group(1))] = k
    assert sorted(found) == list(_build.ROW_WIDTHS)
    for w, k in found.items():
        assert int(k["vgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, (w, k)


def test_restatement_equals_the_oracle_observation_bit_for_bit():
    """DeepRMSA, case deep_s129_j4, 64 envs, uniformly random integer actions: at 50, 100, 150 and 200 steps both forms of the
    restatement with j = 4 are oracle.observation(); the states hold full blocks, partial blocks and free rows without a fit."""
    case = slot_agent.CASE_BY_NAME["deep_s129_j4"]
    ora = OracleBackend("DeepRMSA", TOPOLOGY, list(range(100, 164)), **case.kw)
    rng = np.random.default_rng(0)
    full = partial = nofit = nofit_150 = 0
    for point in (50, 100, 150, 200):
        pf.walk(ora, rng, 50)
        env_type, avail, services = pf.state_of(ora)
        obs = ora.observation()
        slow = pf.restate(env_type, avail, services, ora.topology, 4)
        assert slow.shape == obs.shape == (64, 1 + 2 * 14 + K * 11)
        assert np.array_equal(_bits(slow), _bits(obs)), point
        assert np.array_equal(_bits(pf.restate_fast(env_type, avail, services, ora.topology, 4)), _bits(obs)), point
        exists, listed, free = pf.block_counts(slow, services, ora.topology, K, 4)
        full += int((exists & (listed == 4)).sum())
        partial += int((exists & (listed >= 1) & (listed <= 3)).sum())
        nofit += int((exists & free & (listed == 0)).sum())
        if point == 150:
            nofit_150 = nofit
    print("rows with 4 blocks %d, with 1 to 3 %d, free without a fit %d (%d by step 150)" % (full, partial, nofit, nofit_150))
    assert full >= 10 and partial >= 100 and nofit_150 >= 10


def _rmcsa_oracle(C, S, n, steps):
    kw = dict(load=40, num_spectrum_resources=S, num_spatial_resources=C, worst_xt=-84.7, allow_rejection=True, mean_service_holding_time=10.0,
              episode_length=1000)
    topo, tab = slot_agent.topology(), slot_agent.rmcsa_tables("rmcsa_c7_s64")  # (the tables depend on worst_xt and the rates, not on C or S)
    ora = OracleBackend("RMCSA", TOPOLOGY, list(range(70, 70 + n)), **kw)
    for t in range(steps):
        _t, avail, services = pf.state_of(ora)
        ora.step(slot_agent.rmcsa_agent_actions(avail, services, topo, tab, t, np.random.RandomState(t), S, C)[0], auto_reset=True)
    return ora, tab


@pytest.mark.parametrize("j", [1, 4, 8])
def test_slow_and_fast_restatement_agree(j):
    for fam, kw in (("RMSA", pf.RMSA_S64_KW), ("RMSA", slot_agent.CASE_BY_NAME["rmsa_s65"].kw), ("RWA", pf.RWA_S16_KW)):
        ora = OracleBackend(fam, TOPOLOGY, list(range(20, 36)), **kw)
        rng = np.random.default_rng(j)
        for _ in range(3):
            pf.walk(ora, rng, 40)
            env_type, avail, services = pf.state_of(ora)
            slow = pf.restate(env_type, avail, services, ora.topology, j)
            assert slow.shape == (16, 1 + 28 + K * (2 * j + 3))
            assert np.array_equal(_bits(slow), _bits(pf.restate_fast(env_type, avail, services, ora.topology, j))), fam
            assert np.array_equal(slow[:, 0], np.zeros(16) if fam == "RWA" else services[:, 4] / 100)
            assert (slow[:, 1:29].sum(axis=1) == 2).all()
    C, S = 3, 40
    ora, tab = _rmcsa_oracle(C, S, 12, 60)
    env_type, avail, services = pf.state_of(ora)
    rows = {}
    for mod in (-1, 0, M - 1):
        slow = pf.restate(env_type, avail, services, ora.topology, j, tab, mod)
        assert slow.shape == (12, 1 + 28 + K * C * (2 * j + 3))
        assert np.array_equal(_bits(slow), _bits(pf.restate_fast(env_type, avail, services, ora.topology, j, tab, mod))), mod
        rows[mod] = slow
    assert not np.array_equal(rows[0], rows[M - 1])  # (the slots needed differ between the modulations)
    blk = rows[-1][:, 29:].reshape(12, K, C, 2 * j + 3)
    assert (blk[:, :, 0] != blk[:, :, 1]).any()  # two cores of one path differ somewhere


def test_the_gpu_walks_hold_full_rows_on_the_oracle():
    """What tests/test_path_features_gpu.py relies on: RMSA with S = 64 holds at least 4 path rows without a free slot at every
    checkpoint, RWA with S = 16 over 100 of its 320 rows after 120 steps."""
    for fam, kw, S, need in (("RMSA", pf.RMSA_S64_KW, 64, {60: 4, 120: 4, 180: 4}), ("RWA", pf.RWA_S16_KW, 16, {120: 101})):
        ora = OracleBackend(fam, TOPOLOGY, pf.walk_seeds(S), **kw)
        rng = np.random.default_rng(S)
        for point in pf.WALK_POINTS:
            pf.walk(ora, rng, 60)
            env_type, avail, services = pf.state_of(ora)
            exists, _listed, free = pf.block_counts(pf.restate_fast(env_type, avail, services, ora.topology, 1), services, ora.topology, K, 1)
            busy = int((exists & ~free).sum())
            print("%s S = %d after %d steps: %d of %d rows without a free slot" % (fam, S, point, busy, exists.size))
            assert busy >= need.get(point, 0), (fam, point)


class FeatureOracle(OracleBackend):
    """The oracle stand-in with a `path_features` of its own: the numpy restatement on its read-back state."""

    def path_features_shape(self, j=1):
        dim, R = pf.shape_of(self.ENV_TYPE, self.topology, self.C, j)
        return dim, R, (dim + 3) // 4 * 4

    def path_features(self, j=1, modulation=None, fetch=True, out=None):
        rows = np.float32(pf.of_batch(self, j, modulation, fast=False))
        if out is None:
            return rows
        out[...] = rows
        return out


@pytest.mark.parametrize("fam,kw,j", [("RMSA", pf.RMSA_S64_KW, 1), ("RMSA", pf.RMSA_S64_KW, 3), ("DeepRMSA", dict(pf.RMSA_S64_KW, j=2), 4),
                                      ("RWA", pf.RWA_S16_KW, 2)])
def test_vecenv_hands_out_the_path_features(fam, kw, j):
    batch = FeatureOracle(fam, TOPOLOGY, list(range(30, 38)), **dict(kw, episode_length=10))
    venv = OpticalVecEnv(batch, observation="path_features", path_features_j=j)
    dim = 1 + 28 + K * (2 * j + 3)
    sp = venv.observation_space
    assert sp.shape == (dim,) and sp.dtype == np.float32 and float(np.min(sp.low)) == -2.0 ** 30 and float(np.max(sp.high)) == 2.0 ** 30
    obs = venv.reset()
    assert obs.shape == (8, dim) and obs.dtype == np.float32
    assert np.array_equal(obs.view(np.uint32), np.float32(pf.of_batch(batch, j)).view(np.uint32))
    rng = np.random.default_rng(1)
    finished = 0
    for _ in range(24):
        held = obs
        before = held.copy()
        obs, _reward, done, infos = venv.step(pf.random_actions(batch, rng))
        assert obs.shape == (8, dim) and obs.dtype == np.float32 and np.abs(obs).max() <= 2.0 ** 30
        assert np.array_equal(obs.view(np.uint32), np.float32(pf.of_batch(batch, j)).view(np.uint32))
        assert np.array_equal(held, before)  # the rows a step handed out stay as they were over the next step
        for i in np.flatnonzero(done):  # the soft reset keeps the pending service and the maps: the terminal observation is the row
            assert np.array_equal(infos[i]["terminal_observation"], obs[i])
            finished += 1
    assert finished >= 8
