"""MatrixObservationWithPaths of QoSConstrainedRA (include/orl.h, orl_batch_matrix_paths_observation) without a GPU: the ABI
surface, the kernel in the code object, the numpy restatement the GPU tests compare with (against the observations captured
from the reference's own wrapper, tests/golden/m1_qos_matrix_paths.npz) and OpticalVecEnv's "matrix_paths" mode over the CPU
oracle."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

from optical_rl_gym_amd import _lib
from optical_rl_gym_amd.topology import Topology
from optical_rl_gym_amd.vec_env import OpticalVecEnv
from tests.helpers import load_golden
from tests.oracle_backend import OracleBackend
from tests.qos_obs_restate import restate, restate_fast, spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "m1_qos_matrix_paths"
QOS_KW = dict(load=1000, mean_service_holding_time=25, episode_length=10, num_spectrum_resources=12, num_service_classes=3,
              classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0], allow_rejection=True)


class QoSObsOracle(OracleBackend):
    """The oracle stand-in with a MatrixObservationWithPaths of its own: the numpy restatement on its read-back state."""

    def matrix_paths_obs_shape(self):
        dim = self.topology.n_links * self.S * (self.k + 1) + 1
        return dim, (dim + 15) // 16 * 16

    def matrix_observation_with_paths(self, fetch=True, out=None):
        spectrum = np.stack([self.spectrum(i) for i in range(self.n)])
        rows = restate_fast(spectrum, self.services()[:, 2:5].astype(np.int64), self.topology, self.S, self.k)
        if out is None:
            return rows
        out[...] = rows
        return out


def fixture_rows(g, stream):
    """uint8 [T + 1, dim] observations of a stream of the fixture, unpacked."""
    dim = g["meta"]["dim"]
    bits = np.unpackbits(g[stream + "_obs_bits"], axis=1)[:, :dim - 1]
    return np.concatenate([bits, g[stream + "_obs_class"][:, None]], axis=1)


def test_header_and_binding_declare_the_matrix_paths_api():
    h = open(os.path.join(ROOT, "include", "orl.h")).read()
    assert re.search(r"int orl_batch_matrix_paths_obs_shape\(const orl_batch\* b, int32_t\* dim, int32_t\* pitch\);", h)
    assert re.search(r"int orl_batch_matrix_paths_observation\(orl_batch\* b, uint8_t\* out\);", h)
    assert re.search(r"#define ORL_BUF_MATRIX_PATHS_OBS 8\b", h)
    assert re.search(r"#define ORL_ABI_VERSION 2\b", h)
    assert len(_lib.EXPORTS["orl_batch_matrix_paths_obs_shape"][1]) == 3
    assert len(_lib.EXPORTS["orl_batch_matrix_paths_observation"][1]) == 2


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_kernel_is_in_the_library_without_spills_or_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    from optical_rl_gym_amd import _build

    lib = _build.build()
    found = [k for k in kernel_regs.kernels(lib) if kernel_regs.demangle(k["name"]).startswith(("k_qos_matrix_obs", "void k_qos_matrix_obs"))]
    assert len(found) == 1
    k = found[0]
    assert int(k["vgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) == 0, k
    for name in ("orl_batch_matrix_paths_obs_shape", "orl_batch_matrix_paths_observation"):
        assert hasattr(_lib.lib(), name)


@pytest.mark.parametrize("stream", ["sapff", "random"])
def test_restatement_reproduces_the_reference_wrapper(stream):
    g = load_golden(FIXTURE)
    meta = g["meta"]
    topo = Topology.load(meta["topology"])
    S, k = meta["kwargs"]["num_spectrum_resources"], meta["k_paths"]
    assert k == topo.k_paths and meta["dim"] == topo.n_links * S * (k + 1) + 1
    want = fixture_rows(g, stream)
    spectrum, pending = g[stream + "_spectrum"], g[stream + "_pending"]
    assert np.array_equal(restate(spectrum, pending, topo, S, k), want)
    assert np.array_equal(restate_fast(spectrum, pending, topo, S, k), want)
    # the fixture exercises the spill column and class-0 services (only the shortest path)
    sp = spills(spectrum, pending, topo, k)
    assert sp.sum() == meta["streams"][stream]["n_spill"] > 0
    assert (pending[:, 2] == 0).sum() == meta["streams"][stream]["n_class0"] > 0
    assert (pending[:, 2] >= 2).any() and len(want) == meta["n_steps"] + 1


def test_vecenv_matrix_paths_mode():
    batch = QoSObsOracle("QoSConstrainedRA", "nsfnet_chen", list(range(40, 48)), **QOS_KW)
    venv = OpticalVecEnv(batch, observation="matrix_paths")
    dim = 22 * 12 * 6 + 1
    sp = venv.observation_space
    assert tuple(sp.shape) == (dim,) and np.dtype(sp.dtype) == np.uint8
    assert np.all(np.asarray(sp.low) == 0) and np.all(np.asarray(sp.high) == 1)
    obs = venv.reset()
    assert obs.shape == (8, dim) and obs.dtype == np.uint8
    assert np.array_equal(obs, batch.matrix_observation_with_paths())
    seen, finished = [obs], 0
    rng = np.random.default_rng(5)
    for t in range(25):
        obs, rew, done, infos = venv.step(rng.integers(0, 6, size=8))
        assert obs.shape == (8, dim) and obs.dtype == np.uint8 and rew.shape == (8,) and done.shape == (8,)
        assert np.array_equal(obs, batch.matrix_observation_with_paths())
        for i in np.flatnonzero(done):
            # the in-kernel reset is soft (reset(only_counters=True)): the observation does not change
            assert np.array_equal(infos[i]["terminal_observation"], obs[i])
            finished += 1
        seen.append(obs)
    assert finished >= 8
    # host rows go into a ring of three reused arrays
    assert seen[-1] is seen[-4] and seen[-1] is not seen[-2] and seen[-1] is not seen[-3]
    assert (obs[:, -1] == batch.services()[:, 4]).all()


def test_vecenv_matrix_paths_mode_is_qos_only():
    batch = OracleBackend("RMSA", "nsfnet_chen", [1, 2], load=10, num_spectrum_resources=16)
    with pytest.raises(ValueError, match="QoSConstrainedRA"):
        OpticalVecEnv(batch, observation="matrix_paths")
