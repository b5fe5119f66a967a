"""MatrixObservationWithPaths on the device (include/orl.h, orl_batch_matrix_paths_observation; k_qos_matrix_obs in
csrc/orl_qos_obs.h): bit for bit against the observations captured from the reference's wrapper, against the numpy restatement
(tests/qos_obs_restate.py) on every env after the states both QoS step kernels leave behind, zero-copy, under graph capture,
across devices and through OpticalVecEnv."""
import os

import numpy as np
import pytest

from tests.helpers import load_golden
from tests.qos_obs_restate import restate, restate_fast, spills
from tests.test_gpu_parity import _need_devices, _product, _qos_step_kernel_is, qos_impl  # noqa: F401  (qos_impl: a fixture)
from tests.test_qos_matrix_obs import FIXTURE, fixture_rows

pytestmark = pytest.mark.gpu

# high load: links without a free unit, hence spill columns, are common
HOT = dict(load=1000, mean_service_holding_time=25, episode_length=60, num_spectrum_resources=24, num_service_classes=3,
           classes_arrival_probabilities=[0.3, 0.4, 0.3], classes_reward=[4.0, 2.0, 1.0], allow_rejection=True)
# tools/qos_step_rate.py's configuration (B of tools/qos_obs_rate.py)
CFG_B = dict(load=300, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64, num_service_classes=3,
             classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[4.0, 2.0, 1.0], allow_rejection=True)


def _make(n, kw=HOT, seed0=100, topology="nsfnet_chen", fam="QoSConstrainedRA", **extra):
    import optical_rl_gym_amd as orl

    return orl.make(fam, topology=topology, num_envs=n, seeds=list(range(seed0, seed0 + n)), **kw, **extra)


def _state(env, envs=None):
    idx = range(env.num_envs) if envs is None else envs
    spectrum = np.stack([env.spectrum(int(e)) for e in idx])
    pending = env.services()[:, 2:5].astype(np.int64)
    return spectrum, (pending if envs is None else pending[np.asarray(envs)])


def _expected(env, envs=None, fast=True):
    spectrum, pending = _state(env, envs)
    fn = restate_fast if fast else restate
    return fn(spectrum, pending, env.topology, env.num_spectrum_resources, env.k_paths)


def _check(env, what):
    got = env.matrix_observation_with_paths()
    dim, _pitch = env.matrix_paths_obs_shape()
    assert got.shape == (env.num_envs, dim) and got.dtype == np.uint8, what
    want = _expected(env)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, "%s: %d envs differ, first %d" % (what, len(bad), bad[0])
    return got


@pytest.mark.parametrize("stream", ["sapff", "random"])
def test_replays_the_reference_wrapper_bit_for_bit(stream, qos_impl):  # noqa: F811
    g = load_golden(FIXTURE)
    meta = g["meta"]
    env = _product(meta)
    assert _qos_step_kernel_is(env, qos_impl)
    want = fixture_rows(g, stream)
    assert env.matrix_paths_obs_shape()[0] == meta["dim"]
    acts, reset_before = g[stream + "_actions"], g[stream + "_reset_before"]
    for t in range(meta["n_steps"] + 1):
        if t < meta["n_steps"] and reset_before[t]:
            env.reset(full=False)
        assert np.array_equal(env.spectrum(0), g[stream + "_spectrum"][t]), t
        assert np.array_equal(env.services()[0, 2:5].astype(np.int64), g[stream + "_pending"][t]), t
        got = env.matrix_observation_with_paths()
        assert np.array_equal(got[0], want[t]), "step %d: %d columns differ" % (t, int((got[0] != want[t]).sum()))
        if t < meta["n_steps"]:
            env.step(np.array([[acts[t]]]))
    assert not env.flags().any()
    env.close()


def test_every_env_after_run_and_random_steps(qos_impl):  # noqa: F811
    n = 4096
    env = _make(n)
    assert _qos_step_kernel_is(env, qos_impl)
    env.run("SAP_FF", 300)
    _check(env, "after run(SAP_FF, 300)")
    assert spills(*_state(env), env.topology, env.k_paths).any()
    rng = np.random.default_rng(11)
    for t in range(50):
        env.step(rng.integers(0, env.k_paths + 1, size=(n, 1)), auto_reset=True)
    got = _check(env, "after 50 random steps")
    spectrum, pending = _state(env)
    assert spills(spectrum, pending, env.topology, env.k_paths).sum() > 10 and (pending[:, 2] == 0).any()
    assert (got[:, -1] == pending[:, 2]).all()
    env.close()


def test_pairs_with_fewer_paths(golden_dir):
    """tests/golden/tiny5_k3.npz: every pair has one or two of k = 3 paths.  The blocks of the paths >= n_paths are 0 but for
    the spill column of the block right behind the last allowed path."""
    env = _make(512, dict(HOT, num_spectrum_resources=16, load=300), topology=os.path.join(golden_dir, "tiny5_k3.npz"))
    env.run("SAP_FF", 200)
    got = _check(env, "tiny5_k3")
    assert np.array_equal(got, _expected(env, fast=False))
    spectrum, pending = _state(env)
    k, S, E = env.k_paths, env.num_spectrum_resources, env.topology.n_links
    assert k == 3
    n_paths = env.topology.n_paths[pending[:, 0], pending[:, 1]]
    allowed = np.where(pending[:, 2] == 0, np.minimum(n_paths, 1), n_paths)
    assert (n_paths == 1).any() and (n_paths == 2).any()
    blocks = got[:, :-1].reshape(env.num_envs, E, k + 1, S)
    for i in range(env.num_envs):
        assert not blocks[i, :, allowed[i] + 1:, 1:].any() and not blocks[i, :, allowed[i] + 2:, :].any(), i
    assert spills(spectrum, pending, env.topology, k).any()
    env.close()


def test_full_size_batch(monkeypatch):
    monkeypatch.delenv("ORL_AGENT_STEP", raising=False)  # the library's own kernel choice
    n = 65536
    env = _make(n, CFG_B, seed0=1)
    env.run("SAP_FF", 300)
    got = env.matrix_observation_with_paths()
    dim, pitch = env.matrix_paths_obs_shape()
    assert got.shape == (n, dim) and dim == 22 * 64 * 6 + 1 and pitch == (dim + 15) // 16 * 16
    sample = np.random.default_rng(0).choice(n, 1024, replace=False)
    sample.sort()
    assert np.array_equal(got[sample], _expected(env, sample))
    assert (got[:, -1] == env.services()[:, 4]).all()
    env.close()


def test_fetch_false_and_the_device_view():
    import torch

    from optical_rl_gym_amd._lib import OrlError

    n = 2048
    env = _make(n)
    with pytest.raises(OrlError, match="no MatrixObservationWithPaths yet"):
        env.device_tensor("matrix_paths_obs")
    env.run("SAP_FF", 100)
    rng = np.random.default_rng(3)
    acts = env.device_tensor("actions")
    a = rng.integers(0, env.k_paths + 1, size=n)
    with torch.cuda.stream(env.torch_stream()):
        acts[:, 0].copy_(torch.as_tensor(a, dtype=torch.int32, device=acts.device))
        env.step(None, auto_reset=True, fetch=False)
        assert env.matrix_observation_with_paths(fetch=False) is None  # queued behind the step: no synchronisation in between
    env.sync()
    view = env.device_tensor("matrix_paths_obs")
    dim, pitch = env.matrix_paths_obs_shape()
    assert view.shape == (n, dim) and view.dtype == torch.uint8 and view.stride() == (pitch, 1)
    lazy = view.cpu().numpy().copy()
    assert np.array_equal(lazy, env.matrix_observation_with_paths())
    assert np.array_equal(lazy, _expected(env))
    out = env.host_array((n, dim), np.uint8)
    assert env.matrix_observation_with_paths(out=out) is out and np.array_equal(out, lazy)
    env.close()


def test_graph_capture_equals_the_eager_loop():
    """{actions from a torch tensor, step, observation, copy out} captured in a torch.cuda graph on the batch's stream and
    replayed equals the eager loop on a second batch with the same seeds."""
    import torch

    N, T = 2048, 16
    envs = [_make(N, dict(HOT, num_spectrum_resources=16), seed0=9) for _ in range(2)]
    for e in envs:
        e.run("SAP_FF", 200)
    e0 = envs[0]
    dev = "cuda:%d" % e0.device_id
    dim = e0.matrix_paths_obs_shape()[0]
    actions = torch.randint(0, e0.k_paths + 1, (T, N), device=dev, dtype=torch.int32)  # drawn once, outside the capture
    out = [dict(obs=torch.zeros((T, N, dim), dtype=torch.uint8, device=dev), rew=torch.zeros((T, N), dtype=torch.float64, device=dev))
           for _ in envs]
    for e in envs:
        e.matrix_observation_with_paths(fetch=False)  # (the first call allocates the buffer: outside the capture)
    torch.cuda.synchronize()

    def loop(i):
        e = envs[i]
        view, acts, rew = e.device_tensor("matrix_paths_obs"), e.device_tensor("actions"), e.device_tensor("reward")
        for t in range(T):
            acts[:, 0].copy_(actions[t])
            e.step(None, auto_reset=True, fetch=False)
            e.matrix_observation_with_paths(fetch=False)
            out[i]["obs"][t].copy_(view)
            out[i]["rew"][t].copy_(rew)

    s0, s1 = e0.torch_stream(), envs[1].torch_stream()
    s0.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s0):
        loop(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s1):  # (capturing runs nothing: envs[1] is still in the start state)
        loop(1)
    g.replay()
    torch.cuda.synchronize()
    for k in ("obs", "rew"):
        assert torch.equal(out[0][k], out[1][k]), k
    last = envs[1].matrix_observation_with_paths()
    assert np.array_equal(out[1]["obs"][-1].cpu().numpy(), last) and np.array_equal(last, _expected(envs[1]))
    assert np.array_equal(e0.counters(), envs[1].counters())
    for e in envs:
        e.check()
        e.close()


@pytest.mark.parametrize("devs", [pytest.param((0,), id="one_gpu"), pytest.param((0, 1), id="two_gpus")])
def test_multi_device_batch_equals_the_shards(devs):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    _need_devices(devs)
    n = 4096
    if len(devs) == 1:
        m = MultiDeviceBatch.from_shards([_make(n, seed0=3)])
    else:
        m = orl.make("QoSConstrainedRA", topology="nsfnet_chen", num_envs=n, seeds=list(range(3, 3 + n)), device_ids=list(devs), **HOT)
    rng = np.random.default_rng(4)
    for _ in range(30):
        m.step(rng.integers(0, 6, size=(n, 1)), auto_reset=True)
    whole = m.matrix_observation_with_paths()
    parts = [s.matrix_observation_with_paths() for s in m.shards]
    assert np.array_equal(whole, np.concatenate(parts))
    for s, part in zip(m.shards, parts):
        assert np.array_equal(part, _expected(s))
    into = np.zeros_like(whole)
    assert m.matrix_observation_with_paths(out=into) is into and np.array_equal(into, whole)
    m.close()


def test_vecenv_matrix_paths_mode_on_the_device():
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    n = 1024
    env = _make(n, dict(HOT, episode_length=8))
    venv = OpticalVecEnv(env, observation="matrix_paths")
    dim = env.matrix_paths_obs_shape()[0]
    assert tuple(venv.observation_space.shape) == (dim,)
    obs = venv.reset()
    assert obs.shape == (n, dim) and np.array_equal(obs, _expected(env))
    rng = np.random.default_rng(6)
    finished = 0
    for _ in range(10):
        obs, rew, done, infos = venv.step(rng.integers(0, 6, size=n))
        assert np.array_equal(obs, _expected(env))
        for i in np.flatnonzero(done)[:50]:
            assert np.array_equal(infos[i]["terminal_observation"], obs[i])
        finished += int(done.sum())
    assert finished >= n
    t = venv.device_tensors()
    assert "matrix_paths_obs" in t and np.array_equal(t["matrix_paths_obs"].cpu().numpy(), obs)
    venv.close()


@pytest.mark.parametrize("fam,kw", [("RMSA", dict(load=100, num_spectrum_resources=64)), ("RWA", dict(load=60, num_spectrum_resources=16)),
                                    ("RMCSA", dict(load=100, num_spectrum_resources=64, num_spatial_resources=7))])
def test_other_families_have_no_matrix_paths_observation(fam, kw):
    from optical_rl_gym_amd._lib import OrlError
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    env = _make(64, kw, fam=fam)
    for call in (env.matrix_paths_obs_shape, env.matrix_observation_with_paths,
                 lambda: env.matrix_observation_with_paths(fetch=False)):
        with pytest.raises(OrlError, match="QoSConstrainedRA only"):
            call()
    with pytest.raises(OrlError):
        env.device_tensor("matrix_paths_obs")
    with pytest.raises(ValueError):
        OpticalVecEnv(env, observation="matrix_paths")
    env.close()
