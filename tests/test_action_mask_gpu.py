"""Action masks on the device (include/orl.h, orl_batch_action_mask; k_action_mask in csrc/orl_mask.h) against the numpy
restatement of the reference's definitions (tests/mask_restate.py) on every env, against the step itself (a column is 1 exactly
when stepping it provisions the service), after the states every step implementation leaves behind, zero-copy and under graph
capture."""
import numpy as np
import pytest

from tests.mask_restate import restate, restate_fast, row_words, unpack_slots
from tests.test_gpu_parity import IMPLS, _need_devices, force_impl

pytestmark = pytest.mark.gpu

CFG2 = dict(load=300, mean_service_holding_time=25, episode_length=1000, num_spectrum_resources=320, allow_rejection=False)
CFG3 = dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=1, episode_length=50)
CFG1 = dict(load=450, mean_service_holding_time=25, episode_length=1000, allow_rejection=True)
# (family, kwargs, heuristic of the device loop)
CONFIGS = {
    "rmsa_s64": ("RMSA", dict(load=100, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64), "SAP_FF"),
    "rmsa_s320": ("RMSA", CFG2, "SAP_FF"),
    "deeprmsa_j1": ("DeepRMSA", CFG3, "SAP"),
    "deeprmsa_j3": ("DeepRMSA", dict(CFG3, j=3, allow_rejection=True), "SAP"),
    "rwa": ("RWA", CFG1, "SAP_FF"),
}


def _make(fam, kw, n, seed0=1000, topology="nsfnet_chen", **extra):
    import optical_rl_gym_amd as orl

    return orl.make(fam, topology=topology, num_envs=n, seeds=list(range(seed0, seed0 + n)), **kw, **extra)


def _layouts(env):
    return ("joint",) if env.ENV_TYPE == 1 else ("joint", "path")


def _expected(env, layout, fast=True, chunk=8192):
    """The restatement from the batch's read-back state (slots_packed, services, topology)."""
    fam_t = env.ENV_TYPE
    cw = 50.0 if fam_t == 2 else 12.5
    packed, svc = env.slots_packed(), env.services()
    fn = restate_fast if fast else restate
    parts = []
    for lo in range(0, env.num_envs, chunk):
        avail = unpack_slots(packed[lo:lo + chunk], env.topology.n_links, env.num_spectrum_resources, row_words(env.num_spectrum_resources))
        parts.append(fn(fam_t, avail, svc[lo:lo + chunk], env.topology, env.k_paths, env.num_spectrum_resources, env.j, cw,
                        env.allow_rejection, layout))
    return np.concatenate(parts)


def _check(env, what):
    for lay in _layouts(env):
        got = env.action_mask(lay)
        want = _expected(env, lay)
        assert got.shape == want.shape and got.dtype == np.bool_, (what, lay)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "%s, %s layout: %d envs differ, first %d" % (what, lay, len(bad), bad[0])


def _random_actions(env, rng):
    n = env.num_envs
    if env.ENV_TYPE == 1:
        return rng.integers(0, env.k_paths * env.j + 1, size=(n, 1))
    a = env.policy("SAP_FF")[:, :2].copy()
    pick = rng.random(n) < 0.3
    a[pick, 0] = rng.integers(0, env.k_paths, size=pick.sum())
    a[pick, 1] = rng.integers(0, env.num_spectrum_resources, size=pick.sum())
    return a


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_mask_equals_restatement_after_reset_and_host_steps(name):
    fam, kw, _pol = CONFIGS[name]
    env = _make(fam, kw, 2048)
    _check(env, "after construction")
    rng = np.random.default_rng(5)
    for _ in range(40):
        env.step(_random_actions(env, rng), auto_reset=True)
    _check(env, "after host-driven random steps")
    env.reset(full=True)
    _check(env, "after a full reset")
    env.close()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_mask_equals_restatement_after_run_under_every_impl(name, monkeypatch):
    fam, kw, pol = CONFIGS[name]
    for impl in IMPLS:
        force_impl(monkeypatch, impl)
        env = _make(fam, kw, 2048)
        env.run(pol, 300)
        _check(env, "after run(%s, 300) [%s]" % (pol, impl))
        env.close()


def _column_action(env, c, dim):
    if env.ENV_TYPE == 1:
        return np.full((env.num_envs, 1), c)
    S = env.num_spectrum_resources
    return np.tile([c // S, c % S], (env.num_envs, 1))


@pytest.mark.parametrize("name", ["rmsa_s64", "deeprmsa_j3", "rwa", "rmsa_s320"])
def test_mask_predicts_acceptance_of_every_column(name):
    fam, kw, pol = CONFIGS[name]
    env = _make(fam, kw, 64, seed0=77)
    env.run(pol, 150)
    mask = env.action_mask("joint")
    pmask = env.action_mask("path") if fam != "DeepRMSA" else None
    dim = mask.shape[1]
    snap = env.get_state()
    acc0 = env.counters()[:, 1].copy()  # services_accepted
    svc = env.services()
    n_paths = env.topology.n_paths[svc[:, 2].astype(int), svc[:, 3].astype(int)]
    reject = np.array([[env.k_paths * env.j]] if fam == "DeepRMSA" else [[env.k_paths, env.num_spectrum_resources]])
    accepted = np.zeros((env.num_envs, dim - 1), bool)
    for c in range(dim - 1):
        env.set_state(snap)
        a = _column_action(env, c, dim)
        if fam != "DeepRMSA":
            lacks = (c // env.num_spectrum_resources) >= n_paths  # the reference raises IndexError: step the reject action there
            a[lacks] = reject[0]
        env.step(a)
        accepted[:, c] = env.counters()[:, 1] - acc0 == 1
    fb = ~accepted.any(axis=1)
    assert np.array_equal(mask[~fb, :-1], accepted[~fb]), name
    # fallback rows: nothing provisions; all non-reject columns set unless rejection is allowed
    if env.allow_rejection:
        assert not mask[fb, :-1].any()
    else:
        assert mask[fb, :-1].all()
    assert (mask[:, -1] == env.allow_rejection).all()
    assert fb.sum() < env.num_envs
    if fam == "DeepRMSA":
        env.close()
        return
    # the path layout against what PathOnlyFirstFitAction's first fit (policy "PATH_FF", rmsa_env.py:840-874 / rwa_env.py:505-536)
    # then provisions, path by path
    paccepted = np.zeros((env.num_envs, env.k_paths), bool)
    for p in range(env.k_paths):
        env.set_state(snap)
        env.step(env.policy("PATH_FF", paths=np.full(env.num_envs, p))[:, :2].copy())
        paccepted[:, p] = env.counters()[:, 1] - acc0 == 1
    assert not paccepted[np.arange(env.k_paths)[None, :] >= n_paths[:, None]].any()
    pfb = ~paccepted.any(axis=1)
    assert np.array_equal(pmask[~pfb, :-1], paccepted[~pfb]), name
    assert pmask[pfb, :-1].all() if not env.allow_rejection else not pmask[pfb, :-1].any()
    assert (pmask[:, -1] == env.allow_rejection).all()
    env.close()


def test_pairs_with_fewer_paths_give_zero_columns(golden_dir):
    """A 5-node topology with k = 3 (tests/golden/tiny5_k3.npz: a line with a triangle at one end): every pair has one or two
    paths, so the columns of path 2 — and of path 1 for the one-path pairs — are 0 in every row."""
    import os

    topo = os.path.join(golden_dir, "tiny5_k3.npz")
    kw = dict(load=10, mean_service_holding_time=25, episode_length=50, num_spectrum_resources=64)
    env = _make("RMSA", kw, 256, topology=topo)
    env.run("SAP_FF", 20)
    svc = env.services()
    n_paths = env.topology.n_paths[svc[:, 2].astype(int), svc[:, 3].astype(int)]
    assert (n_paths == 1).any() and (n_paths == 2).any()
    for lay in ("joint", "path"):
        m = env.action_mask(lay)
        assert np.array_equal(m, _expected(env, lay, fast=False)), lay
        w = 64 if lay == "joint" else 1
        assert not m[:, 2 * w:3 * w].any() and not m[n_paths == 1, w:2 * w].any()
        assert m[n_paths == 2, w:2 * w].any() and m[:, :w].any()
    env.close()


@pytest.mark.parametrize("name", ["rmsa_s320", "deeprmsa_j1"])
def test_full_size_batch_equals_restatement(name):
    fam, kw, pol = CONFIGS[name]
    env = _make(fam, kw, 65536, seed0=1)
    env.run(pol, 300)
    _check(env, "65 536 envs after run(%s, 300)" % pol)
    env.close()


def test_fetch_false_and_the_device_view():
    import torch

    fam, kw, pol = CONFIGS["rmsa_s320"]
    env = _make(fam, kw, 2048)
    env.run(pol, 100)
    rng = np.random.default_rng(3)
    a = _random_actions(env, rng)
    acts = env.device_tensor("actions")
    with torch.cuda.stream(env.torch_stream()):
        acts[:, :2].copy_(torch.as_tensor(a, dtype=torch.int32, device=acts.device))
        env.step(None, auto_reset=True, fetch=False)
        env.action_mask(fetch=False)  # queued behind the step: no synchronisation in between
    env.sync()
    view = env.device_tensor("action_mask")
    dim, pitch = env.action_mask_shape("joint")
    assert view.shape == (2048, dim) and view.dtype == torch.bool and view.stride() == (pitch, 1)
    lazy = view.cpu().numpy().copy()
    assert np.array_equal(lazy, env.action_mask("joint"))
    assert np.array_equal(lazy, _expected(env, "joint"))
    # a view belongs to its layout: path-layout launches do not touch the joint rows it shows
    path = env.action_mask("path")
    pview = env.device_tensor("action_mask")
    assert pview.shape == (2048, env.k_paths + 1) and np.array_equal(pview.cpu().numpy(), path)
    assert np.array_equal(view.cpu().numpy(), lazy)
    env.close()


def test_graph_capture_equals_the_eager_loop_and_masked_sampling_is_accepted():
    """{actions, step, mask} captured in a torch.cuda graph on the batch's stream and replayed equals the eager loop bit for bit;
    a uniformly sampled masked agent (uniform over the provisioning columns) gets every action accepted whenever its row had one."""
    import torch

    fam, kw, _pol = CONFIGS["deeprmsa_j3"]
    N, T = 2048, 16
    envs = [_make(fam, kw, N, seed0=9) for _ in range(2)]  # same seeds: the same states
    for e in envs:
        e.run("SAP", 300)  # (steady state: some rows without a provisioning action)
    e0 = envs[0]
    dev = "cuda:%d" % e0.device_id
    n_act = e0.k_paths * e0.j + 1
    reject = e0.k_paths * e0.j
    noise = torch.rand((T, N, n_act - 1), device=dev)  # drawn once, outside the capture
    out = [dict(mask=torch.zeros((T, N, n_act), dtype=torch.bool, device=dev), rew=torch.zeros((T, N), dtype=torch.float64, device=dev),
                had=torch.zeros((T, N), dtype=torch.bool, device=dev)) for _ in envs]

    def loop(i):
        e = envs[i]
        m, acts, rew = e.device_tensor("action_mask"), e.device_tensor("actions"), e.device_tensor("reward")
        for t in range(T):
            cur = m[:, :n_act]
            had = cur[:, :-1].any(dim=1)  # (allow_rejection=True: no fallback rows)
            a = torch.where(cur[:, :-1], noise[t], torch.full_like(noise[t], -1.0)).argmax(dim=1)
            acts[:, 0] = torch.where(had, a, torch.full_like(a, reject)).int()
            out[i]["mask"][t].copy_(cur)
            out[i]["had"][t].copy_(had)
            e.step(None, auto_reset=True, fetch=False)
            out[i]["rew"][t].copy_(rew)
            e.action_mask(fetch=False)

    for e in envs:
        e.action_mask(fetch=False)  # (the first call allocates the buffer: outside the capture)
    torch.cuda.synchronize()
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
    for k in ("mask", "rew", "had"):
        assert torch.equal(out[0][k], out[1][k]), k
    assert np.array_equal(e0.action_mask("joint"), envs[1].action_mask("joint"))
    assert np.array_equal(e0.counters(), envs[1].counters())
    had, rew = out[0]["had"].cpu().numpy(), out[0]["rew"].cpu().numpy()
    assert had.mean() > 0.2 and (~had).any()
    assert (rew[had] == 1.0).all() and (rew[~had] == -1.0).all()  # deeprmsa_env.py:123-124: +1 accepted, -1 blocked
    for e in envs:
        e.check()
        e.close()


@pytest.mark.parametrize("devs", [pytest.param((0,), id="one_gpu"), pytest.param((0, 1), id="two_gpus")])
def test_multi_device_batch_masks_equal_the_shards(devs):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    _need_devices(devs)
    fam, kw, pol = CONFIGS["rmsa_s64"]
    n = 4096
    if len(devs) == 1:
        m = MultiDeviceBatch.from_shards([_make(fam, kw, n, seed0=3)])
    else:
        m = orl.make(fam, topology="nsfnet_chen", num_envs=n, seeds=list(range(3, 3 + n)), device_ids=list(devs), **kw)
    rng = np.random.default_rng(4)
    for _ in range(30):
        m.step(np.concatenate([_random_actions(s, rng) for s in m.shards]), auto_reset=True)
    for lay in ("joint", "path"):
        whole = m.action_mask(lay)
        parts = [s.action_mask(lay) for s in m.shards]
        assert np.array_equal(whole, np.concatenate(parts))
        for s, part in zip(m.shards, parts):
            assert np.array_equal(part, _expected(s, lay))
    m.close()


@pytest.mark.parametrize("fam,kw", [("RMCSA", dict(load=100, num_spectrum_resources=64, num_spatial_resources=7)),
                                    ("QoSConstrainedRA", dict(load=10))])
def test_rmcsa_and_qos_have_no_masks(fam, kw):
    from optical_rl_gym_amd._lib import OrlError

    env = _make(fam, kw, 64)
    for lay in ("joint", "path"):
        with pytest.raises(OrlError, match="not available"):
            env.action_mask(lay)
        with pytest.raises(OrlError):
            env.action_mask(lay, fetch=False)
    env.close()


def test_maskable_ppo_smoke():
    sb3_contrib = pytest.importorskip("sb3_contrib")
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    fam, kw, _pol = CONFIGS["deeprmsa_j1"]
    venv = OpticalVecEnv(_make(fam, kw, 64), obs_dtype=np.float32)
    model = sb3_contrib.MaskablePPO("MlpPolicy", venv, n_steps=16, batch_size=256, n_epochs=1, device="cpu", seed=0)
    model.learn(total_timesteps=64 * 32)
    masks = np.stack(venv.env_method("action_masks"))
    assert masks.shape == (64, venv.action_space.n)
    venv.close()
