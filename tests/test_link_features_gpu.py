"""The per-link feature observation on the device (include/orl.h, orl_batch_link_features; k_link_features in
csrc/orl_link_obs.h) against the numpy restatement of the reference's definitions (tests/link_features_restate.py) on every env,
bit for bit as np.float32 of the float64 rows; after every way of stepping; zero-copy, under graph capture, over a sharded batch;
and the calls it refuses."""
import numpy as np
import pytest

from tests import link_features_restate as lf
from tests import path_features_restate as pf
from tests import rmcsa_mask_restate as rr
from tests import slot_agent

pytestmark = pytest.mark.gpu

TOPOLOGY = slot_agent.TOPOLOGY
K, N, E = 5, 14, 22


def _make(fam, kw, n, seeds=None, **extra):
    import optical_rl_gym_amd as orl

    return orl.make(fam, topology=TOPOLOGY, num_envs=n, seeds=list(range(n)) if seeds is None else seeds, **dict(kw, **extra))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(env, what, seen=None):
    """link_features() of every env against np.float32 of the restatement; returns the float32 rows."""
    env_type, avail, services = pf.state_of(env)
    lstat = env.link_stats_all()
    want = np.float32(lf.restate_fast(env_type, avail, services, env.topology, lstat))
    got = env.link_features()
    C = avail.shape[1]
    dim, rows, width, pitch = env.link_features_shape()
    assert (dim, rows, width) == lf.shape_of(env.topology, C) == (1 + 2 * N + C * E * (10 + K), C * E, 10 + K) and pitch == (dim + 3) // 4 * 4
    assert got.shape == want.shape == (env.num_envs, dim) and got.dtype == np.float32, what
    bad = np.flatnonzero((_u32(got) != _u32(want)).any(axis=1))
    if len(bad):
        col = np.flatnonzero(_u32(got[bad[0]]) != _u32(want[bad[0]]))[0]
        r, i = divmod(int(col) - 1 - 2 * N, 10 + K)
        pytest.fail("%s: %d envs differ, first env %d at column %d (block %d value %d): %r, restatement %r"
                    % (what, len(bad), bad[0], col, r, i, got[bad[0], col], want[bad[0], col]))
    stats = np.transpose(np.float32(lstat[:, 0:3, :]), (0, 2, 1))[:, None].repeat(C, axis=1)
    assert np.array_equal(_u32(lf.blocks_of(got, env.topology, C)[..., 7:10]), _u32(stats)), what
    if seen is not None:
        seen.add(avail)
    return got


def _holds(name, seen):
    print(name, vars(seen))
    for what in lf.WALK_HOLDS.get(name, ()):
        assert getattr(seen, what) >= 1, (name, what)


@pytest.mark.parametrize("name", ["rmsa_s64", "rmsa_s65", "rmsa_s129", "rmsa_s512"])
def test_rmsa_rows_equal_the_restatement(name):
    kw, S = (pf.RMSA_S64_KW, 64) if name == "rmsa_s64" else (slot_agent.CASE_BY_NAME[name].kw, slot_agent.CASE_BY_NAME[name].S)
    env = _make("RMSA", kw, pf.WALK_ENVS, seeds=pf.walk_seeds(S))
    assert env.lib.orl_batch_row_words(env._h) == {64: 1, 65: 2, 129: 5, 512: 8}[S]
    _check(env, "%s after the reset" % name)  # every row free, every average 0
    rng, seen = np.random.default_rng(S), lf.Seen()
    for point in pf.WALK_POINTS:
        pf.walk(env, rng, 60)
        _check(env, "%s after %d steps" % (name, point), seen)
    _holds(name, seen)
    env.check()
    env.close()


def test_deeprmsa_rows_equal_the_restatement():
    case = slot_agent.CASE_BY_NAME["deep_s129_j4"]
    env = _make("DeepRMSA", case.kw, 64, seeds=list(range(100, 164)))
    rng = np.random.default_rng(0)
    for point in (50, 100, 150):
        pf.walk(env, rng, 50)
        _check(env, "deep_s129_j4 after %d steps" % point)
    env.check()
    env.close()


@pytest.mark.parametrize("name", ["rwa_s16", "rwa_s65"])
def test_rwa_rows_equal_the_restatement(name):
    kw, S = (pf.RWA_S16_KW, 16) if name == "rwa_s16" else (slot_agent.CASE_BY_NAME[name].kw, 65)
    env = _make("RWA", kw, pf.WALK_ENVS, seeds=pf.walk_seeds(S))
    rng, seen = np.random.default_rng(S), lf.Seen()
    for point in pf.WALK_POINTS:
        pf.walk(env, rng, 60)
        got = _check(env, "%s after %d steps" % (name, point), seen)
        assert (got[:, 0] == 0.0).all()  # RWA services carry no bit rate
    _holds(name, seen)
    env.check()
    env.close()


# (c7_s65 and c31_s64: rows beyond the LDS budget, every lane stores its own blocks; c3_s128: one wavefront per workgroup; the c2
# cases: two)
@pytest.mark.parametrize("name,n_envs", [("rmcsa_c7_s65", 24), ("rmcsa_c2_s129", 20), ("rmcsa_c31_s64", 24), ("rmcsa_c2_s512", 24),
                                         ("rmcsa_c3_s128", 24)])
def test_rmcsa_rows_equal_the_restatement(name, n_envs):
    from tests.test_rmcsa_mask_gpu import _agent_steps

    case = slot_agent.CASE_BY_NAME[name]
    C = slot_agent.cores_of(case)
    env = _make("RMCSA", case.kw, n_envs, seeds=list(range(1000, 1000 + n_envs)))
    tab = rr.tables_of(env)
    rs = np.random.RandomState(case.S)
    cores_differ = 0
    for point in (30, 60):
        _agent_steps(env, tab, 30, rs, t0=point - 30)
        got = _check(env, "%s after %d agent steps" % (name, point))
        assert env.link_features_shape()[1] == C * E
        blk = lf.blocks_of(got, env.topology, C)
        cores_differ += int((blk[:, :1, :, :7] != blk[:, :, :, :7]).any(axis=(1, 3)).sum())
        assert np.array_equal(blk[:, :1, :, 7:].repeat(C, axis=1), blk[:, :, :, 7:])  # the link's own columns, the same for every core
    assert cores_differ > 0  # the rows of two cores of one link differ somewhere
    env.check()
    env.close()


@pytest.fixture(scope="module")
def topo_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("link_features_topologies")


# The chunked cases above (c7_s65, c31_s64) stage their rounds on 4 wavefronts per workgroup: with 5 paths the link sets are small.
# The 8 envs' link sets take 128 k bytes and a round of 8 slot rows 256 (10 + k) (csrc/orl_view_plan.h): from k = 26 only 2
# wavefronts' staging fits 48 KiB, from k = 58 only 1.  k6full (6 nodes, 15 links) with 2 cores: 30 blocks of 10 + k values, chunked.
@pytest.mark.parametrize("k,waves", [(40, 2), (64, 1)])
def test_rmcsa_rows_chunked_on_two_and_one_wavefronts(k, waves, topo_dir):
    import optical_rl_gym_amd as orl
    from tests import envelope
    from tests.helpers import view_plan_of

    n, C = 20, 2
    kw = dict(slot_agent.CASE_BY_NAME["rmcsa_c7_s65"].kw, num_spatial_resources=C)
    env = orl.make("RMCSA", topology=envelope.topology_npz("k6full", k, topo_dir), num_envs=n, seeds=list(range(700, 700 + n)), **kw)
    t = env.topology
    plan = view_plan_of(env, "link_features")
    assert plan["ok"] == 1 and plan["chunk"] > 0 and plan["chunk"] < plan["rows"] and plan["waves"] == waves, plan
    busy = 0
    for point in (0, 25, 50):
        if point:
            env.run("SAP_BM_FC_FF", 25)
        env_type, avail, services = pf.state_of(env)
        want = np.float32(lf.restate_fast(env_type, avail, services, t, env.link_stats_all()))
        got = env.link_features()
        dim, rows, width, pitch = env.link_features_shape()
        assert (dim, rows, width) == lf.shape_of(t, C) == (1 + 2 * 6 + C * 15 * (10 + k), C * 15, 10 + k) and pitch == (dim + 3) // 4 * 4
        assert (dim, rows, width, pitch) == tuple(plan[f] for f in ("dim", "rows", "width", "pitch"))
        assert got.shape == want.shape == (n, dim) and got.dtype == np.float32
        bad = np.flatnonzero((_u32(got) != _u32(want)).any(axis=1))
        assert len(bad) == 0, "after %d steps: %d envs differ, first env %d at column %d" % (
            point, len(bad), bad[0], np.flatnonzero(_u32(got[bad[0]]) != _u32(want[bad[0]]))[0])
        busy += int((np.asarray(avail) == 0).sum())
    assert busy > 0  # (rows that are not entirely free)
    env.check()
    env.close()


@pytest.mark.parametrize("n", [32, 27, 9])
def test_rows_after_every_way_of_stepping(n):
    case = slot_agent.CASE_BY_NAME["rmsa_s129"]
    env = _make("RMSA", case.kw, n, seeds=list(range(300, 300 + n)))
    rng = np.random.default_rng(n)
    pf.walk(env, rng, 30)
    _check(env, "%d envs after step(actions)" % n)
    for _ in range(30):
        env.policy_step("SAP_FF", auto_reset=True)
    _check(env, "%d envs after policy_step" % n)
    env.run("SAP_FF", 40)
    _check(env, "%d envs after a device-resident run" % n)
    pf.walk(env, rng, 5)
    _check(env, "%d envs, steps after the run" % n)
    env.check()
    env.close()


def test_zero_copy_view_and_out():
    import torch

    from optical_rl_gym_amd._lib import OrlError

    case = slot_agent.CASE_BY_NAME["rmsa_s129"]
    n = 200  # 25 wavefronts: the last workgroup is not full
    env = _make("RMSA", case.kw, n, seeds=list(range(50, 50 + n)))
    with pytest.raises(OrlError, match=r"link_features\(\)"):
        env.device_array("link_features")
    pf.walk(env, np.random.default_rng(4), 40)
    want = _check(env, "200 envs")
    assert env.link_features(fetch=False) is None
    env.sync()
    v = env.device_tensor("link_features")
    dim, _rows, _width, pitch = env.link_features_shape()
    assert pitch > dim  # (359 columns at a pitch of 360: there is a pad column to look at)
    assert v.shape == (n, dim) and v.dtype == torch.float32 and v.stride() == (pitch, 1)
    assert np.array_equal(_u32(v.cpu().numpy()), _u32(want))
    padded = torch.as_strided(v, (n - 1, pitch), (pitch, 1)).cpu().numpy()  # (the view ends with the last row's last column)
    assert np.array_equal(_u32(padded[:, :dim]), _u32(want[:-1])) and (padded[:, dim:].view(np.uint32) == 0).all()  # pad columns
    out = np.zeros((n, dim), np.float32)
    assert env.link_features(out=out) is out and np.array_equal(_u32(out), _u32(want))
    for bad in (np.zeros((n, dim + 1), np.float32), np.zeros((n, dim), np.float64), np.zeros((dim, n), np.float32).T):
        with pytest.raises(ValueError):
            env.link_features(out=bad)
    env.check()
    env.close()


def test_under_graph_capture():
    import torch

    case = slot_agent.CASE_BY_NAME["rmsa_s129"]
    n = 200
    env = _make("RMSA", case.kw, n, seeds=list(range(50, 50 + n)))
    rng = np.random.default_rng(5)
    pf.walk(env, rng, 20)
    acts = env.device_tensor("actions")
    s = env.torch_stream()

    def load(a):
        full = np.zeros((n, 4), np.int32)
        full[:, :2] = a
        with torch.cuda.stream(s):
            acts.copy_(torch.as_tensor(full, device=acts.device))

    # one serial chain under capture on the batch's stream, after one warm call of each (the first call allocates the buffer)
    load(pf.random_actions(env, rng))
    with torch.cuda.stream(s):
        env.step(None, auto_reset=True, fetch=False)
        env.link_features(fetch=False)
    torch.cuda.synchronize()
    v = env.device_tensor("link_features")
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        env.step(None, auto_reset=True, fetch=False)
        env.link_features(fetch=False)
    torch.cuda.synchronize()
    for _ in range(20):
        load(pf.random_actions(env, rng))
        env.sync()
        g.replay()
        torch.cuda.synchronize()
    got = v.cpu().numpy()
    assert np.array_equal(_u32(got), _u32(np.float32(lf.of_batch(env))))
    assert np.array_equal(_u32(got), _u32(env.link_features()))
    env.check()
    env.close()


def test_two_shards_on_one_gpu_equal_the_whole_batch():
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    case = slot_agent.CASE_BY_NAME["rmsa_s65"]
    n, cut = 100, 36
    seeds = list(range(40, 40 + n))
    whole = _make("RMSA", case.kw, n, seeds=seeds)
    multi = MultiDeviceBatch.from_shards([_make("RMSA", case.kw, cut, seeds=seeds[:cut]), _make("RMSA", case.kw, n - cut, seeds=seeds[cut:])])
    rng = np.random.default_rng(2)
    for _ in range(40):
        a = pf.random_actions(whole, rng)
        whole.step(a, auto_reset=True)
        multi.step(a, auto_reset=True)
    assert multi.link_features_shape() == whole.link_features_shape()
    want = _check(whole, "the whole batch")
    assert np.array_equal(_u32(multi.link_features()), _u32(want))
    out = np.zeros_like(want)
    assert multi.link_features(out=out) is out and np.array_equal(_u32(out), _u32(want))
    assert multi.link_features(fetch=False) is None
    for s in multi.shards:
        s.sync()
    views = np.concatenate([s.device_tensor("link_features").cpu().numpy() for s in multi.shards])
    assert np.array_equal(_u32(views), _u32(want))
    multi.close()
    whole.close()


def test_refusals_and_the_env_state_stays():
    from optical_rl_gym_amd._lib import OrlError

    qos = _make("QoSConstrainedRA", dict(load=10), 16)
    for call in (lambda: qos.link_features(), lambda: qos.link_features(fetch=False), lambda: qos.link_features_shape()):
        with pytest.raises(OrlError, match="QoSConstrainedRA"):
            call()
    with pytest.raises(OrlError, match=r"link_features\(\)"):  # nothing was queued, no buffer exists
        qos.device_array("link_features")
    qos.close()
    for fam, name, policy in (("RMSA", "rmsa_s65", "SAP_FF"), ("RMCSA", "rmcsa_c7_s65", "SAP_BM_FC_FF")):
        env = _make(fam, slot_agent.CASE_BY_NAME[name].kw, 24, seeds=list(range(7, 31)))
        env.run(policy, 30)
        before, flags = env.get_state().copy(), env.flags().copy()
        dim = env.link_features_shape()[0]
        for bad in (np.zeros((24, dim + 1), np.float32), np.zeros((24, dim), np.float64), np.zeros((25, dim), np.float32)):
            with pytest.raises(ValueError):
                env.link_features(out=bad)
        env.link_features()
        env.link_features(fetch=False)
        env.sync()
        assert np.array_equal(env.get_state(), before) and np.array_equal(env.flags(), flags)
        env.check()
        env.close()
