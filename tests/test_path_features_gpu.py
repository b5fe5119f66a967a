"""The path-feature observation on the device (include/orl.h, orl_batch_path_features; k_path_features in csrc/orl_path_obs.h)
against the numpy restatement of the reference's definitions (tests/path_features_restate.py) on every env, bit for bit as
np.float32 of the float64 rows; against DeepRMSA's own observation; zero-copy, under graph capture, over a sharded batch; and
the calls it refuses."""
import numpy as np
import pytest

from tests import envelope
from tests import path_features_restate as pf
from tests import rmcsa_mask_restate as rr
from tests import slot_agent

pytestmark = pytest.mark.gpu

TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6


def _make(fam, kw, n, seeds=None, topology=TOPOLOGY, **extra):
    import optical_rl_gym_amd as orl

    return orl.make(fam, topology=topology, num_envs=n, seeds=list(range(n)) if seeds is None else seeds, **dict(kw, **extra))


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(env, j, what, modulation=None, tables=None):
    """path_features(j) of every env against np.float32 of the restatement; returns the float64 rows and the services."""
    env_type, avail, services = pf.state_of(env)
    want = pf.restate_fast(env_type, avail, services, env.topology, j, tables, -1 if modulation is None else modulation)
    got = env.path_features(j, modulation)
    dim, rows, pitch = env.path_features_shape(j)
    assert got.shape == want.shape == (env.num_envs, dim) and got.dtype == np.float32 and pitch == (dim + 3) // 4 * 4, what
    assert dim == 1 + 2 * env.topology.n_nodes + rows * (2 * j + 3)
    bad = np.flatnonzero((_u32(got) != _u32(np.float32(want))).any(axis=1))
    assert len(bad) == 0, "%s, j = %d, modulation %r: %d envs differ, first %d" % (what, j, modulation, len(bad), bad[0])
    return want, services


class Seen:
    """What the checked rows held, for the preconditions: rows with exactly j blocks, with fewer, free rows without a fitting
    block, rows without a free slot (existing paths only), rows of paths the pair does not have."""

    def __init__(self):
        self.full = self.fewer = self.nofit = self.busy = self.missing = 0

    def add(self, rows64, services, topo, R, j):
        exists, listed, free = pf.block_counts(rows64, services, topo, R, j)
        self.full += int((exists & (listed == j)).sum())
        self.fewer += int((exists & (listed >= 1) & (listed < j)).sum())
        self.nofit += int((exists & free & (listed == 0)).sum())
        self.busy += int((exists & ~free).sum())
        self.missing += int((~exists).sum())


@pytest.mark.parametrize("name", ["rmsa_s64", "rmsa_s65", "rmsa_s129", "rmsa_s512"])
def test_rmsa_rows_equal_the_restatement(name):
    kw, S = (pf.RMSA_S64_KW, 64) if name == "rmsa_s64" else (slot_agent.CASE_BY_NAME[name].kw, slot_agent.CASE_BY_NAME[name].S)
    env = _make("RMSA", kw, pf.WALK_ENVS, seeds=pf.walk_seeds(S))
    assert env.lib.orl_batch_row_words(env._h) == {64: 1, 65: 2, 129: 5, 512: 8}[S]
    rng, seen = np.random.default_rng(S), {1: Seen(), 4: Seen()}
    for point in pf.WALK_POINTS:
        pf.walk(env, rng, 60)
        for j in (1, 4):
            rows64, services = _check(env, j, "%s after %d steps" % (name, point))
            seen[j].add(rows64, services, env.topology, K, j)
    print(name, {j: vars(s) for j, s in seen.items()})
    if name == "rmsa_s64":  # the only branch that leaves [2 j + 2] at -1 on an existing path
        assert seen[1].busy >= 1 and seen[4].busy >= 1
    if name in ("rmsa_s65", "rmsa_s129"):
        assert seen[4].full > 0 and seen[4].fewer > 0 and seen[4].nofit > 0, vars(seen[4])
    env.check()
    env.close()


def test_deeprmsa_rows_equal_its_own_observation():
    case = slot_agent.CASE_BY_NAME["deep_s129_j4"]
    env = _make("DeepRMSA", case.kw, 64, seeds=list(range(100, 164)))
    rng = np.random.default_rng(0)
    for point in (50, 100, 150):
        pf.walk(env, rng, 50)
        obs = env.observation()
        got = env.path_features(4)
        assert got.shape == obs.shape and np.array_equal(_u32(got), _u32(np.float32(obs))), point
        for j in (1, 4, 8):  # the call's j is independent of the batch's own
            _check(env, j, "deep_s129_j4 after %d steps" % point)
    env.check()
    env.close()


@pytest.mark.parametrize("name", ["rwa_s16", "rwa_s65"])
def test_rwa_rows_equal_the_restatement(name):
    kw, S = (pf.RWA_S16_KW, 16) if name == "rwa_s16" else (slot_agent.CASE_BY_NAME[name].kw, 65)
    env = _make("RWA", kw, pf.WALK_ENVS, seeds=pf.walk_seeds(S))
    rng, seen = np.random.default_rng(S), Seen()
    for point in pf.WALK_POINTS:
        pf.walk(env, rng, 60)
        for j in (1, 4):
            rows64, services = _check(env, j, "%s after %d steps" % (name, point))
            assert (rows64[:, 0] == 0.0).all()  # RWA services carry no bit rate
            assert (rows64[:, 29:].reshape(len(rows64), K, 2 * j + 3)[:, :, 2 * j] == (1 - 5.5) / 3.5).all()  # one wavelength
        if point == 120:
            at_120 = Seen()
            at_120.add(rows64, services, env.topology, K, 4)
        seen.add(rows64, services, env.topology, K, 4)
    print(name, vars(seen))
    if name == "rwa_s16":
        assert at_120.busy > 100, vars(at_120)  # fully busy rows of 320
    env.check()
    env.close()


@pytest.mark.parametrize("name,n_envs", [("rmcsa_c7_s65", 24), ("rmcsa_c2_s129", 20), ("rmcsa_c31_s64", 24), ("rmcsa_c2_s512", 24)])
def test_rmcsa_rows_equal_the_restatement(name, n_envs):
    from tests.test_rmcsa_mask_gpu import _agent_steps

    case = slot_agent.CASE_BY_NAME[name]
    C = slot_agent.cores_of(case)
    env = _make("RMCSA", case.kw, n_envs, seeds=list(range(1000, 1000 + n_envs)))
    tab = rr.tables_of(env)
    assert len(tab["lmax_xt"]) == M
    rs = np.random.RandomState(case.S)
    cores_differ = mods_differ = 0
    for point in (30, 60):
        _agent_steps(env, tab, 30, rs, t0=point - 30)
        for j in (1, 8):  # (c31 at j = 8: rows beyond the LDS budget, every lane stores its own blocks)
            per_mod = {}
            for mod in (None, 0, M - 1):
                rows64, _services = _check(env, j, "%s after %d agent steps" % (name, point), modulation=mod, tables=tab)
                assert env.path_features_shape(j)[1] == K * C
                per_mod[mod] = rows64
            blk = per_mod[None][:, 29:].reshape(n_envs, K, C, 2 * j + 3)
            cores_differ += int((blk[:, :, :1] != blk).any(axis=(2, 3)).sum())
            mods_differ += int((per_mod[0] != per_mod[M - 1]).any(axis=1).sum())
    assert cores_differ > 0 and mods_differ > 0  # rows of two cores of one path differ somewhere; so do two modulations' rows
    env.check()
    env.close()


@pytest.fixture(scope="module")
def topo_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("path_features_topologies")


@pytest.mark.parametrize("name", ["ring10c8_k9_rmsa", "star65_rmsa"])
def test_envelope_more_than_eight_paths_and_missing_paths(name, topo_dir):
    case = {c.name: c for c in envelope.CASES}[name]
    path = envelope.topology_npz(case.topo, case.k, topo_dir)
    seeds = envelope.seeds_of(case)[:case.batch]
    env = _make(case.fam, case.kw, len(seeds), seeds=seeds, topology=path)
    env.run("SAP_FF", case.warm)
    rng, seen = np.random.default_rng(9), Seen()
    for point in (10, 20):
        for _ in range(10):  # (a random path index stays below the pair's path count: beyond it the reference raises IndexError)
            a, services = pf.random_actions(env, rng), env.services()
            n_paths = env.topology.n_paths[services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)]
            a[:, 0] = np.where(a[:, 0] < case.k, np.minimum(a[:, 0], n_paths - 1), a[:, 0])
            env.step(a, auto_reset=True)
        for j in (1, 8):
            rows64, services = _check(env, j, "%s, %d steps after the run" % (name, point))
            seen.add(rows64, services, env.topology, case.k, j)
    if name == "star65_rmsa":
        assert seen.missing > 0  # pairs with fewer than k paths: rows of -1.0
    else:
        assert case.k > 8 and seen.missing == 0
    env.check()
    env.close()


def test_zero_copy_views_and_graph_capture():
    import torch

    from optical_rl_gym_amd._lib import OrlError

    case = slot_agent.CASE_BY_NAME["rmsa_s129"]
    n = 200  # 25 wavefronts: the last workgroup is not full
    env, twin = (_make("RMSA", case.kw, n, seeds=list(range(50, 50 + n))) for _ in range(2))
    with pytest.raises(OrlError, match=r"path_features\(\)"):
        env.device_tensor("path_features")
    rng = np.random.default_rng(4)
    for _ in range(40):
        a = pf.random_actions(twin, rng)
        env.step(a, auto_reset=True)
        twin.step(a, auto_reset=True)
    want4 = twin.path_features(4)
    assert env.path_features(4, fetch=False) is None
    env.sync()
    v4 = env.device_tensor("path_features")
    dim, _rows, pitch = env.path_features_shape(4)
    assert v4.shape == (n, dim) and v4.dtype == torch.float32 and v4.stride() == (pitch, 1)
    assert np.array_equal(_u32(v4.cpu().numpy()), _u32(want4))
    out = np.zeros((n, dim), np.float32)
    assert env.path_features(4, out=out) is out and np.array_equal(_u32(out), _u32(want4))
    for bad in (np.zeros((n, dim + 1), np.float32), np.zeros((n, dim), np.float64), np.zeros((dim, n), np.float32).T):
        with pytest.raises(ValueError):
            env.path_features(4, out=bad)
    env.path_features(1, fetch=False)  # another j has a buffer of its own: the view of j = 4 keeps its rows
    env.sync()
    v1 = env.device_tensor("path_features")
    assert v1.shape == (n, env.path_features_shape(1)[0]) and np.array_equal(_u32(v1.cpu().numpy()), _u32(twin.path_features(1)))
    assert np.array_equal(_u32(v4.cpu().numpy()), _u32(want4))
    # one serial chain under capture on the batch's stream, after one warm call of each
    acts = env.device_tensor("actions")
    s = env.torch_stream()

    def load(a):
        full = np.zeros((n, 4), np.int32)
        full[:, :2] = a
        with torch.cuda.stream(s):
            acts.copy_(torch.as_tensor(full, device=acts.device))

    a = pf.random_actions(twin, rng)
    load(a)
    with torch.cuda.stream(s):
        env.step(None, auto_reset=True, fetch=False)
        env.path_features(4, fetch=False)
    twin.step(a, auto_reset=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        env.step(None, auto_reset=True, fetch=False)
        env.path_features(4, fetch=False)
    torch.cuda.synchronize()
    for _ in range(3):
        a = pf.random_actions(twin, rng)
        load(a)
        env.sync()
        g.replay()
        torch.cuda.synchronize()
        twin.step(a, auto_reset=True)
        assert np.array_equal(_u32(v4.cpu().numpy()), _u32(twin.path_features(4)))
    assert np.array_equal(env.slots_packed(), twin.slots_packed()) and np.array_equal(env.services(), twin.services())
    env.check()
    env.close()
    twin.close()


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
    assert multi.path_features_shape(4) == whole.path_features_shape(4)
    want = whole.path_features(4)
    assert np.array_equal(_u32(multi.path_features(4)), _u32(want))
    out = np.zeros_like(want)
    assert multi.path_features(4, out=out) is out and np.array_equal(_u32(out), _u32(want))
    assert multi.path_features(4, fetch=False) is None
    for s in multi.shards:
        s.sync()
    views = np.concatenate([s.device_tensor("path_features").cpu().numpy() for s in multi.shards])
    assert np.array_equal(_u32(views), _u32(want))
    multi.close()
    whole.close()


def _state(env):
    return env.slots_packed().copy(), env.services().copy(), env.counters().copy()


def test_refusals_leave_the_batch_as_it_was():
    from optical_rl_gym_amd._lib import OrlError

    qos = _make("QoSConstrainedRA", dict(load=10), 16)
    for call in (lambda: qos.path_features(1), lambda: qos.path_features(1, fetch=False), lambda: qos.path_features_shape(1)):
        with pytest.raises(OrlError, match="QoSConstrainedRA"):
            call()
    qos.close()
    case = slot_agent.CASE_BY_NAME["rmsa_s65"]
    rcase = slot_agent.CASE_BY_NAME["rmcsa_c7_s65"]
    for fam, kw, refused, policy in (
            ("RMSA", case.kw, [dict(j=0), dict(j=9), dict(j=1, modulation=0)], "SAP_FF"),
            ("RMCSA", rcase.kw, [dict(j=0), dict(j=9), dict(j=1, modulation=M), dict(j=1, modulation=-2)], "SAP_BM_FC_FF")):
        env, twin = (_make(fam, kw, 24, seeds=list(range(7, 31))) for _ in range(2))
        env.run(policy, 30)
        twin.run(policy, 30)
        for args in refused:
            for fetch in (True, False):
                with pytest.raises(OrlError):
                    env.path_features(fetch=fetch, **args)
        for j in (0, 9):
            with pytest.raises(OrlError):
                env.path_features_shape(j)
        with pytest.raises(OrlError, match=r"path_features\(\)"):  # nothing was queued, no buffer exists
            env.device_tensor("path_features")
        for a, b in zip(_state(env), _state(twin)):
            assert np.array_equal(a, b)
        for _ in range(10):
            env.step(env.policy(policy), auto_reset=True)
            twin.step(twin.policy(policy), auto_reset=True)
        for a, b in zip(_state(env), _state(twin)):
            assert np.array_equal(a, b)
        assert np.array_equal(_u32(env.path_features(2)), _u32(twin.path_features(2)))
        env.check()
        env.close()
        twin.close()
