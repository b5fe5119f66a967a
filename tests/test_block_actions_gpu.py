"""Block actions on the device (include/orl.h, orl_batch_block_table / orl_batch_select_blocks; k_block_table and k_select_blocks in
csrc/orl_blocks.h) against the run-length restatement (tests/block_restate.py, pinned to a per-slot loop, to DeepRMSA's block list, to
the oracle's step and to the first-fit tables in tests/test_block_actions.py): table, mask and selection on every restated env,
fetched and in place, indices from the host and from the actions buffer; device against device with the path features, DeepRMSA's
joint mask, assign_spectrum, route_cores and the path-modulation mask; against the step; under graph capture; over a sharded batch;
through the VecEnv; and the refusals.

Cases: the nine shapes of tests/assign_cases.py (W = 1, 2, 5, 8, RWA, 88 links, services of up to 33 slots), four of tests/envelope.py
(k = 9: a second stripe of one row; k = 64; n_paths = 1 < k: rows of missing paths; services of 64 slots) and five RMCSA shapes (W = 1,
2, 5, 8; 20 envs: a half-empty group; 31 cores: 155 rows, the direct form at j = 8)."""
import numpy as np
import pytest

from tests import assign_cases as ac
from tests import block_restate as br
from tests import complete_restate as cr
from tests import path_features_restate as pf
from tests import rmcsa_mask_restate as rr
from tests import route_cores_cases as cc
from tests import slot_agent
from tests.oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6
JS = (1, 3, 8)
ENVELOPE = ("ring10c8_k9_rmsa", "k6full_k64_rwa", "star129_rmsa", "s512_w64_rmsa")
SINGLE = [s.name for s in ac.SHAPES] + list(ENVELOPE)
RMCSA = {"rmcsa_c7_s64": 512, "rmcsa_c7_s65": 512, "rmcsa_c2_s129": 20, "rmcsa_c31_s64": 24, "rmcsa_c2_s512": 24}
WHOLE = ("rmsa_nsf_s65", "rmcsa_c7_s65")  # the 512-env shapes restated on every env; the others on their first 64
POINTS = ("construction", "walk", "crowded", "crafted", "reset")


@pytest.fixture(scope="module")
def topo_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("block_topologies")


class Shape:
    """A named shape opened as a batch: the walk, the crowded maps (where the shape has them) and RMCSA's tables"""

    def __init__(self, name, topo_dir):
        from tests.test_rmcsa_complete_gpu import _agent_steps, _make, crowd
        from tests.test_route_spectrum_gpu import Case

        self.name, self.tab = name, None
        if name in RMCSA:
            kw = slot_agent.CASE_BY_NAME[name].kw
            self.env = _make(kw, RMCSA[name])
            self.tab = rr.tables_of(self.env)
            self.walk = lambda: (_agent_steps(self.env, self.tab, 30, np.random.RandomState(self.env.num_spectrum_resources)),
                                 self.env.run("SAP_BM_FC_FF", 60))
            self.crowd = lambda avail, services: crowd(avail, services, self.env.topology, self.tab)
        else:
            case = Case(name, topo_dir)
            self.env = case.make()
            self.walk = lambda: case.walk(self.env)
            self.crowd = None if case.shape is None else (lambda avail, services: ac.crowd(case.shape, avail[:, 0], services)[:, None])
        self.cn = self.env.num_envs if self.env.num_envs <= 64 or name in WHOLE else 64

    def state(self):
        env_type, avail, services = pf.state_of(self.env)
        return env_type, avail, services


def _differ(what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert len(bad) == 0, "%s: %d envs differ, first %d: got %r, want %r" % (what, len(bad), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


def _check(shape, what, seen):
    """Every restated env of the present state: table, mask and selection for j = 1, 3, 8 (RMCSA: under each path's best and one fixed
    modulation), fetched and in place over buffers filled with junk, indices from the host and from column 0 of the actions buffer, both
    placements; then device against device.  State and flags stay as they are."""
    import torch

    env, cn, tab = shape.env, shape.cn, shape.tab
    n, S = env.num_envs, env.num_spectrum_resources
    snap, flags = env.get_state(), env.flags().copy()
    env_type, avail, services = shape.state()
    rmcsa = env_type == 3
    C = env.num_spatial_resources
    k = env.k_paths
    R = k * C
    stream = env.torch_stream()
    acts = env.device_tensor("actions")
    mods = (None, cc.fixed_modulation(services, env.topology, tab)) if rmcsa else (None,)
    rng = np.random.default_rng(S + n)
    for mod in mods:
        rows = br.Rows(env_type, avail[:cn], services[:cn], env.topology, tab, mod)
        if mod is None:
            br.count_kinds(rows, 3, seen)
        else:
            seen["fixed_beyond_reach"] = seen.get("fixed_beyond_reach", 0) + rows.fixed_beyond_reach
        for j in JS:
            tag = "%s, j = %d, modulation %r" % (what, j, mod)
            dim = R * j + 1
            assert env.block_table_shape(j) == (R, 2 + 2 * j, (R * (2 + 2 * j) + 3) // 4 * 4, dim, (dim + 15) // 16 * 16), tag
            got_t, got_m = env.block_table(j, mod)
            assert got_t.dtype == np.int32 and got_t.shape == (n, R, 2 + 2 * j) and got_m.dtype == np.bool_ and got_m.shape == (n, dim), tag
            _differ(tag + " (table)", got_t[:cn], br.table(rows, j))
            _differ(tag + " (mask)", got_m[:cn], br.mask(rows, j, env.allow_rejection))
            tt, mt = env.device_tensor("block_table"), env.device_tensor("block_mask")
            assert tuple(tt.shape) == (n, R * (2 + 2 * j)) and tt.dtype == torch.int32 and tuple(mt.shape) == (n, dim) and mt.dtype == torch.bool
            with torch.cuda.stream(stream):
                tt.fill_(-7)
                mt.fill_(True)
                assert env.block_table(j, mod, fetch=False) is None
            env.sync()
            assert np.array_equal(tt.cpu().numpy().reshape(n, R, 2 + 2 * j), got_t) and np.array_equal(mt.cpu().numpy(), got_m), tag
            if env_type == 1:
                continue
            idx = rng.integers(-2, R * j + 3, size=n).astype(np.int32)
            idx[:cn] = br.draw_indices(rows, j, rng)
            for placement in ("first", "last"):
                want = br.select(rows, j, idx[:cn], placement)
                got = env.select_blocks(idx, j, mod, placement)
                assert got.shape == (n, 4) and got.dtype == np.int32, tag
                _differ(tag + ", %s, host indices" % placement, got[:cn], want)
                junk = np.full((n, 4), -9, np.int32)
                junk[:, 0] = idx
                with torch.cuda.stream(stream):
                    acts.copy_(torch.as_tensor(junk, device=acts.device))
                    assert env.select_blocks(None, j, mod, placement, fetch=False) is None
                env.sync()
                assert np.array_equal(acts.cpu().numpy(), got), tag
                rej = (want == np.array(rows.reject)).all(axis=1)
                seen["selected"] = seen.get("selected", 0) + int((~rej).sum())
                seen["rejected"] = seen.get("rejected", 0) + int(rej.sum())
    # ---- device against device --------------------------------------------------------------------------------------------------
    N = env.topology.n_nodes
    for j in JS:
        mod = mods[-1]  # (RMCSA: the path features take m for every path, the table only where it is within reach — the rows compared)
        t, m = env.block_table(j, mod)
        feat = env.path_features(j, mod)[:, 1 + 2 * N:].reshape(n, R, 2 * j + 3)
        usable = t[:, :, 0] > 0
        there = (t[:, :, 3::2] > 0) & usable[:, :, None]
        st, ln = t[:, :, 2::2].astype(np.float64), t[:, :, 3::2].astype(np.float64)
        want0, want1 = np.float32(2 * (st - 0.5 * S) / S), np.float32((ln - 8) / 8)
        f0, f1 = feat[:, :, 0:2 * j:2], feat[:, :, 1:2 * j:2]
        assert np.array_equal(f0[there], want0[there]) and np.array_equal(f1[there], want1[there]), (what, j)
        gone = ~there & usable[:, :, None]
        assert (f0[gone] == -1.0).all() and (f1[gone] == -1.0).all(), (what, j)
        if not rmcsa:
            assert (feat[~usable] == -1.0).all(), (what, j)
        assert np.array_equal(m[:, :-1].reshape(n, R, j) & usable[:, :, None], there) or not env.allow_rejection, (what, j)
    if env_type == 1:
        assert np.array_equal(env.block_table(env.j)[1], env.action_mask("joint")), what
    elif not rmcsa:
        for p in range(min(k, 9)):
            for j in (1, 3):
                assert np.array_equal(env.select_blocks(np.full(n, p * j, np.int32), j), env.assign_spectrum("first", paths=np.full(n, p, np.int32))), (what, p, j)
    else:
        pairs = cc.draw_given(n, K, C, 2, shift=3)
        inside = (pairs[:, 0] >= 0) & (pairs[:, 0] < K) & (pairs[:, 1] >= 0) & (pairs[:, 1] < C)
        for j in (1, 3):
            a = np.where(inside, (pairs[:, 0] * C + pairs[:, 1]) * j, -1).astype(np.int32)
            for mod in mods:
                assert np.array_equal(env.select_blocks(a, j, mod), env.route_cores("first", "ksp", paths=pairs[:, 0], cores=pairs[:, 1], modulation=mod)), (what, j, mod)
        # an OR over block 0 of a path's cores = the path-modulation column of m*(p)
        block0 = env.block_table(1)[1][:, :-1].reshape(n, K, C).any(axis=2)
        mstar = cr.best_in_reach(env.services(), env.topology, tab)
        pm = env.action_mask("path_modulation")
        fallback = ~pm[:, -1] & pm[:, :-1].all(axis=1)  # (a row without a provisioning column and no rejection)
        col = np.take_along_axis(pm[:, :-1].reshape(n, K, M), np.maximum(mstar, 0)[:, :, None], axis=2)[:, :, 0] & (mstar >= 0)
        assert np.array_equal(block0[~fallback], col[~fallback]), what
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.flags(), flags), what


@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("name", SINGLE + list(RMCSA))
def test_table_mask_and_selection_equal_the_restatement(name, point, topo_dir):
    """After construction, after the walk, on crowded and on crafted maps set through a snapshot, and after a full reset."""
    from optical_rl_gym_amd._lib import OrlError
    from tests.test_rmcsa_complete_gpu import set_maps

    shape = Shape(name, topo_dir)
    env = shape.env
    if point == "crowded" and shape.crowd is None:
        env.close()
        return  # (the envelope cases have no crowded maps: their crafted ones stand for both)
    for view in ("block_table", "block_mask"):
        with pytest.raises(OrlError, match=r"call block_table\(\)"):
            env.device_tensor(view)
    if point != "construction":
        shape.walk()
    if point in ("crowded", "crafted"):
        snap = env.get_state()
        env_type, avail, services = shape.state()
        maps = shape.crowd(avail, services) if point == "crowded" else br.craft(env_type, avail, services, env.topology, shape.tab)
        set_maps(env, snap, maps)
        assert np.array_equal(shape.state()[1], maps)
    if point == "reset":
        env.reset(full=True)
    seen = {}
    _check(shape, "%s, %s" % (name, point), seen)
    print(name, point, seen)
    assert seen["selected"] > 0 and seen["rejected"] > 0
    if point == "crafted" and env.num_envs >= 64:  # the kinds the crafted maps hold whatever the walk left, where the restated envs are many
        for kind in ("runs_0", "runs_below_j", "runs_j", "ends_at_top", "starts_at_0", "exactly_n"):  # (tests/test_block_actions.py: per family)
            assert seen[kind] > 0, (kind, seen)
    if name == "star129_rmsa":
        assert (env.block_table(1)[0][:, 1:, 0] == 0).any()  # rows of missing paths
    if point in ("crowded", "crafted"):
        env.set_state(snap)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


def test_deeprmsa_mask_is_its_joint_mask_and_selection_is_refused():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    case = slot_agent.CASE_BY_NAME["deep_s129_j4"]
    env = orl.make("DeepRMSA", topology=TOPOLOGY, num_envs=64, seeds=list(range(100, 164)), **case.kw)
    rng = np.random.default_rng(0)
    for point in (0, 50, 100):
        if point:
            pf.walk(env, rng, 50)
        env_type, avail, services = pf.state_of(env)
        rows = br.Rows(1, avail, services, env.topology)
        for j in (1, 4, 8):  # the call's j is independent of the batch's own
            tab, msk = env.block_table(j)
            _differ("deep, %d, j = %d (table)" % (point, j), tab, br.table(rows, j))
            _differ("deep, %d, j = %d (mask)" % (point, j), msk, br.mask(rows, j, env.allow_rejection))
        assert np.array_equal(env.block_table(4)[1], env.action_mask("joint")), point
    snap = env.get_state()
    for fetch in (True, False):
        with pytest.raises(OrlError, match="natively"):
            env.select_blocks(np.zeros(64, np.int32), 4, fetch=fetch)
    assert np.array_equal(env.get_state(), snap)
    env.check()
    env.close()


@pytest.mark.parametrize("j", [1, 3])
def test_deeprmsa_stepped_with_indices_and_rmsa_stepped_with_select_blocks_stay_equal(j):
    """Two batches, same seeds, 200 steps: DeepRMSA takes the index, RMSA select_blocks(fetch=False) and step(None).  Half the envs take a
    set column of the block mask, the others a uniformly random index (absent blocks and the reject action included)."""
    import optical_rl_gym_amd as orl

    n, S = 64, 129
    kw = dict(mean_service_holding_time=10.0, num_spectrum_resources=S, allow_rejection=True, episode_length=50)
    seeds = list(range(300, 300 + n))
    deep = orl.make("DeepRMSA", topology=TOPOLOGY, num_envs=n, seeds=seeds, j=j, mean_service_inter_arrival_time=10.0 / 130, **kw)
    rmsa = orl.make("RMSA", topology=TOPOLOGY, num_envs=n, seeds=seeds, load=130, **kw)
    rng = np.random.default_rng(j)
    placed = absent = 0
    for t in range(200):
        msk = rmsa.block_table(j)[1]
        assert np.array_equal(msk, deep.action_mask("joint")), t
        a = rng.integers(0, K * j + 1, size=n).astype(np.int32)
        for i in range(0, n, 2):
            have = np.flatnonzero(msk[i, :-1])
            if len(have):
                a[i] = have[rng.integers(len(have))]
        deep.step(a.reshape(n, 1), auto_reset=True)
        assert rmsa.select_blocks(a, j, fetch=False) is None
        _, rew, _, _ = rmsa.step(None, auto_reset=True)
        hit = msk[np.arange(n), a] & (a < K * j)
        assert np.array_equal(rew > 0, hit), t  # every selection that is not the reject row provisions
        placed += int(hit.sum())
        absent += int((~hit & (a < K * j)).sum())
        assert np.array_equal(deep.slots_packed(), rmsa.slots_packed()) and np.array_equal(deep.counters(), rmsa.counters()), t
        assert np.array_equal(deep.services(), rmsa.services()), t
    assert placed > 1000 and absent > 0
    for e in (deep, rmsa):
        assert not (e.flags() & 2).any()
        e.check()
        e.close()


@pytest.mark.parametrize("name", ["rmsa_nsf_s129", "rwa_nsf_s65", "rmcsa_c2_s129"])
def test_select_blocks_then_step_against_the_oracle(name, topo_dir):
    """select_blocks(fetch=False); step(None) for 60 steps, j and the placement changing per step, against an oracle stepped with the
    restated action: reward, done, counters, maps and services; accepted exactly where the selection is not the reject row."""
    shape = Shape(name, topo_dir)
    env = shape.env
    if name in RMCSA:
        ora = OracleBackend("RMCSA", TOPOLOGY, list(range(1000, 1000 + env.num_envs)), **slot_agent.CASE_BY_NAME[name].kw)
    else:
        s = ac.SHAPE_BY_NAME[name]
        ora = OracleBackend(s.fam, s.topology, ac.seeds_of(s), **s.kw)
    rng = np.random.default_rng(7)
    accepted = 0
    for t in range(60):
        j, placement = JS[t % 3], ("first", "last")[(t // 3) % 2]
        env_type, avail, services = shape.state()
        rows = br.Rows(env_type, avail, services, env.topology, shape.tab)
        idx = br.draw_indices(rows, j, rng)
        want = br.select(rows, j, idx, placement)
        before = env.counters()[:, 1].copy()
        assert env.select_blocks(idx, j, None, placement, fetch=False) is None
        _, rew, done, _ = env.step(None, auto_reset=True)
        _, rew_o, done_o, _ = ora.step(want, auto_reset=True)
        tag = (name, t, j, placement)
        assert np.array_equal(env.device_tensor("actions").cpu().numpy(), want), tag
        assert np.array_equal(rew, rew_o) and np.array_equal(np.asarray(done, bool), np.asarray(done_o, bool)), tag
        assert np.array_equal(env.counters(), ora.counters()) and np.array_equal(env.services(), ora.services()), tag
        assert np.array_equal(env.slots_packed(), ora.slots_packed()), tag
        hit = ~(want == np.array(rows.reject)).all(axis=1)
        assert np.array_equal(env.counters()[:, 1] - before == 1, hit) or np.asarray(done, bool).any(), tag
        accepted += int(hit.sum())
    assert accepted > 0 and not (env.flags() & 2).any()
    env.check()
    env.close()


def test_mask_index_selection_and_step_captured_in_one_graph():
    """{block_table; the lowest set column into column 0 of the actions; select_blocks; step} captured on the batch's stream after a
    first call outside the capture, replayed 10 times against an eager twin driven through the host."""
    import torch

    import optical_rl_gym_amd as orl

    case = slot_agent.CASE_BY_NAME["rmcsa_c2_s129"]
    n, j = 200, 3  # 25 wavefronts: the last workgroup is not full
    env, twin = (orl.make("RMCSA", topology=TOPOLOGY, num_envs=n, seeds=list(range(50, 50 + n)), **case.kw) for _ in range(2))
    env.run("SAP_BM_FC_FF", 40)
    twin.set_state(env.get_state())
    s = env.torch_stream()
    env.block_table(j, fetch=False)
    acts, mask = env.device_tensor("actions"), env.device_tensor("block_mask")

    def chain():
        env.block_table(j, fetch=False)
        acts[:, 0].copy_(mask.to(torch.uint8).argmax(dim=1).to(torch.int32))
        env.select_blocks(None, j, placement="last", fetch=False)
        env.step(None, auto_reset=True, fetch=False)

    def eager():
        msk = twin.block_table(j)[1]
        twin.select_blocks(msk.argmax(axis=1).astype(np.int32), j, placement="last", fetch=False)
        twin.step(None, auto_reset=True, fetch=False)
        twin.sync()

    with torch.cuda.stream(s):
        chain()
    eager()
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state(), twin.get_state())
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        chain()
    torch.cuda.synchronize()
    for it in range(10):
        g.replay()
        torch.cuda.synchronize()
        eager()
        assert np.array_equal(acts.cpu().numpy(), twin.device_tensor("actions").cpu().numpy()), it
        assert np.array_equal(env.device_tensor("reward").cpu().numpy(), twin.device_tensor("reward").cpu().numpy()), it
        assert np.array_equal(env.get_state(), twin.get_state()), it
    assert env.counters()[:, 1].sum() > 0
    for e in (env, twin):
        assert not (e.flags() & 2).any()
        e.check()
        e.close()


def test_two_shards_equal_the_unsharded_batch():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    case = slot_agent.CASE_BY_NAME["rmsa_s65"]
    n, cut = 100, 36
    seeds = list(range(40, 40 + n))
    make = lambda sd: orl.make("RMSA", topology=TOPOLOGY, num_envs=len(sd), seeds=sd, **case.kw)
    whole, multi = make(seeds), MultiDeviceBatch.from_shards([make(seeds[:cut]), make(seeds[cut:])])
    rng = np.random.default_rng(2)
    for _ in range(40):
        a = pf.random_actions(whole, rng)
        whole.step(a, auto_reset=True)
        multi.step(a, auto_reset=True)
    for j in (1, 4):
        assert multi.block_table_shape(j) == whole.block_table_shape(j)
        (t, m), (u, v) = whole.block_table(j), multi.block_table(j)
        assert np.array_equal(t, u) and np.array_equal(m, v), j
        assert multi.block_table(j, fetch=False) is None
        idx = rng.integers(-1, K * j + 2, size=n).astype(np.int32)
        for placement in ("first", "last"):
            assert np.array_equal(multi.select_blocks(idx, j, placement=placement), whole.select_blocks(idx, j, placement=placement)), (j, placement)
        assert multi.select_blocks(idx, j, fetch=False) is None
        for s in multi.shards:
            s.sync()
        assert np.array_equal(np.concatenate([s.device_tensor("actions").cpu().numpy() for s in multi.shards]), whole.select_blocks(idx, j))
        assert np.array_equal(np.concatenate([s.device_tensor("block_mask").cpu().numpy() for s in multi.shards]), m)
    with pytest.raises(ValueError):
        multi.select_blocks(np.zeros(cut, np.int32))
    multi.close()
    whole.close()


@pytest.mark.parametrize("fam", ["RMSA", "RMCSA"])
def test_vec_env_block_actions_through_a_masked_random_rollout(fam):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    j, n = 3, 48
    kw = slot_agent.CASE_BY_NAME["rmsa_s65" if fam == "RMSA" else "rmcsa_c7_s64"].kw
    batch = orl.make(fam, topology=TOPOLOGY, num_envs=n, seeds=list(range(n)), **kw)
    venv = OpticalVecEnv(batch, block_actions=j, block_placement="last", observation="path_features", path_features_j=j)
    R = K * batch.num_spatial_resources
    assert venv.action_space.n == R * j + 1
    obs = venv.reset()
    assert obs.shape == (n, batch.path_features_shape(j)[0])
    rng = np.random.default_rng(5)
    total = 0
    for t in range(40):
        masks = venv.action_masks()
        assert masks.shape == (n, R * j + 1) and masks.dtype == np.bool_ and masks[:, -1].all()
        a = np.array([rng.choice(np.flatnonzero(masks[i])) for i in range(n)])
        before = batch.counters()[:, 1].copy()
        obs, rew, done, infos = venv.step(a)
        placed = a < R * j
        assert np.array_equal(rew > 0, placed), t  # a set column provisions; the reject action does not
        if not done.any():
            assert np.array_equal(batch.counters()[:, 1] - before, placed.astype(np.int64)), t
        total += int(placed.sum())
    assert total > 10 * n
    for bad in (dict(block_actions=0), dict(block_actions=9)):
        with pytest.raises(Exception):
            OpticalVecEnv(batch, **bad)
    with pytest.raises(ValueError):
        OpticalVecEnv(batch, block_actions=j, block_placement="middle")
    venv.close()


def test_refusals_leave_the_batch_as_it_was():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    qos = orl.make("QoSConstrainedRA", topology=TOPOLOGY, num_envs=16, seeds=list(range(16)), load=10)
    for call in (lambda: qos.block_table(1), lambda: qos.block_table(1, fetch=False), lambda: qos.block_table_shape(1),
                 lambda: qos.select_blocks(np.zeros(16, np.int32)), lambda: qos.select_blocks(fetch=False)):
        with pytest.raises(OrlError, match="QoSConstrainedRA"):
            call()
    qos.close()
    ok = np.zeros(24, np.int32)
    for fam, kw, refused, policy in (
            ("RMSA", slot_agent.CASE_BY_NAME["rmsa_s65"].kw, [dict(j=0), dict(j=9), dict(j=1, modulation=0)], "SAP_FF"),
            ("RMCSA", slot_agent.CASE_BY_NAME["rmcsa_c7_s65"].kw, [dict(j=0), dict(j=9), dict(j=1, modulation=M), dict(j=1, modulation=-2)], "SAP_BM_FC_FF")):
        env, twin = (orl.make(fam, topology=TOPOLOGY, num_envs=24, seeds=list(range(7, 31)), **kw) for _ in range(2))
        env.run(policy, 30)
        twin.run(policy, 30)
        acts = env.device_tensor("actions").cpu().numpy().copy()
        for args in refused:
            for fetch in (True, False):
                with pytest.raises(OrlError):
                    env.block_table(fetch=fetch, **args)
                with pytest.raises(OrlError):
                    env.select_blocks(ok, fetch=fetch, **args)
        for placement in (2, -1):
            for fetch in (True, False):
                with pytest.raises(OrlError, match="placement"):
                    env.select_blocks(ok, 1, placement=placement, fetch=fetch)
        for j in (0, 9):
            with pytest.raises(OrlError):
                env.block_table_shape(j)
        for bad in (dict(blocks=ok[:23]), dict(blocks=ok.astype(np.float64)), dict(placement="middle")):
            with pytest.raises(ValueError):
                env.select_blocks(**bad)
        with pytest.raises(OrlError, match=r"block_table\(\)"):  # nothing was queued, no buffer exists
            env.device_tensor("block_mask")
        env.sync()
        assert np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)
        assert np.array_equal(env.get_state(), twin.get_state()) or np.array_equal(env.slots_packed(), twin.slots_packed())
        for _ in range(10):
            env.step(env.policy(policy), auto_reset=True)
            twin.step(twin.policy(policy), auto_reset=True)
        assert np.array_equal(env.slots_packed(), twin.slots_packed()) and np.array_equal(env.counters(), twin.counters())
        assert np.array_equal(env.block_table(2)[0], twin.block_table(2)[0])
        env.check()
        env.close()
        twin.close()
    one = orl.RMCSAEnv(topology=TOPOLOGY, seed=3, load=100, num_spectrum_resources=64, num_spatial_resources=7)
    one.reset()
    msk = one.block_mask(2)
    assert msk.shape == (K * 7 * 2 + 1,) and msk.dtype == np.bool_
    a = int(np.flatnonzero(msk)[0])
    full = one.block_action(a, j=2)
    assert isinstance(full, tuple) and len(full) == 4 and full == tuple(int(v) for v in one.batch.select_blocks(np.array([a], np.int32), 2)[0])
    assert full == one.route_cores("first", "ksp", path=full[0], core=full[2]) and one.block_action(-1) == (K, M, 7, 64)
    one.close()
    flat = orl.RMSAEnv(topology=TOPOLOGY, seed=3, load=100, num_spectrum_resources=64)
    flat.reset()
    assert flat.block_action(0) == flat.assign_spectrum("first", path=0) and flat.block_action(K) == (K, 64)
    flat.close()
