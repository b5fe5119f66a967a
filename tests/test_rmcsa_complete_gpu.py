"""First-fit completion of partial RMCSA actions on the device (include/orl.h, orl_batch_complete_actions; k_rmcsa_complete in
csrc/orl_rmcsa_complete.h) against the numpy restatement (tests/complete_restate.py, pinned to the oracle's step in
tests/test_rmcsa_complete.py) on every env, against the step itself, from every source of the prefix, under graph capture, over a
sharded batch, through the VecEnv's one-head action spaces and through a one-head masked agent."""
import functools

import numpy as np
import pytest

from tests import complete_restate as cr
from tests import rmcsa_mask_restate as rr
from tests import slot_agent

pytestmark = pytest.mark.gpu

TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6
# the shapes of slot_agent's RMCSA cases, the smallest at which the kernel can go wrong: (case, envs)
SHAPES = [("rmcsa_c7_s64", 512),   # W = 1: the last bit of the word
          ("rmcsa_c7_s65", 512),   # W = 2: one slot in the second word
          ("rmcsa_c3_s128", 24),   # worst_xt = -54.8: the crosstalk limit binds
          ("rmcsa_c2_s129", 20),   # W = 5, 20 envs: the third group of 8 is half empty
          ("rmcsa_c31_s64", 24),   # 155 (path, core) pairs: 20 chunks of 8
          ("rmcsa_c2_s512", 24)]   # W = 8, discrete rates (40, 100, 400): services of up to 33 slots
AGENT_ENVS = 24  # envs the boundary-seeking agent drives (a Python loop per env); the others of a larger batch take the heuristic's action


def _make(kw, n, seed0=1000, seeds=None, **extra):
    import optical_rl_gym_amd as orl

    return orl.make("RMCSA", topology=TOPOLOGY, num_envs=n, seeds=list(range(seed0, seed0 + n)) if seeds is None else seeds, **dict(kw, **extra))


def _state(env):
    t = env.topology
    return rr.unpack_cores(env.slots_packed(), env.num_spatial_resources, t.n_links, env.num_spectrum_resources), env.services().copy()


def _agent_steps(env, tab, n_steps, rng, t0=0):
    """n_steps of slot_agent's RMCSA agent on the device's read-back state (the first AGENT_ENVS envs; SAP_BM_FC_FF's action elsewhere)."""
    S, C, n = env.num_spectrum_resources, env.num_spatial_resources, min(env.num_envs, AGENT_ENVS)
    for t in range(t0, t0 + n_steps):
        avail, services = _state(env)
        acts = env.policy("SAP_BM_FC_FF").copy() if env.num_envs > n else np.zeros((n, 4), np.int32)
        acts[:n] = slot_agent.rmcsa_agent_actions(avail[:n], services[:n], env.topology, tab, t, rng, S, C)[0]
        env.step(acts, auto_reset=True)


def draw_prefix(services, topo, tab, rng, g, C):
    """A prefix [n, g] per env, by env index mod 7 as _draw_given of tests/test_rmcsa_mask_gpu.py: 0-1 a pair within reach, 2 p = k
    (>= n_paths), 3 m = M, 4 a negative entry, 5 beyond lmax_snr, 6 beyond lmax_xt (alone where such a pair exists); the core is
    drawn in range, and for g = 3 the index runs mod 9: 7 c = C, 8 c = -1 under a pair within reach."""
    src, dst = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)
    br = np.array([tab["rate_index"][int(b)] for b in services[:, 4]], np.int64)
    length = tab["path_length"][src, dst][:, :, None]
    has = (np.arange(K)[None, :] < topo.n_paths[src, dst][:, None])[:, :, None]
    xt, snr = has & (length < tab["lmax_xt"][None, None, :]), has & (length < tab["lmax_snr"].T[br][:, None, :])
    n = len(services)
    given = np.zeros((n, 3), np.int32)

    def pick(mask):
        idx = np.flatnonzero(mask.ravel())
        return np.unravel_index(idx[rng.integers(len(idx))], mask.shape) if len(idx) else None

    for i in range(n):
        kind = i % (9 if g == 3 else 7)
        pair = (rng.integers(K), rng.integers(M))
        core = rng.integers(C)
        if kind <= 1 or kind >= 7:
            pair = pick(xt[i] & snr[i]) or pair
            core = {7: C, 8: -1}.get(kind, core)
        elif kind == 2:
            pair = (K, pair[1])
        elif kind == 3:
            pair = (pair[0], M)
        elif kind == 4:
            pair = (-1, pair[1]) if i % 2 else (pair[0], -1)
        elif kind == 5:
            pair = pick(has[i] & ~snr[i]) or pair
        else:
            pair = pick(snr[i] & ~xt[i]) or pick(has[i] & ~xt[i]) or pair
        given[i] = (pair[0], pair[1], core)
    return np.ascontiguousarray(given[:, :g])


def crowd(avail, services, topo, tab):
    """Slot maps no walk at these loads makes (the maps of the shapes stay below 12 % utilisation: no path is ever without room):
    `avail` with further slots taken, by env index mod 4 — 0: every slot of every row taken with a probability that grows with the
    index; 1: the first link of path 0 full in every core (path 0 has no room, later paths may); 2: only the top n slots free
    everywhere, n = the slots of m*(path 0) (a completion lands on S - n); 3: core 0 full."""
    out = avail.copy()
    n, C, _, S = avail.shape
    rng = np.random.default_rng(S + C)
    mstar, need = cr.best_in_reach(services, topo, tab), cr.slots_of(services, tab)
    for i in range(n):
        src, dst = int(services[i, 2]), int(services[i, 3])
        kind = i % 4
        if kind == 0:
            out[i] &= rng.random(out[i].shape) >= 0.04 * (1 + (i // 4) % 12)
        elif kind == 1:
            out[i, :, int(topo.path_links[src, dst, 0, 0]), :] = False
        elif kind == 2:
            out[i, :, :, :S - int(need[i, max(int(mstar[i, 0]), 0)])] = False
        else:
            out[i, 0] = False
    return out


def expected(avail, services, topo, tab, rng, seen):
    """[(g, given, want)] for g = 0 .. 3 on one state, with the kinds it holds counted into `seen`"""
    C = avail.shape[1]
    pv = rr.prov_all(avail, services, topo, tab)
    pv_free = rr.prov_all(avail, services, topo, cr.free_tables(tab))
    out = []
    for g in range(4):
        given = draw_prefix(services, topo, tab, rng, g, C) if g else None
        want = cr.complete(pv, services, topo, tab, g, given)
        seen.count(pv, pv_free, services, topo, tab, g, given, want)
        out.append((g, given, want))
    return out


def _check(env, tab, what, rng, seen):
    avail, services = _state(env)
    for g, given, want in expected(avail, services, env.topology, tab, rng, seen):
        got = env.complete_actions(given=given, n_given=g)
        assert got.shape == want.shape and got.dtype == np.int32, (what, g)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "%s, g = %d: %d envs differ, first %d: given %r, got %r, want %r" % (
            what, g, len(bad), bad[0], None if given is None else given[bad[0]], got[bad[0]], want[bad[0]])


def set_maps(env, snap, avail):
    """The snapshot `snap` of env with the slot maps `avail` (bool [n, C, links, S]) in place of its own, restored into env."""
    n, C, E, S = avail.shape
    lay = env.state_layout()
    words = env.lib.orl_batch_map_words(env._h)
    W = env.lib.orl_batch_row_words(env._h)
    assert lay[2] == 8 * words and words >= C * E * W
    bits = np.zeros((n, C * E, 64 * W), np.uint8)
    bits[:, :, :S] = avail.reshape(n, C * E, S)
    packed = np.packbits(bits, axis=2, bitorder="little").view("<u8").reshape(n, C * E * W)
    buf = snap.copy()
    off = n * (lay[0] + lay[1])
    maps = buf[off:off + n * lay[2]].view(np.uint64).reshape(n, words)
    maps[:, :C * E * W] = packed
    env.set_state(buf)


@functools.lru_cache(maxsize=None)
def _walk(name, n_envs, allow_rejection):
    """Every env of the shape against the restatement at every point; returns what the checked states held."""
    case = slot_agent.CASE_BY_NAME[name]
    env = _make(case.kw, n_envs, allow_rejection=allow_rejection)
    assert env.lib.orl_batch_row_words(env._h) == {64: 1, 65: 2, 128: 2, 129: 5, 512: 8}[case.S]
    tab = rr.tables_of(env)
    rng, seen = np.random.default_rng(case.S), cr.Seen()
    _check(env, tab, "after construction", rng, seen)
    _agent_steps(env, tab, 60, np.random.RandomState(case.S))
    _check(env, tab, "after 60 agent steps", rng, seen)
    env.run("SAP_BM_FC_FF", 100)
    _check(env, tab, "after run(SAP_BM_FC_FF, 100)", rng, seen)
    # crowded maps under the same pending services, through a snapshot (no step follows: the snapshot is put back)
    snap = env.get_state()
    avail, services = _state(env)
    set_maps(env, snap, crowd(avail, services, env.topology, tab))
    assert np.array_equal(_state(env)[0], crowd(avail, services, env.topology, tab))
    _check(env, tab, "on crowded maps", rng, seen)
    env.set_state(snap)
    env.reset(full=True)
    _check(env, tab, "after a full reset", rng, seen)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()
    return seen


@pytest.mark.parametrize("allow_rejection", [False, True])
@pytest.mark.parametrize("name,n_envs", SHAPES)
def test_completion_equals_restatement_on_every_env(name, n_envs, allow_rejection):
    """After construction, after 60 agent steps, after run("SAP_BM_FC_FF", 100), on crowded maps and after a full reset, for
    g = 0 .. 3.  Every shape must hold the six kinds of tests/test_rmcsa_complete.py itself: a completion on s = S - n, one in a
    core above 0, g = 0 choosing a path above 0, a reject by reach alone, one by occupancy alone, m*(p) other than the path's
    best-modulation byte."""
    seen = _walk(name, n_envs, allow_rejection)
    print(name, allow_rejection, vars(seen))
    assert seen.all_positive(), vars(seen)


@pytest.mark.parametrize("allow_rejection", [False, True])
def test_completion_predicts_the_step(allow_rejection):
    C, S, n = 3, 40, 64
    kw = dict(slot_agent.CASE_BY_NAME["rmcsa_c7_s64"].kw, num_spatial_resources=C, num_spectrum_resources=S, allow_rejection=allow_rejection)
    env = _make(kw, n, seed0=77)
    tab = rr.tables_of(env)
    _agent_steps(env, tab, 80, np.random.RandomState(8))
    snap = env.get_state()
    acc0 = env.counters()[:, 1].copy()
    avail, services = _state(env)
    bare = rr.restate_rmcsa_fast(avail, services, env.topology, tab, "path_modulation", allow_rejection=allow_rejection, fallback=False)[:, :-1]
    pm = env.action_mask("path_modulation")[:, :-1]
    fb = ~bare.any(axis=1)
    assert np.array_equal(pm[~fb], bare[~fb]) and (pm[fb].all() if not allow_rejection else not pm[fb].any())
    reject = np.array([K, M, C, S])

    def stepped(given, g):
        """accepted [n] after complete_actions(given) + step(None) from the snapshot; the completion touches no state byte"""
        env.set_state(snap)
        done = env.complete_actions(given=given, n_given=g)
        assert np.array_equal(env.get_state(), snap), (g, None if given is None else given[0])
        env.step(None)
        assert not (env.flags() & 2).any()
        acc = env.counters()[:, 1] - acc0
        assert np.array_equal(acc == 1, ~(done == reject).all(axis=1)) and set(np.unique(acc)) <= {0, 1}
        return acc == 1

    for p in range(K):
        for m in range(M):
            assert np.array_equal(stepped(np.tile(np.array([p, m], np.int32), (n, 1)), 2), bare[:, p * M + m]), (p, m)
        assert np.array_equal(stepped(np.full((n, 1), p, np.int32), 1), bare[:, p * M:(p + 1) * M].any(axis=1)), p
    assert np.array_equal(stepped(None, 0), bare.any(axis=1))
    assert 0 < bare.any(axis=1).sum() < n and 0 < bare.sum() < bare.size  # (both kinds of row and of column)
    for g, pre in ((1, (K,)), (1, (-1,)), (2, (K + 2, -3)), (2, (0, M)), (3, (0, 0, C)), (3, (0, 0, -1)), (3, (-5, M + 1, C + 7))):
        assert not stepped(np.tile(np.array(pre, np.int32), (n, 1)), g).any(), pre
    env.set_state(snap)
    env.check()
    env.close()


def test_sources_of_the_prefix_and_graph_capture():
    import torch

    case = slot_agent.CASE_BY_NAME["rmcsa_c7_s65"]
    n = 128
    env, twin = _make(case.kw, n, seed0=31), _make(case.kw, n, seed0=31)
    tab = rr.tables_of(env)
    rng = np.random.default_rng(6)
    env.run("SAP_BM_FC_FF", 60)
    # the twin starts from env's snapshot, not from a run of its own: a snapshot also holds the records of release slots that were
    # never used or are free again, which no kernel initialises, and two batches agree on those bytes only when one was copied
    # from the other
    twin.set_state(env.get_state())
    acts = env.device_tensor("actions")
    s = env.torch_stream()
    reject = np.array([K, M, 7, case.S])

    avail, services = _state(twin)
    pv = rr.prov_all(avail, services, twin.topology, tab)  # (nothing below steps an env before the captured loop)

    def want_of(given, g):
        return cr.complete(pv, services, twin.topology, tab, g, given)

    # a host `given`: the actions buffer is written by the kernel only, all four columns, the prefix as given where it is valid
    for g in (1, 2, 3):
        given = draw_prefix(twin.services(), twin.topology, tab, rng, g, 7)
        with torch.cuda.stream(s):
            acts.fill_(-7)
            assert env.complete_actions(given=given if g > 1 else given[:, 0], fetch=False) is None
        env.sync()
        got, want = acts.cpu().numpy(), want_of(given, g)
        assert np.array_equal(got, want), g
        ok = ~(got == reject).all(axis=1)
        assert 0 < ok.sum() < n and np.array_equal(got[ok, :g], given[ok])
    # given=None: what a torch write on the batch's stream put into the actions tensor
    for g in (0, 1, 2, 3):
        given = draw_prefix(twin.services(), twin.topology, tab, rng, 3, 7)
        with torch.cuda.stream(s):
            acts.fill_(-7)
            acts[:, :3].copy_(torch.as_tensor(given, dtype=torch.int32, device=acts.device))
            env.complete_actions(n_given=g, fetch=False)
        env.sync()
        assert np.array_equal(acts.cpu().numpy(), want_of(given[:, :g], g)), g
    # {complete; step} captured on the batch's stream (both have run: nothing is allocated inside), replayed with fresh pairs,
    # against an eager twin
    def load(pairs):
        with torch.cuda.stream(s):
            acts[:, :2].copy_(torch.as_tensor(pairs, dtype=torch.int32, device=acts.device))

    def eager(pairs):
        twin.complete_actions(given=pairs, fetch=False)
        twin.step(None, auto_reset=True, fetch=False)
        twin.sync()
        return twin.device_tensor("reward").cpu().numpy(), twin.device_tensor("done").cpu().numpy()

    def same_state(what):
        a, b = env.get_state(), twin.get_state()
        if not np.array_equal(a, b):  # which section of the snapshot (state_layout), and the first env in it
            off, where = 0, []
            for sec, row in enumerate(env.state_layout()):
                d = np.flatnonzero((a[off:off + n * row] != b[off:off + n * row]).reshape(n, row).any(axis=1))
                if len(d):
                    where.append((sec, len(d), int(d[0])))
                off += n * row
            raise AssertionError("%s: snapshots differ in (section, envs, first env) %r" % (what, where))

    pairs = draw_prefix(twin.services(), twin.topology, tab, rng, 2, 7)
    load(pairs)
    with torch.cuda.stream(s):
        env.complete_actions(n_given=2, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    eager(pairs)
    torch.cuda.synchronize()
    same_state("after the eager step of both")
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        env.complete_actions(n_given=2, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    torch.cuda.synchronize()
    rew, done = env.device_tensor("reward"), env.device_tensor("done")
    for it in range(3):
        pairs = draw_prefix(twin.services(), twin.topology, tab, rng, 2, 7)
        load(pairs)
        env.sync()
        g.replay()
        torch.cuda.synchronize()
        r, d = eager(pairs)
        assert np.array_equal(rew.cpu().numpy(), r) and np.array_equal(done.cpu().numpy(), d)
        assert np.array_equal(acts.cpu().numpy(), twin.device_tensor("actions").cpu().numpy())
        same_state("replay %d" % it)
    for e in (env, twin):
        e.check()
        e.close()


@pytest.mark.parametrize("fam,kw", [("RMSA", dict(load=100, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64)),
                                    ("DeepRMSA", dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=2, episode_length=50)),
                                    ("RWA", dict(load=450, mean_service_holding_time=25, episode_length=1000, allow_rejection=True)),
                                    ("QoSConstrainedRA", dict(load=10))])
def test_other_families_refuse_the_completion(fam, kw):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = orl.make(fam, topology=TOPOLOGY, num_envs=16, seeds=list(range(16)), **kw)
    snap = env.get_state()
    acts = env.device_tensor("actions").cpu().numpy().copy()
    for fetch in (True, False):
        for g in (0, 1, 2, 3):
            with pytest.raises(OrlError, match="RMCSA only"):
                env.complete_actions(n_given=g, fetch=fetch)
        with pytest.raises(OrlError, match="RMCSA only"):
            env.complete_actions(given=np.zeros((16, 2), np.int32), fetch=fetch)
    env.sync()
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    env.close()


def test_arguments_are_checked():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = _make(dict(load=100, num_spectrum_resources=64, num_spatial_resources=7), 16)
    env.complete_actions(n_given=0)
    acts = env.device_tensor("actions").cpu().numpy().copy()
    ok = np.zeros((16, 2), np.int32)
    for fetch in (True, False):
        for g in (-1, 4):
            with pytest.raises(OrlError, match="outside 0 .. 3"):
                env.complete_actions(n_given=g, fetch=fetch)
            with pytest.raises(OrlError, match="outside 0 .. 3"):
                env.complete_actions(given=ok, n_given=g, fetch=fetch)
        with pytest.raises(OrlError, match="n_given == 0"):
            env.complete_actions(given=ok, n_given=0, fetch=fetch)
    env.sync()
    assert np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    for bad in (np.zeros((16, 4), np.int32), np.zeros((15, 2), np.int32), np.zeros(32, np.int32), np.zeros((16, 2), np.float64),
                np.zeros((16, 0), np.int32), np.zeros((16, 2, 1), np.int32)):
        with pytest.raises(ValueError):
            env.complete_actions(given=bad)
    with pytest.raises(ValueError):
        env.complete_actions(given=ok, n_given=3)
    with pytest.raises(ValueError):
        env.complete_actions()
    assert env.complete_actions(given=ok).shape == (16, 4) and env.complete_actions(given=np.zeros(16, np.int64)).shape == (16, 4)
    env.close()
    one = orl.RMCSAEnv(topology=TOPOLOGY, seed=3, load=100, num_spectrum_resources=64, num_spatial_resources=7)
    one.reset()
    full = one.complete_action()
    assert isinstance(full, tuple) and len(full) == 4 and all(isinstance(v, int) for v in full)
    assert full == tuple(int(v) for v in one.batch.complete_actions(n_given=0)[0])
    if full != (K, M, 7, 64):
        assert one.complete_action(full[:1]) == full and one.complete_action(full[:2]) == full and one.complete_action(full[:3]) == full
    assert one.complete_action((K,)) == (K, M, 7, 64)
    with pytest.raises(ValueError):
        one.complete_action((0, 0, 0, 0))
    one.close()


def test_multi_device_batch_cuts_given_by_shard():
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    case = slot_agent.CASE_BY_NAME["rmcsa_c7_s65"]
    n, cut = 200, 72
    seeds = list(range(40, 40 + n))
    whole = _make(case.kw, n, seeds=seeds)
    multi = MultiDeviceBatch.from_shards([_make(case.kw, cut, seeds=seeds[:cut]), _make(case.kw, n - cut, seeds=seeds[cut:])])
    tab = rr.tables_of(whole)
    rng = np.random.RandomState(2)
    for t in range(20):
        avail, services = _state(whole)
        acts = whole.policy("SAP_BM_FC_FF").copy()
        acts[:AGENT_ENVS] = slot_agent.rmcsa_agent_actions(avail[:AGENT_ENVS], services[:AGENT_ENVS], whole.topology, tab, t, rng, case.S, 7)[0]
        whole.step(acts, auto_reset=True)
        multi.step(acts, auto_reset=True)
    avail, services = _state(whole)
    for g in (1, 2):
        given = draw_prefix(services, whole.topology, tab, np.random.default_rng(g), g, 7)
        want = whole.complete_actions(given=given)
        assert np.array_equal(want, cr.complete_state(avail, services, whole.topology, tab, g, given))
        assert np.array_equal(multi.complete_actions(given=given), want), g
        assert multi.complete_actions(given=given, fetch=False) is None
        for s in multi.shards:
            s.sync()
        assert np.array_equal(np.concatenate([s.device_tensor("actions").cpu().numpy() for s in multi.shards]), want), g
        with pytest.raises(ValueError):
            multi.complete_actions(given=given[:cut])
    multi.close()
    whole.close()


def _bare_rows(env, tab):
    avail, services = _state(env)
    return rr.restate_rmcsa_fast(avail, services, env.topology, tab, "path_modulation", allow_rejection=env.allow_rejection, fallback=False)[:, :-1]


@pytest.mark.parametrize("mode", ["path_modulation", "path"])
def test_vec_env_one_head_action_spaces(mode):
    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    n = 32
    env = _make(rr.AGENT_KW, n, seeds=rr.AGENT_SEEDS[:n])
    tab = rr.tables_of(env)
    with pytest.raises(ValueError):
        OpticalVecEnv(env, action_completion="core_slot")
    plain = OpticalVecEnv(env)
    assert tuple(plain.action_space.nvec) == (K, M, 7, 64) and plain.action_completion is None  # (the default: nothing changes)
    venv = OpticalVecEnv(env, action_completion=mode)
    cols = K * M if mode == "path_modulation" else K
    assert int(venv.action_space.n) == cols + 1 and not hasattr(venv.action_space, "nvec")
    venv.reset()
    rng = np.random.default_rng(5)
    kinds = [0, 0]
    for t in range(50):
        masks = venv.action_masks()
        pm = env.action_mask("path_modulation")
        want = pm if mode == "path_modulation" else np.concatenate([pm[:, :-1].reshape(n, K, M).any(axis=2), pm[:, -1:]], axis=1)
        assert masks.shape == (n, cols + 1) and masks.dtype == np.bool_ and np.array_equal(masks, want)
        assert np.array_equal(np.stack(venv.env_method("action_masks")), masks)
        fb = ~_bare_rows(env, tab).any(axis=1)
        actions = rr.sample_columns(masks, rng)
        if t % 10 == 9:
            actions[0] = cols  # the reject action of the one-head space
            fb[0] = True
        before = env.counters()[:, 1].copy()
        venv.step_async(actions)
        venv.step_wait()
        assert np.array_equal(env.counters()[:, 1] - before, (~fb).astype(np.int64))
        kinds[0] += int(fb.sum())
        kinds[1] += int((~fb).sum())
    assert min(kinds) > 0 and not (env.flags() & 2).any()
    env.check()
    venv.close()


def test_maskable_ppo_trains_on_the_one_head_space():
    pytest.importorskip("sb3_contrib")
    from sb3_contrib import MaskablePPO

    from optical_rl_gym_amd.vec_env import OpticalVecEnv

    env = _make(dict(rr.AGENT_KW, episode_length=20), 8, seeds=rr.AGENT_SEEDS[:8])
    venv = OpticalVecEnv(env, action_completion="path_modulation", observation="path_features")
    model = MaskablePPO("MlpPolicy", venv, n_steps=16, batch_size=32, n_epochs=1, device="cpu", seed=1)
    model.learn(total_timesteps=256)
    assert env.counters()[:, 0].sum() >= 256 and not (env.flags() & 2).any()
    venv.close()


def test_one_head_masked_agent():
    """Uniformly from the path-modulation row, completed with g = 2, stepped from the device-resident actions: every env-step whose
    row had a provisioning column provisions, no fallback one does."""
    n, steps = 24, 200
    env = _make(rr.AGENT_KW, n, seeds=rr.AGENT_SEEDS[:n])
    tab = rr.tables_of(env)
    rng = np.random.default_rng(rr.AGENT_SEED)
    fallback, accepted = [], []
    for _ in range(steps):
        col = rr.sample_columns(env.action_mask("path_modulation"), rng)
        fallback.append(~_bare_rows(env, tab).any(axis=1))
        before = env.counters()[:, 1].copy()
        env.complete_actions(given=np.stack([col // M, col % M], axis=1).astype(np.int32), fetch=False)
        env.step(None, auto_reset=True)
        accepted.append(env.counters()[:, 1] - before)
    fallback, accepted = np.array(fallback), np.array(accepted)
    assert np.array_equal(accepted, (~fallback).astype(accepted.dtype))
    assert 0 < fallback.sum() < fallback.size and not (env.flags() & 2).any()
    print("fallback share %.4f" % fallback.mean())
    env.check()
    env.close()
