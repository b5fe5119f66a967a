"""RMCSA's two-stage action masks on the device (include/orl.h, ORL_MASK_PATH_MOD / ORL_MASK_CORE_SLOT; k_rmcsa_mask in
csrc/orl_rmcsa_mask.h) against the numpy restatement of the reference's definitions (tests/rmcsa_mask_restate.py) on every env,
against the step itself (a column is 1 exactly when stepping it provisions the service), zero-copy, under graph capture, through
a two-stage masked agent and over a sharded batch."""
import numpy as np
import pytest

from tests import rmcsa_mask_restate as rr
from tests import slot_agent

pytestmark = pytest.mark.gpu

TOPOLOGY = slot_agent.TOPOLOGY
K, M = 5, 6
# the shapes of slot_agent's RMCSA cases: (case, envs, allow_rejection) — the fallback rule under both settings
CASES = [("rmcsa_c7_s64", 512, True),    # W = 1: the last bit of the word
         ("rmcsa_c7_s65", 512, False),   # W = 2: one slot in the second word
         ("rmcsa_c3_s128", 24, True),    # worst_xt = -54.8: the crosstalk limit binds
         ("rmcsa_c2_s129", 20, False),   # W = 5, 20 envs: the third group of 8 is half empty
         ("rmcsa_c17_s65", 24, True),
         ("rmcsa_c31_s64", 24, False),   # the core field full, the largest rows in LDS per slot word
         ("rmcsa_c2_s512", 24, True)]    # W = 8, discrete rates (40, 100, 400): services of up to 33 slots
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


def _reach(services, tab):
    """(within lmax_xt, within lmax_snr): bool [n, K, M] each"""
    src, dst = services[:, 2].astype(np.int64), services[:, 3].astype(np.int64)
    br = np.array([tab["rate_index"][int(b)] for b in services[:, 4]], np.int64)
    length = tab["path_length"][src, dst][:, :, None]
    return length < tab["lmax_xt"][None, None, :], length < tab["lmax_snr"].T[br][:, None, :]


def _draw_given(services, tab, rng):
    """A pair per env, by env index mod 7: 0-1 a pair within reach, 2 p = k (>= n_paths), 3 m = M, 4 a negative entry, 5 beyond
    lmax_snr, 6 beyond lmax_xt (alone where such a pair exists)."""
    xt, snr = _reach(services, tab)
    n = len(services)
    given = np.zeros((n, 2), np.int32)

    def pick(mask):
        idx = np.flatnonzero(mask.ravel())
        return np.unravel_index(idx[rng.integers(len(idx))], mask.shape) if len(idx) else None

    for i in range(n):
        kind = i % 7
        pair = (rng.integers(K), rng.integers(M))
        if kind <= 1:
            pair = pick(xt[i] & snr[i]) or pair
        elif kind == 2:
            pair = (K, pair[1])
        elif kind == 3:
            pair = (pair[0], M)
        elif kind == 4:
            pair = (-1, pair[1]) if i % 2 else (pair[0], -1)
        elif kind == 5:
            pair = pick(~snr[i]) or pair
        else:
            pair = pick(snr[i] & ~xt[i]) or pick(~xt[i]) or pair
        given[i] = pair
    return given


class Seen:
    """What the checked states held, for the preconditions."""

    def __init__(self):
        self.by_occupancy = self.by_reach = self.last_start = self.fallback = self.plain = 0


def _check(env, tab, what, rng, seen):
    avail, services = _state(env)
    n, C, _, S = avail.shape
    pv = rr.prov_all(avail, services, env.topology, tab)
    given = _draw_given(services, tab, rng)
    xt, snr = _reach(services, tab)
    for layout in rr.LAYOUTS:
        g = given if layout == "core_slot" else None
        got = env.action_mask(layout, given=g)
        want = rr.restate_rmcsa_fast(None, None, env.topology, tab, layout, given=g, allow_rejection=env.allow_rejection, pv=pv)
        assert got.shape == want.shape and got.dtype == np.bool_, (what, layout)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "%s, %s: %d envs differ, first %d (given %r)" % (what, layout, len(bad), bad[0], given[bad[0]])
        bare = rr.restate_rmcsa_fast(None, None, env.topology, tab, layout, given=g, allow_rejection=env.allow_rejection, fallback=False, pv=pv)[:, :-1]
        seen.fallback += int((~bare.any(axis=1)).sum())
        seen.plain += int(bare.any(axis=1).sum())
    # what the zeros and ones are made of
    n_of = tab["n_slots"][np.array([tab["rate_index"][int(b)] for b in services[:, 4]])]  # [n, M]
    inside = (np.arange(S)[None, None, :] + n_of[:, :, None]) <= S                        # [n, M, S]
    reach = xt & snr
    seen.by_occupancy += int((~pv & reach[:, :, :, None, None] & inside[:, None, :, None, :]).sum())
    # by reach alone: the slots are free and inside, only the pair's reach says no
    pv_free = rr.prov_all(avail, services, env.topology, dict(tab, lmax_xt=np.full(M, np.inf), lmax_snr=np.full_like(tab["lmax_snr"], np.inf)))
    seen.by_reach += int((pv_free & ~reach[:, :, :, None, None]).sum())
    last = S - n_of                                                                       # [n, M]
    seen.last_start += int(np.take_along_axis(pv, np.broadcast_to(last[:, None, :, None, None], (n, K, M, C, 1)), axis=4).sum())


@pytest.mark.parametrize("name,n_envs,allow_rejection", CASES)
def test_mask_equals_restatement_on_every_env(name, n_envs, allow_rejection):
    case = slot_agent.CASE_BY_NAME[name]
    env = _make(case.kw, n_envs, allow_rejection=allow_rejection)
    assert env.lib.orl_batch_row_words(env._h) == {64: 1, 65: 2, 128: 2, 129: 5, 512: 8}[case.S]
    tab = rr.tables_of(env)
    rng, seen = np.random.default_rng(case.S), Seen()
    _check(env, tab, "after construction", rng, seen)
    _agent_steps(env, tab, 60, np.random.RandomState(case.S))
    _check(env, tab, "after 60 agent steps", rng, seen)
    env.run("SAP_BM_FC_FF", 100)
    _check(env, tab, "after run(SAP_BM_FC_FF, 100)", rng, seen)
    env.reset(full=True)
    _check(env, tab, "after a full reset", rng, seen)
    assert seen.by_occupancy > 0 and seen.by_reach > 0 and seen.last_start > 0 and seen.fallback > 0 and seen.plain > 0, vars(seen)
    env.check()
    env.close()


@pytest.fixture(scope="module")
def topo_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("rmcsa_mask_topologies")


# The cases above all launch 4 wavefronts per workgroup (csrc/orl_view_plan.h: what 48 KiB of LDS rows allow).  Path-modulation keeps
# k + 2 + k C words per env: 64 paths (k6full: 6 nodes, 15 links) with 7 cores leave room for 2 wavefronts, with 11 cores for 1.
# Core-slot keeps 2 W C + 2 words: 31 cores of 512 slots leave room for 2 (and no accepted shape for fewer).
@pytest.mark.parametrize("topo,k,C,S,layout,waves", [("k6full", 64, 7, 64, "path_modulation", 2), ("k6full", 64, 11, 64, "path_modulation", 1),
                                                     ("nsfnet_chen", 5, 31, 512, "core_slot", 2)])
def test_mask_equals_restatement_on_two_and_one_wavefronts(topo, k, C, S, layout, waves, topo_dir):
    import optical_rl_gym_amd as orl
    from tests import envelope
    from tests.helpers import view_plan_of

    n = 24
    kw = dict(slot_agent.CASE_BY_NAME["rmcsa_c7_s64"].kw, num_spatial_resources=C, num_spectrum_resources=S)
    env = orl.make("RMCSA", topology=envelope.topology_npz(topo, k, topo_dir), num_envs=n, seeds=list(range(500, 500 + n)), **kw)
    plan = view_plan_of(env, "rmcsa_mask", env.MASK_LAYOUTS[layout])
    assert plan["ok"] == 1 and plan["waves"] == waves and plan["grid"] == -(-n // (8 * waves)), plan
    tab = rr.tables_of(env)
    n_mod = len(tab["lmax_xt"])
    rng = np.random.default_rng(k + C)
    ones = zeros = 0
    for point in (0, 30, 60):
        if point:
            env.run("SAP_BM_FC_FF", 30)
        avail, services = _state(env)
        pv = rr.prov_all(avail, services, env.topology, tab)
        given = np.stack([rng.integers(-1, k + 1, n), rng.integers(-1, n_mod + 1, n)], axis=1).astype(np.int32)  # (out of range at either end too)
        for lay in rr.LAYOUTS:
            g = given if lay == "core_slot" else None
            got = env.action_mask(lay, given=g)
            want = rr.restate_rmcsa_fast(None, None, env.topology, tab, lay, given=g, allow_rejection=env.allow_rejection, pv=pv)
            assert got.shape == want.shape and got.dtype == np.bool_, (point, lay)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert len(bad) == 0, "after %d steps, %s: %d envs differ, first %d (given %r)" % (point, lay, len(bad), bad[0], given[bad[0]])
            if lay == layout:
                ones += int(got[:, :-1].sum())
                zeros += int((~got[:, :-1]).sum())
    assert ones > 0 and zeros > 0
    env.check()
    env.close()


@pytest.mark.parametrize("allow_rejection", [False, True])
def test_mask_predicts_the_step_of_every_column(allow_rejection):
    C, S, n = 3, 40, 64
    kw = dict(slot_agent.CASE_BY_NAME["rmcsa_c7_s64"].kw, num_spatial_resources=C, num_spectrum_resources=S, allow_rejection=allow_rejection)
    env = _make(kw, n, seed0=77)
    tab = rr.tables_of(env)
    _agent_steps(env, tab, 80, np.random.RandomState(8))
    snap = env.get_state()
    acc0 = env.counters()[:, 1].copy()
    pm = env.action_mask("path_modulation")
    env.action_mask("core_slot", given=np.tile(np.array([K + 2, -3], np.int32), (n, 1)))
    assert np.array_equal(env.get_state(), snap)  # the masks touch neither env state nor flags, whatever the pair
    accepted = np.zeros((n, K, M, C, S), bool)
    for p in range(K):
        for m in range(M):
            given = np.tile(np.array([p, m], np.int32), (n, 1))
            env.set_state(snap)
            cs = env.action_mask("core_slot", given=given)
            assert (cs[:, -1] == allow_rejection).all()
            for col in range(C * S):
                env.set_state(snap)
                env.step(np.tile(np.array([p, m, col // S, col % S], np.int32), (n, 1)))
                accepted[:, p, m, col // S, col % S] = env.counters()[:, 1] - acc0 == 1
            got = accepted[:, p, m].reshape(n, C * S)
            fb = ~got.any(axis=1)
            assert np.array_equal(cs[~fb, :-1], got[~fb]), (p, m)
            assert not cs[fb, :-1].any() if allow_rejection else cs[fb, :-1].all(), (p, m)
    env.set_state(snap)
    stage1 = accepted.any(axis=(3, 4)).reshape(n, K * M)
    fb = ~stage1.any(axis=1)
    assert np.array_equal(pm[~fb, :-1], stage1[~fb])
    assert not pm[fb, :-1].any() if allow_rejection else pm[fb, :-1].all()
    assert (pm[:, -1] == allow_rejection).all()
    assert 0 < fb.sum() < n  # (both kinds of row)
    env.close()


def test_device_path_given_sources_and_graph_capture():
    import torch

    case = slot_agent.CASE_BY_NAME["rmcsa_c7_s65"]
    n = 512
    env = _make(case.kw, n, seed0=31)
    tab = rr.tables_of(env)
    rng = np.random.default_rng(6)
    env.run("SAP_BM_FC_FF", 60)
    given = _draw_given(env.services(), tab, rng)
    # fetch=False and the device views, one per layout
    want_pm = env.action_mask("path_modulation")
    want_cs = env.action_mask("core_slot", given=given)
    acts = env.device_tensor("actions")
    before = acts.cpu().numpy().copy()
    with torch.cuda.stream(env.torch_stream()):
        env.action_mask("core_slot", fetch=False, given=given)
    env.sync()
    cs_view = env.device_tensor("action_mask")
    dim, pitch = env.action_mask_shape("core_slot")
    assert dim == 7 * 65 + 1 and cs_view.shape == (n, dim) and cs_view.dtype == torch.bool and cs_view.stride() == (pitch, 1)
    assert np.array_equal(cs_view.cpu().numpy(), want_cs)
    assert np.array_equal(acts.cpu().numpy(), before)  # a host `given` leaves the actions buffer alone
    env.action_mask("path_modulation", fetch=False)
    env.sync()
    pm_view = env.device_tensor("action_mask")
    assert pm_view.shape == (n, K * M + 1) and np.array_equal(pm_view.cpu().numpy(), want_pm)
    assert np.array_equal(cs_view.cpu().numpy(), want_cs)  # each view keeps showing its own layout
    # given=None: the pairs an agent wrote into columns 0 and 1 of the actions buffer
    other = _draw_given(env.services(), tab, rng)
    with torch.cuda.stream(env.torch_stream()):
        acts[:, :2].copy_(torch.as_tensor(other, dtype=torch.int32, device=acts.device))
        env.action_mask("core_slot", fetch=False)
    env.sync()
    from_actions = cs_view.cpu().numpy().copy()
    assert np.array_equal(from_actions, env.action_mask("core_slot", given=other))
    avail, services = _state(env)
    assert np.array_equal(from_actions, rr.restate_rmcsa_fast(avail, services, env.topology, tab, "core_slot", given=other, allow_rejection=True))
    assert np.array_equal(pm_view.cpu().numpy(), want_pm)
    # one linear chain under capture on the batch's stream (the buffers exist: allocated by the calls above)
    torch.cuda.synchronize()
    s = env.torch_stream()
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        env.action_mask("path_modulation", fetch=False)
        env.action_mask("core_slot", fetch=False)
    torch.cuda.synchronize()
    for _ in range(2):
        env.run("SAP_BM_FC_FF", 25)
        pairs = _draw_given(env.services(), tab, rng)
        with torch.cuda.stream(s):
            acts[:, :2].copy_(torch.as_tensor(pairs, dtype=torch.int32, device=acts.device))
        env.sync()
        g.replay()
        torch.cuda.synchronize()
        avail, services = _state(env)
        pv = rr.prov_all(avail, services, env.topology, tab)
        assert np.array_equal(pm_view.cpu().numpy(), rr.restate_rmcsa_fast(None, None, env.topology, tab, "path_modulation", allow_rejection=True, pv=pv))
        assert np.array_equal(cs_view.cpu().numpy(),
                              rr.restate_rmcsa_fast(None, None, env.topology, tab, "core_slot", given=pairs, allow_rejection=True, pv=pv))
    env.check()
    env.close()


@pytest.mark.parametrize("fam,kw", [("RMSA", dict(load=100, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64)),
                                    ("DeepRMSA", dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=2, episode_length=50)),
                                    ("RWA", dict(load=450, mean_service_holding_time=25, episode_length=1000, allow_rejection=True)),
                                    ("QoSConstrainedRA", dict(load=10))])
def test_other_families_refuse_the_two_stage_layouts(fam, kw):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = orl.make(fam, topology=TOPOLOGY, num_envs=16, seeds=list(range(16)), **kw)
    for layout in rr.LAYOUTS:
        with pytest.raises(OrlError):
            env.action_mask(layout)
        with pytest.raises(OrlError):
            env.action_mask(layout, fetch=False)
        with pytest.raises(OrlError):
            env.action_mask_shape(layout)
    env.close()


def test_given_is_checked():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = _make(dict(load=100, num_spectrum_resources=64, num_spatial_resources=7), 16)
    ok = np.zeros((16, 2), np.int32)
    for bad in (np.zeros((16, 4), np.int32), np.zeros((15, 2), np.int32), np.zeros(32, np.int32), np.zeros((16, 2), np.float64)):
        with pytest.raises(ValueError):
            env.action_mask("core_slot", given=bad)
    with pytest.raises(ValueError):
        env.action_mask("path_modulation", given=ok)
    with pytest.raises(ValueError):
        env.action_mask("joint", given=ok)
    with pytest.raises(OrlError, match="not available.*ORL_MASK_PATH_MOD.*ORL_MASK_CORE_SLOT"):
        env.action_mask("joint")
    assert env.action_mask("core_slot", given=ok).shape == (16, 7 * 64 + 1)
    env.close()
    one = orl.RMCSAEnv(topology=TOPOLOGY, seed=3, load=100, num_spectrum_resources=64, num_spatial_resources=7)
    one.reset()
    pm = one.action_mask("path_modulation")
    cs = one.action_mask("core_slot", given=(0, 0))
    assert pm.shape == (K * M + 1,) and cs.shape == (7 * 64 + 1,) and pm.dtype == np.bool_
    assert np.array_equal(pm, one.batch.action_mask("path_modulation")[0])
    with pytest.raises(ValueError):
        one.action_mask("core_slot", given=(0, 0, 0))
    one.close()


def test_two_stage_masked_agent():
    """Stage 1 uniformly from the path-modulation row, stage 2 uniformly from the core-slot row of the sampled pair: every env-step
    whose rows had a provisioning action provisions, no fallback one does; no action is out of range.  The shares of both kinds
    are those tests/test_rmcsa_mask.py::test_two_stage_masked_agent_over_the_oracle finds on the oracle."""
    env = _make(rr.AGENT_KW, rr.AGENT_ENVS, seeds=rr.AGENT_SEEDS)
    bad_action = []

    def masks(layout, given):
        if layout == "path_modulation":
            bad_action.append(int((env.flags() & 2).sum()))
        return env.action_mask(layout, given=given)

    fallback, accepted = rr.two_stage_walk(env, masks, M)
    assert np.array_equal(accepted, (~fallback).astype(accepted.dtype))
    assert accepted.sum() == (~fallback).sum()
    assert not any(bad_action) and not (env.flags() & 2).any()
    share = fallback.mean()
    print("fallback share %.4f" % share)
    assert 1 - share >= 0.25 and share >= 0.01
    env.check()
    env.close()


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
    given = _draw_given(whole.services(), tab, np.random.default_rng(1))
    for layout in rr.LAYOUTS:
        g = given if layout == "core_slot" else None
        want = whole.action_mask(layout, given=g)
        assert np.array_equal(multi.action_mask(layout, given=g), want), layout
        assert multi.action_mask(layout, fetch=False, given=g) is None
        for s in multi.shards:
            s.sync()
        views = np.concatenate([s.device_tensor("action_mask").cpu().numpy() for s in multi.shards])
        assert np.array_equal(views, want), layout
    with pytest.raises(ValueError):
        multi.action_mask("core_slot", given=given[:cut])
    multi.close()
    whole.close()
