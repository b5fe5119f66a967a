"""Routing rules and the per-path assignment table on the device (include/orl.h, orl_batch_route_spectrum; k_route_spectrum in
csrc/orl_route.h) against the restatement (tests/route_restate.py, pinned to the reference, to the restatement of assign_spectrum,
to brute-force loops and to the oracle's step in tests/test_route_spectrum.py): every env, every rule x route, actions and table;
device against device with assign_spectrum; against the step itself; under graph capture; over a sharded batch; refusals.

Cases: the nine shapes of tests/assign_cases.py (W = 1, 2, 5, 8, RWA, 88 links, services of up to 33 slots) and five of
tests/envelope.py — k = 9 (a second chunk holding one path), k = 64 (eight chunks), n_paths = 1 < k on 128 links (table rows of missing
paths), 30-hop paths (every plane of the cut counts), services of 64 slots (the whole-word shift)."""
import numpy as np
import pytest

from tests import assign_cases as ac
from tests import assign_restate as ar
from tests import envelope
from tests import route_cases as rc
from tests import route_restate as rr
from tests.oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

ENVELOPE = ("ring10c8_k9_rmsa", "k6full_k64_rwa", "star129_rmsa", "ring31_rmsa", "s512_w64_rmsa")
NAMES = [s.name for s in ac.SHAPES] + list(ENVELOPE)
PAIRS = [(rule, route) for rule in rr.RULES for route in rr.ROUTES]


class Case:
    def __init__(self, name, topo_dir):
        self.name = name
        self.shape = ac.SHAPE_BY_NAME.get(name)
        if self.shape is not None:
            s = self.shape
            self.fam, self.topology, self.k, self.S, self.kw, self.okw = s.fam, s.topology, ac.K, s.S, s.kw, s.kw
            self.seeds, self.warm, self.topo = ac.seeds_of(s), 0, ac.topology(s.topology)
        else:
            c = envelope.CASE_BY_NAME[name]
            assert c.batch <= 64
            self.fam, self.k, self.S, self.kw, self.okw = c.fam, c.k, c.kw["num_spectrum_resources"], c.kw, envelope.oracle_kwargs(c)
            self.topology = envelope.topology_npz(c.topo, c.k, topo_dir)
            self.seeds, self.warm, self.topo = envelope.seeds_of(c), c.warm, envelope.topology_of(self.topology)

    def make(self, seeds=None):
        import optical_rl_gym_amd as orl

        seeds = self.seeds if seeds is None else seeds
        return orl.make(self.fam, topology=self.topology, num_envs=len(seeds), seeds=seeds, **self.kw)

    def oracle(self, seeds=None):
        return OracleBackend(self.fam, self.topology, self.seeds if seeds is None else seeds, **self.okw)

    def state(self, env):
        return ar.unpack_slots(env.slots_packed(), self.topo.n_links, self.S, ar.row_words(self.S)), env.services().copy()

    def expected(self, avail, services, seen=None):
        return rc.expected(self.fam, self.topo, self.k, self.S, avail, services, seen)

    def walk(self, env):
        """The state the checks want after construction: the agent's steps, or the case's warm-up run()"""
        if self.shape is not None:
            ac.agent_steps(env, self.shape, ac.AGENT_STEPS, np.random.RandomState(self.S))
        else:
            env.run("SAP_FF", self.warm)


@pytest.fixture(scope="module")
def topo_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("route_topologies")


def _rows(got, want, what):
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape, got.dtype)
    bad = np.flatnonzero((got.reshape(len(got), -1) != want.reshape(len(want), -1)).any(axis=1))
    assert len(bad) == 0, "%s: %d envs differ, first %d: got %r, want %r" % (what, len(bad), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())


def _check(case, env, what, seen, in_place=False):
    """Every env, every rule x route, actions and table against the restatement, with no state byte or flag changed; then device
    against device: route ksp = assign_spectrum, table column 0 of row p = assign_spectrum on path p.  in_place: read through
    fetch=False and the device tensors on the batch's stream instead."""
    import torch

    avail, services = case.state(env)
    exp = case.expected(avail, services, seen)
    snap, flags = env.get_state(), env.flags().copy()
    n, k, S = len(services), case.k, case.S
    for rule, route in PAIRS:
        tab_want, acts_want = exp[rule][0], exp[rule][1][route]
        if in_place:
            with torch.cuda.stream(env.torch_stream()):
                env.device_tensor("actions").fill_(-7)
                env.device_tensor("assign_table").fill_(-7)
                assert env.route_spectrum(rule, route, fetch=False) is None
            env.sync()
            acts, tab = env.device_tensor("actions").cpu().numpy(), env.device_tensor("assign_table").cpu().numpy()
            assert tab.shape == (n, 4 * k)
            tab = tab.reshape(n, k, 4)
        else:
            acts, tab = env.route_spectrum(rule, route, table=True)
            _rows(env.route_spectrum(rule, route), acts_want, "%s, %s, %s, actions alone" % (what, rule, route))
        _rows(acts, acts_want, "%s, %s, %s, actions" % (what, rule, route))
        _rows(tab, tab_want, "%s, %s, %s, table" % (what, rule, route))
    for rule in ar.RULES:  # device against device
        acts, tab = env.route_spectrum(rule, "ksp", table=True)
        _rows(acts, env.assign_spectrum(rule), "%s, %s: route ksp against assign_spectrum" % (what, rule))
        for p in range(k):
            on_p = env.assign_spectrum(rule, paths=np.full(n, p, np.int32))
            assert np.array_equal(tab[:, p, 0], np.where(on_p[:, 0] == k, S, on_p[:, 1])), (what, rule, p)
        seen["device_pairs"] = seen.get("device_pairs", 0) + 1
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.flags(), flags), what
    return exp


_WALKS = {}


def _walk(name, topo_dir):
    if name in _WALKS:
        return _WALKS[name]
    case = Case(name, topo_dir)
    env = case.make()
    assert env.lib.orl_batch_row_words(env._h) == ar.row_words(case.S)
    assert env.assign_table_shape() == (case.k, 4, 4 * case.k)
    from optical_rl_gym_amd._lib import OrlError

    with pytest.raises(OrlError, match="call route_spectrum"):
        env.device_tensor("assign_table")
    seen = {}
    _check(case, env, "after construction", seen)
    case.walk(env)
    _check(case, env, "after the walk", seen)
    # crowded / crafted maps under the same pending services, through a snapshot (no step follows: the snapshot is put back)
    snap = env.get_state()
    avail, services = case.state(env)
    maps = [rc.craft(case.fam, case.topo, case.k, case.S, avail, services)]
    if case.shape is not None:
        maps.insert(0, ac.crowd(case.shape, avail, services))
    for m in maps:
        ac.set_maps(env, snap, m)
        assert np.array_equal(case.state(env)[0], m)
        exp = _check(case, env, "on crowded / crafted maps", seen, in_place=True)
    seen["cuts_max"] = int(max(c for c in exp["min_cuts"][0][:, :, 1].ravel() if c != rr.NO_FIT))
    seen["widest"] = int(exp["first"][0][:, :, 2].max())
    seen["missing_rows"] = int((exp["first"][0][:, :, 2] == 0).sum())
    env.set_state(snap)
    env.reset(full=True)
    _check(case, env, "after a full reset", seen)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()
    _WALKS[name] = seen
    return seen


@pytest.mark.parametrize("name", NAMES)
def test_actions_and_table_equal_restatement_on_every_env(name, topo_dir):
    """After construction, after the walk, on crowded and crafted maps (there read in place after fetch=False) and after a full
    reset.  What the states hold is printed; tests/test_route_spectrum.py establishes the kinds per family on the oracle."""
    seen = _walk(name, topo_dir)
    print(name, seen)
    assert seen["cuts_zero"] > 0 and seen["min_cuts_at_0"] > 0 and seen["min_cuts_at_top"] > 0 and seen["cuts_max"] >= 1, seen  # (the crafted maps)
    if name == "rmsa_nsf_s65":  # 512 envs, walked on the oracle too: every kind in one shape
        missing = [kd for kd in rr.RMSA_KINDS if seen.get(kd, 0) == 0]
        assert not missing, (missing, seen)
    if name == "star129_rmsa":
        assert seen["missing_rows"] > 0, seen  # n_paths = 1 < k
    if name == "ring31_rmsa":
        assert seen["cuts_max"] >= 16, seen  # the top plane of the counts
    if name == "s512_w64_rmsa":
        assert seen["widest"] == 64, seen  # the whole-word shift


@pytest.mark.parametrize("name", NAMES)
def test_route_ksp_is_assign_spectrum_and_the_table_its_answer_per_path(name, topo_dir):
    """Device against device, on the states of the test above (the comparison runs with them)."""
    assert _walk(name, topo_dir)["device_pairs"] >= 6 * 4


def _compare(env, ora, what):
    assert np.array_equal(env.counters(), ora.counters()), what
    assert np.array_equal(env.services(), ora.services()), what
    assert np.array_equal(env.slots_packed(), ora.slots_packed()), what


def _pair(case, seeds):
    env, ora = case.make(seeds), case.oracle(seeds)
    if case.warm:
        env.run("SAP_FF", case.warm)
        ora.run("SAP_FF", case.warm)
        _compare(env, ora, "warm-up")
    return env, ora


def _want(case, ora, rule, route):
    avail, services = case.state(ora)
    prep, links = rc.prepared(case.fam, case.topo, case.k, case.S, avail, services)
    return rr.route(rr.table(prep, links, rule), route, case.k, case.S)


@pytest.mark.parametrize("name", [s.name for s in ac.SHAPES if s.envs <= 24] + ["s512_w64_rmsa"])
def test_route_then_step_equals_the_oracle_stepped_with_the_restatement(name, topo_dir):
    """route_spectrum(fetch=False); step(None) for 60 steps, rule and route changing with the step, against an oracle env stepped
    with the restated action: reward, done, counters, slot maps and services of every env at every step."""
    case = Case(name, topo_dir)
    assert len(case.seeds) <= 24
    env, ora = _pair(case, case.seeds)
    provisioned = 0
    for t in range(60):
        rule, route = rr.RULES[t % 7], rr.ROUTES[(t // 7 + t) % 3]
        want = _want(case, ora, rule, route)
        assert env.route_spectrum(rule, route, fetch=False) is None
        _, r_d, d_d, _ = env.step(None, auto_reset=True)
        _, r_o, d_o, _ = ora.step(want, auto_reset=True)
        assert np.array_equal(r_d, r_o) and np.array_equal(d_d, d_o), (t, rule, route)
        _compare(env, ora, (t, rule, route))
        provisioned += int((want[:, 0] < case.k).sum())
    assert provisioned > 0 and not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("name", NAMES)
def test_captured_route_and_step(name, topo_dir):
    """One single-stream graph of {route_spectrum(fetch=False); step(None)}: 20 replays against the oracle stepped with the
    restated action (the 512-env shapes at 64 envs: the oracle and the restatement run per replay)."""
    import torch

    case = Case(name, topo_dir)
    rule, route = PAIRS[(5 * NAMES.index(name) + 3) % len(PAIRS)]
    env, ora = _pair(case, case.seeds[:64])
    acts, s = env.device_tensor("actions"), env.torch_stream()
    rew, done = env.device_tensor("reward"), env.device_tensor("done")

    def oracle_step(want, what):
        _, r, d, _ = ora.step(want, auto_reset=True)
        assert np.array_equal(rew.cpu().numpy(), r) and np.array_equal(done.cpu().numpy().astype(bool), np.asarray(d).astype(bool)), what
        assert np.array_equal(acts.cpu().numpy(), want), what
        _compare(env, ora, what)

    want = _want(case, ora, rule, route)  # (the first call comes before the capture: the table is allocated outside)
    with torch.cuda.stream(s):
        env.route_spectrum(rule, route, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    torch.cuda.synchronize()
    oracle_step(want, "eager")
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        env.route_spectrum(rule, route, fetch=False)
        env.step(None, auto_reset=True, fetch=False)
    torch.cuda.synchronize()
    for it in range(20):
        want = _want(case, ora, rule, route)
        g.replay()
        torch.cuda.synchronize()
        oracle_step(want, "replay %d" % it)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


def test_two_shards_equal_the_unsharded_batch(topo_dir):
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    case = Case("rmsa_nsf_s65", topo_dir)
    n, cut = 200, 72
    seeds = list(range(40, 40 + n))
    whole = case.make(seeds)
    multi = MultiDeviceBatch.from_shards([case.make(seeds[:cut]), case.make(seeds[cut:])])
    for t in range(20):
        a = whole.policy("SAP_FF").copy()
        whole.step(a, auto_reset=True)
        multi.step(a, auto_reset=True)
    assert multi.assign_table_shape() == whole.assign_table_shape()
    exp = case.expected(*case.state(whole))
    for rule, route in (("best", "best"), ("most_used", "least_loaded"), ("min_cuts", "best")):
        acts, tab = whole.route_spectrum(rule, route, table=True)
        _rows(acts, exp[rule][1][route], (rule, route))
        _rows(tab, exp[rule][0], (rule, route))
        got = multi.route_spectrum(rule, route, table=True)
        assert np.array_equal(got[0], acts) and np.array_equal(got[1], tab), (rule, route)
        assert np.array_equal(multi.route_spectrum(rule, route), acts), (rule, route)
        assert multi.route_spectrum(rule, route, fetch=False) is None
        for sh in multi.shards:
            sh.sync()
        assert np.array_equal(np.concatenate([sh.device_tensor("actions").cpu().numpy() for sh in multi.shards]), acts), (rule, route)
        assert np.array_equal(np.concatenate([sh.device_tensor("assign_table").cpu().numpy() for sh in multi.shards]).reshape(n, ac.K, 4), tab)
    multi.close()
    whole.close()


@pytest.mark.parametrize("fam,kw", [("DeepRMSA", dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=2, episode_length=50)),
                                    ("RMCSA", dict(load=100, num_spectrum_resources=64, num_spatial_resources=7)),
                                    ("QoSConstrainedRA", dict(load=10))])
def test_other_families_refuse_the_routes(fam, kw):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    env = orl.make(fam, topology="nsfnet_chen", num_envs=16, seeds=list(range(16)), **kw)
    snap = env.get_state()
    acts = env.device_tensor("actions").cpu().numpy().copy()
    for fetch in (True, False):
        for rule, route in PAIRS:
            with pytest.raises(OrlError, match="RMSA and RWA only"):
                env.route_spectrum(rule, route, fetch=fetch)
    with pytest.raises(OrlError, match="RMSA and RWA only"):
        env.assign_table_shape()
    with pytest.raises(OrlError, match="call route_spectrum"):
        env.device_tensor("assign_table")
    env.sync()
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    env.reset(full=True)  # (still usable)
    env.check()
    env.close()


def test_arguments_are_checked(topo_dir):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    case = Case("rmsa_nsf_s64", topo_dir)
    env = case.make(list(range(16)))
    with pytest.raises(OrlError, match="call route_spectrum"):
        env.device_array("assign_table")
    env.assign_spectrum()
    acts = env.device_tensor("actions").cpu().numpy().copy()
    for fetch in (True, False):
        for rule in (-1, 7):
            with pytest.raises(OrlError, match=r"unknown spectrum-assignment rule .*0 \.\. 6"):
                env.route_spectrum(rule, "ksp", fetch=fetch)
        for route in (-1, 3):
            with pytest.raises(OrlError, match=r"unknown route .*0 \.\. 2"):
                env.route_spectrum("first", route, fetch=fetch)
    for bad in (("worst", "ksp"), ("first", "shortest")):
        with pytest.raises(ValueError):
            env.route_spectrum(*bad)
    with pytest.raises(OrlError, match="unknown spectrum-assignment rule"):
        env.assign_spectrum(6)  # (min_cuts is the route call's alone)
    with pytest.raises(OrlError, match="call route_spectrum"):
        env.device_array("assign_table")  # (a refused call allocates nothing)
    env.sync()
    assert np.array_equal(env.device_tensor("actions").cpu().numpy(), acts)  # nothing was queued
    assert env.route_spectrum(6, 2).shape == (16, 4) and env.device_tensor("assign_table").shape == (16, 4 * ac.K)
    env.step(None, auto_reset=True)  # (still usable)
    env.check()
    env.close()
    for cls, kw in ((orl.RMSAEnv, dict(load=100, num_spectrum_resources=64)), (orl.RWAEnv, dict(load=100, num_spectrum_resources=64))):
        one = cls(topology="nsfnet_chen", seed=3, **kw)
        one.reset()
        got = one.route_spectrum("min_cuts", "least_loaded")
        assert isinstance(got, tuple) and len(got) == 2 and all(isinstance(v, int) for v in got)
        assert got == tuple(int(v) for v in one.batch.route_spectrum("min_cuts", "least_loaded")[0][:2]) and got != (ac.K, 64)
        assert one.route_spectrum("first", "ksp") == one.assign_spectrum("first")
        one.close()
