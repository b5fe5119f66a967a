"""The time-scale table (tests/timescale.py) through the real kernels.  The rebuild scan of the soon list (release_soon,
csrc/orl_device_split.h) selects on keys with three absolute constants — a quantum of 1/4096 time unit, a clamp 128 units behind the
clock and a saturation 1 920 units ahead of it — and every other GPU test steps holding times of 5 .. 25.  Here every family runs at
2^k times its base means, for the k that put the holding times, the gaps or both on either side of each constant, and at the
reference's own default of 10 800, through every step route: device-resident runs, host steps and both in turn.  Two references:
the CPU oracle at the same scale (a heap and plain doubles: no time constants), and the k = 0 batch of the one-wavefront kernels
with its times multiplied by 2^k (tests/test_timescale.py proves that lever on the oracle) — which ties the scaled runs to the scale
at which the oracle is pinned to the reference's recorded traces.  Every env is compared after every piece, floats as bit patterns."""
import numpy as np
import pytest

from tests import timescale as ts
from tests.helpers import IMPLS, _exact_bits, force_impl

pytestmark = pytest.mark.gpu

N_ENVS = 128
SAMPLED = (0, 4, 5, 15, 37, 64, 99, 127)
QOS = "QoSConstrainedRA"
RUNS, HOSTS = (1, 3, 8, 13, 5), (4, 2, 9, 1, 3)  # launches that end with fewer than 8 services wanted, host steps between them
MIXED = (0, 7, -12, 20, -30, 9, 6, -7)  # rows of ts.SCALES: env i of a mixed batch runs at the scale of row MIXED[i % 8]


# ---- the oracle behind one interface, whether the batch has one scale or one per env --------------------------------------
class Oracles:
    """envs -> OracleBatch by scale: `cases[i]` is env i's case (an int k or a name of ts.PLAIN); read-backs come back in env order"""

    def __init__(self, fam, cases, kwargs_of=ts.kwargs_of):
        from oracle.oracle import OracleBatch

        seeds = ts.seeds_of(fam, len(cases))
        self.n = len(cases)
        self.groups = []
        for c in dict.fromkeys(cases):
            idx = [i for i in range(self.n) if cases[i] == c]
            self.groups.append((idx, OracleBatch(fam, ts.TOPO, [seeds[i] for i in idx], **kwargs_of(fam, c))))
        self.obs_dim = self.groups[0][1].obs_dim

    def _gather(self, fn):
        out = None
        for idx, o in self.groups:
            v = np.asarray(fn(o))
            if out is None:
                out = np.zeros((self.n,) + v.shape[1:], v.dtype)
            out[idx] = v
        return out

    def __getattr__(self, name):
        if name in ("services", "counters", "active", "slots_packed", "link_stats_all", "net_stats_all", "observation"):
            return lambda: self._gather(lambda o: getattr(o, name)())
        raise AttributeError(name)

    def policy(self, policy):
        return self._gather(lambda o: o.policy(policy))

    def step(self, actions):
        res = [(idx, o.step(np.asarray(actions)[idx], auto_reset=True)) for idx, o in self.groups]
        reward, done = np.zeros(self.n), np.zeros(self.n, np.uint8)
        info = np.zeros((self.n, res[0][1][3].shape[1]))
        for idx, (_o, r, d, i) in res:
            reward[idx], done[idx], info[idx] = r, d, i
        return reward, done, info

    def run(self, policy, n):
        for _idx, o in self.groups:
            o.run(policy, n)

    def one(self, i, name):
        """per-env read-back `name` of env i (QoSConstrainedRA: spectrum, link_stats)"""
        for idx, o in self.groups:
            if i in idx:
                return getattr(o, name)(idx.index(i))
        raise IndexError(i)


# ---- one batch through the sequence ------------------------------------------------------------------------------------------
def snapshot(b, qos, ora=None):
    """What is compared after every piece: counters, pending service, pending releases of every env; slot maps, link and network
    statistics and the observation of every env too (one bulk read-back each) — QoSConstrainedRA, which has no bulk read-backs:
    free units per link, utilisation and last update of the sampled envs."""
    s = {"counters": b.counters(), "services": b.services(), "active": b.active()}
    if qos:
        get = (lambda i, name: getattr(b, name)(i)) if ora is None else ora.one
        s["spectrum"] = np.array([get(i, "spectrum") for i in SAMPLED])
        s["link statistics (qos)"] = np.array([get(i, "link_stats")[[0, 3]] for i in SAMPLED])
    else:
        s["slot maps"] = b.slots_packed()
        s["link statistics"] = b.link_stats_all()
        s["network statistics"] = b.net_stats_all()
        if b.obs_dim:
            s["observation"] = b.observation()
    return {what: np.array(v) for what, v in s.items()}  # copies: a read-back may hand out one buffer again and again


def scaled_snapshot(base, ks):
    """the base scale's snapshot as env i must show it at scale 2^ks[i]"""
    out = {}
    for what, v in base.items():
        v = np.array(v)
        if what in ("reward", "done", "info"):  # [host steps][envs]: no times in them
            out[what] = v
            continue
        rows = SAMPLED if what in ("spectrum", "link statistics (qos)") else range(len(v))
        for r, i in enumerate(rows):
            v[r] = ts.scaled(what, v[r], ks[i])
        out[what] = v
    return out


def drive(fam, cases, make_dev, base=None, tag="", ora_kwargs_of=ts.kwargs_of):
    """The sequence of the crafted-stream tests at the given scales -> the device's snapshot after every piece.  Every piece is
    compared with the oracle, and with `base` (the pieces of the k = 0 batch) scaled where it is given."""
    policy, qos = ts.BASES[fam].policy, fam == QOS
    dev = make_dev()
    ora = Oracles(fam, cases, kwargs_of=ora_kwargs_of)
    ks = [c if not isinstance(c, str) else 0 for c in cases]
    pieces = []

    def piece(label, extra=None):
        chk = _exact_bits("%s %s, %s" % (fam, tag, label))
        snap, ref = snapshot(dev, qos), snapshot(ora, qos, ora)
        snap.update(extra or {})
        for what in ref:
            chk(len(pieces), what, snap[what], ref[what])
        assert not dev.flags().any(), label
        if base is not None:
            exp = scaled_snapshot(base[len(pieces)], ks)
            assert set(exp) == set(snap)
            for what in exp:
                chk(len(pieces), what + " against the base scale", snap[what], exp[what])
        pieces.append(snap)

    def host(n, label):
        chk = _exact_bits("%s %s, %s" % (fam, tag, label))
        rewards, dones, infos = [], [], []
        for t in range(n):
            a = ora.policy(policy)
            _o, r_d, d_d, i_d = dev.step(a, auto_reset=True)
            r_o, d_o, i_o = ora.step(a)
            chk(t, "reward", r_d, r_o)
            chk(t, "done", d_d, d_o)
            chk(t, "info", i_d, i_o)
            chk(t, "services", dev.services(), ora.services())
            rewards.append(np.array(r_d)), dones.append(np.array(d_d)), infos.append(np.array(i_d))
        # (reward and info hold no times: the base scale's, bit for bit)
        piece(label, dict(reward=np.array(rewards), done=np.array(dones), info=np.array(infos)))

    def run(n, label):
        dev.run(policy, n)
        ora.run(policy, n)
        piece(label)

    piece("at construction")
    run(150, "run of 150 steps")
    run(150, "second run of 150 steps")
    host(40, "40 host steps")
    for j, (r, h) in enumerate(zip(RUNS, HOSTS)):
        run(r, "piece %d: run of %d steps" % (j, r))
        host(h, "piece %d: %d host steps" % (j, h))
    state = dev.get_state()

    def tail():
        dev.run(policy, 7)
        for _ in range(3):
            dev.step(dev.policy(policy), auto_reset=True)
        return snapshot(dev, qos)

    first = tail()
    ora.run(policy, 10)
    piece("the tail")
    dev.set_state(state)
    again = tail()
    chk = _exact_bits("%s %s, the tail after set_state" % (fam, tag))
    for what in first:
        chk(0, what, again[what], first[what])
    dev.close()
    return pieces


def _make(fam, case):
    import optical_rl_gym_amd as orl

    return lambda: orl.make(fam, topology=ts.TOPO, num_envs=N_ENVS, seeds=ts.seeds_of(fam, N_ENVS), **ts.kwargs_of(fam, case))


def _force(monkeypatch, fam, route):
    if fam == QOS:  # no persistent kernel serves it: its two step kernels
        monkeypatch.setenv("ORL_AGENT_STEP", "1" if route == "agent8" else "0")
    else:
        force_impl(monkeypatch, route)


_BASE = {}


def base_pieces(fam):
    """the k = 0 batch under the one-wavefront kernels (itself compared with the oracle piece by piece): once per family"""
    if fam not in _BASE:
        with pytest.MonkeyPatch.context() as mp:
            _force(mp, fam, "wave64")
            _BASE[fam] = drive(fam, [0] * N_ENVS, _make(fam, 0), tag="base scale, wave64")
    return _BASE[fam]


# persist_pair builds a specialisation per configuration (~15 s of hipcc): RMSA only, as tests/test_crafted_streams_gpu.py
def _routes(fam):
    if fam == QOS:
        return ["wave64", "agent8"]
    return [r for r in IMPLS if r != "persist_pair" or fam == "RMSA"]


# (the sub-quantum scales run under agent8 first: one launch per step, the rounds of the release loop bounded at 64)
def _order(fam, cases):
    return [(fam, c, r) for c in cases for r in sorted(_routes(fam), key=lambda r: r != "agent8")]


SCALED = [x for f in ts.FAMILIES for x in _order(f, ts.ks_of(f))]
PLAIN_CASES = [x for f in ts.FAMILIES for x in _order(f, ts.PLAIN)]


def _ids(cases):
    return ["%s-%s-%s" % (f, ts.case_id(c), r) for f, c, r in cases]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("fam,k,route", SCALED, ids=_ids(SCALED))
def test_every_route_at_every_scale_matches_the_oracle_and_the_base_scale(fam, k, route, monkeypatch):
    base = base_pieces(fam)
    _force(monkeypatch, fam, route)
    drive(fam, [k] * N_ENVS, _make(fam, k), base=base, tag="2^%d, %s" % (k, route))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("fam,case,route", PLAIN_CASES, ids=_ids(PLAIN_CASES))
def test_every_route_at_a_holding_time_of_10800_matches_the_oracle(fam, case, route, monkeypatch):
    """the reference's constructor defaults untouched (what a bare make() gives), and 10 800 at load 100"""
    _force(monkeypatch, fam, route)
    drive(fam, [case] * N_ENVS, _make(fam, case), tag="%s, %s" % (case, route))


# ---- mixed scales in one wavefront ----------------------------------------------------------------------------------------------
def _mixed_ks(fam, shift=0):
    ks = ts.ks_of(fam)
    return [ks[ts.KS.index(MIXED[(i + shift) % 8])] for i in range(N_ENVS)]


def _make_mixed(fam, ks):
    import optical_rl_gym_amd as orl

    b = ts.BASES[fam]
    mht = [b.h0 * 2.0 ** k for k in ks]
    if fam == "DeepRMSA":
        args = dict(mean_service_holding_time=mht, mean_service_inter_arrival_time=[(b.h0 / b.load) * 2.0 ** k for k in ks])
    else:
        args = dict(load=[b.load] * len(ks), mean_service_holding_time=mht)
    return lambda: orl.make(fam, topology=ts.TOPO, num_envs=len(ks), seeds=ts.seeds_of(fam, len(ks)), **b.kw, **args)


# (QoSConstrainedRA keeps no soon list — a step scans all its pending releases — so nothing couples the envs of a wavefront; it takes
# per-env rates like the others and runs here under its two step kernels)
MIXED_ROUTES = ([(f, r) for f in ts.FAMILIES if f != QOS for r in ("persist", "agent8")] + [("RMSA", "persist_pair")]
                + [(QOS, "wave64"), (QOS, "agent8")])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("fam,route", MIXED_ROUTES, ids=["%s-%s" % fr for fr in MIXED_ROUTES])
def test_mixed_scales_in_one_wavefront(fam, route, monkeypatch):
    """One scale per env (per-env load and holding time), cycling through the table: every group of 8 lanes holds all of them, and
    the synchronised rebuild couples their lists.  Env i must be env i of the uniform batch at its scale: the oracle's, and the
    base scale's times 2^k_i."""
    base = base_pieces(fam)
    _force(monkeypatch, fam, route)
    ks = _mixed_ks(fam)
    assert all(len(set(ks[g:g + 8])) == 8 for g in range(0, N_ENVS, 8))
    drive(fam, ks, _make_mixed(fam, ks), base=base, tag="mixed scales, %s" % route)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("route", ["persist", "agent8", "persist_pair"])
def test_set_load_moves_every_env_to_its_neighbours_scale(route, monkeypatch):
    """set_load in the middle of a run: env i goes on at the scale of env i + 1 — from 2^20 to 2^-30, where the new gaps vanish
    below the clock's last bit, and back up — against the oracle with the same set_load."""
    fam = "RMSA"
    b = ts.BASES[fam]
    force_impl(monkeypatch, route)
    ks, nxt = _mixed_ks(fam), _mixed_ks(fam, 1)
    dev = _make_mixed(fam, ks)()
    ora = Oracles(fam, ks)
    n = [0]

    def compare(label):
        chk = _exact_bits("RMSA set_load, %s, %s" % (route, label))
        snap, ref = snapshot(dev, False), snapshot(ora, False)
        for what in ref:
            chk(n[0], what, snap[what], ref[what])
        assert not dev.flags().any(), label
        n[0] += 1

    def run(steps):
        dev.run(b.policy, steps)
        ora.run(b.policy, steps)
        compare("run of %d steps" % steps)

    def host(steps):
        chk = _exact_bits("RMSA set_load, %s, host steps" % route)
        for t in range(steps):
            a = ora.policy(b.policy)
            _o, r_d, d_d, _i = dev.step(a, auto_reset=True)
            r_o, d_o, _i = ora.step(a)
            chk(t, "reward", r_d, r_o)
            chk(t, "done", d_d, d_o)
        compare("%d host steps" % steps)

    run(150)
    dev.set_load(mean_service_holding_time=[b.h0 * 2.0 ** k for k in nxt])
    for idx, o in ora.groups:
        o.set_load(mean_service_holding_time=b.h0 * 2.0 ** nxt[idx[0]])
    compare("set_load")
    run(13)
    host(20)
    run(150)
    host(5)
    dev.close()


# ---- the list-overflow regime at size -----------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("mht", [10800.0, 25.0 * 2.0 ** 9], ids=["h10800", "h25x2^9"])
def test_list_overflow_regime_at_size_every_env_matches_oracle(mht):
    """The RMSA shape of the headline benchmark (320 slots, load 300) at holding times far beyond the saturation: 4 096 envs, 600
    steps of the device-resident loop on the library's own route, every env against the OpenMP oracle."""
    import optical_rl_gym_amd as orl
    from bench import WORKLOADS
    from oracle.oracle import OracleBatch

    fam, topo, kw, policy = WORKLOADS["cfg2"]
    kw = dict(kw, episode_length=100, mean_service_holding_time=mht)
    assert kw["load"] == 300 and kw["num_spectrum_resources"] == 320
    seeds = [10 + i for i in range(4096)]
    dev = orl.make(fam, topology=topo, num_envs=len(seeds), seeds=seeds, **kw)
    dev.run(policy, 600)
    ora = OracleBatch(fam, topo, seeds, omp=True, **kw)
    ora.run(policy, 600)
    chk = _exact_bits("cfg2 shape at a holding time of %g, every env" % mht)
    for what in ("counters", "services", "active", "slots_packed", "link_stats_all", "net_stats_all"):
        chk(600, what, getattr(dev, what)(), getattr(ora, what)())
    assert ora.active().min() >= 48
    assert not dev.flags().any()
    dev.close()
