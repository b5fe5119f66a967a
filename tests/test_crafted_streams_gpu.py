"""Crafted generator states (tests/mt_craft.py) through the real kernels: batches of 128 envs constructed with mt_state= — indices
spread over 0 .. 624 (k_init_mt's loop over the words CPython has already handed out), and in every env one crafted event in a
service 1 .. 24: a run of 40 rejected randint words (a service of 49 words: the look-ahead of the persistent kernel gets batches
that end early), or random() == 0 / 1 - 2^-53 in a time draw (-0.0 times) — stepped by the host, by device-resident runs cut so
that launches end with fewer than 8 services wanted, and by both in turn, through every step route, against the CPU oracle
constructed from the same states (which tests/test_mt_craft.py compares with CPython itself).  Every env is compared after every
piece; floats as bit patterns."""
import functools

import numpy as np
import pytest

from tests import mt_craft as mc
from tests.helpers import IMPLS, _exact_bits, force_impl

N_ENVS = 128
TOPO, N_NODES = "nsfnet_chen", 14
_RMSA = dict(mean_service_holding_time=25, load=100, episode_length=100, allow_rejection=True)
CONFIGS = {
    "rmsa_25_100": ("RMSA", dict(_RMSA, bit_rate_lower_bound=25, bit_rate_higher_bound=100), "SAP_FF"),
    "rmsa_25_88": ("RMSA", dict(_RMSA, bit_rate_lower_bound=25, bit_rate_higher_bound=88), "SAP_FF"),
    "rmsa_25_89": ("RMSA", dict(_RMSA, bit_rate_lower_bound=25, bit_rate_higher_bound=89), "SAP_FF"),
    "rmsa_40_40": ("RMSA", dict(_RMSA, bit_rate_lower_bound=40, bit_rate_higher_bound=40), "SAP_FF"),
    "rmsa_discrete": ("RMSA", dict(_RMSA, num_spectrum_resources=64, bit_rate_selection="discrete"), "SAP_FF"),
    "deeprmsa_j2": ("DeepRMSA", dict(j=2, episode_length=50), "SAP"),
    "rmcsa": ("RMCSA", dict(mean_service_holding_time=25, load=180, episode_length=100, num_spectrum_resources=64, num_spatial_resources=7,
                            worst_xt=-84.7, allow_rejection=True), "SAP_BM_FC_FF"),
    "rwa": ("RWA", dict(mean_service_holding_time=25, load=300, episode_length=200, allow_rejection=True), "SAP_FF"),
    "qos": ("QoSConstrainedRA", dict(mean_service_holding_time=25, load=700, episode_length=200, num_spectrum_resources=40, num_service_classes=3,
                                     classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0], allow_rejection=True), "SAP_FF"),
}
HOST_STEPS = 30
SAMPLED = (0, 4, 5, 15, 37, 64, 99, 127)
# persist_pair builds a specialisation per configuration (~15 s of hipcc): one configuration only
ROUTES = [(c, r) for c in CONFIGS if c != "qos" for r in IMPLS if r != "persist_pair"] + [("rmsa_25_88", "persist_pair")]


@functools.lru_cache(maxsize=None)
def crafted(config):
    fam, kw, _policy = CONFIGS[config]
    cfg = mc.traffic_cfg(fam, N_NODES, **kw)
    states, info = mc.crafted_batch(N_ENVS, fam, cfg)
    states.setflags(write=False)
    return states, info, cfg


def test_crafted_batches_hold_what_the_tests_rely_on():
    """(runs without a device) every index class, every kind of event, and every env's crafted words inside the first HOST_STEPS
    services — consumed by the service they were placed in"""
    for config, (fam, _kw, _p) in CONFIGS.items():
        states, info, cfg = crafted(config)
        assert {0, 1, 227, 397, 623, 624} <= {d["p"] for d in info} and len({d["p"] for d in info}) > 100
        assert [int(s[624]) for s in states] == [d["p"] for d in info]
        kinds = {d["kind"] for d in info}
        assert ("reject_run" in kinds) == mc.seeks(fam, cfg) and {"iat_zero", "ht_zero", "iat_max", "ht_max", "both_zero"} <= kinds
        assert {d["s"] for d in info} >= set(range(1, 25))
        for i, d in enumerate(info):
            w = mc.draw_services(mc.py_rng(states[i]), fam, cfg, d["s"] + 1)["words"]
            assert 1 <= d["s"] < HOST_STEPS and w[d["s"] - 1] <= d["first"] and d["last"] < w[d["s"]], (config, i, d)
        for stop in (1, 4, 12):  # where the runs of "runs_first" stop, a service with a holding time of -0.0 is pending in some env
            assert any(d["s"] == stop and d["kind"] in ("ht_zero", "both_zero") for d in info), (config, stop)


class Pair:
    def __init__(self, config, states=None, **extra):
        import optical_rl_gym_amd as orl
        from oracle.oracle import OracleBatch

        self.fam, kw, self.policy = CONFIGS[config]
        self.states = crafted(config)[0] if states is None else states
        self.qos = self.fam == "QoSConstrainedRA"
        self.dev = orl.make(self.fam, topology=TOPO, num_envs=len(self.states), mt_state=self.states, **kw, **extra)
        assert self.dev.seeds == [None] * len(self.states)
        self.ora = OracleBatch(self.fam, TOPO, mt_state=np.array(self.states), **kw)
        self.tag = config

    def host(self, n):
        chk = _exact_bits(self.tag)
        for t in range(n):
            a = self.ora.policy(self.policy)
            _o, r_d, d_d, _i = self.dev.step(a, auto_reset=True)
            _o, r_o, d_o, _i = self.ora.step(a, auto_reset=True)
            chk(t, "reward", r_d, r_o)
            chk(t, "done", d_d, d_o)
            chk(t, "services", self.dev.services(), self.ora.services())  # (a time of -0.0 shows only while its service is pending)

    def run(self, n):
        st = self.dev.run(self.policy, n)
        self.ora.run(self.policy, n)
        return st

    def compare(self, what, envs=None):
        dev, ora = self.dev, self.ora
        chk = _exact_bits("%s, %s" % (self.tag, what))
        sel = slice(None) if envs is None else envs
        chk(0, "services", dev.services()[sel], ora.services()[sel])
        chk(0, "counters", dev.counters()[sel], ora.counters()[sel])
        chk(0, "active", dev.active()[sel], ora.active()[sel])
        for i in SAMPLED:
            if envs is not None and i not in envs:
                continue
            if self.qos:
                chk(i, "spectrum", dev.spectrum(i), ora.spectrum(i))
                chk(i, "link statistics", dev.link_stats(i)[[0, 3]], ora.link_stats(i)[[0, 3]])
            else:
                chk(i, "slots", dev.slots(i), ora.slots(i))
                chk(i, "link statistics", dev.link_stats(i), ora.link_stats(i))
        if envs is None:
            assert not dev.flags().any()

    def tail(self):
        self.dev.run(self.policy, 7)
        for _ in range(3):
            self.dev.step(self.dev.policy(self.policy), auto_reset=True)
        d = self.dev
        return [mc.bits(d.services()), d.counters(), d.active()] + ([] if self.qos else [d.slots_packed(), mc.bits(d.link_stats_all())])


def _sequence(p, order):
    """order "host_first": the crafted services (1 .. 24) are drawn by host steps, the runs go on from there; "runs_first": they are
    drawn by the device-resident runs, which stop — and are compared — after 1, 4, 12, 25 and 30 steps, each time with the crafted
    service of some envs pending."""
    p.compare("at construction")
    runs = (1, 3, 8, 13, 5)  # launches that end with fewer than 8 services wanted; parked services are picked up again
    assert sum(runs) == HOST_STEPS

    def host_piece():
        p.host(HOST_STEPS)
        p.compare("%d host steps" % HOST_STEPS)

    def run_pieces():
        for n in runs:
            p.run(n)
            p.compare("a run of %d steps" % n)

    for piece in ((host_piece, run_pieces) if order == "host_first" else (run_pieces, host_piece)):
        piece()
    for k, n in enumerate((4, 2, 9, 1, 3)):  # runs and host steps in turn
        (p.run if k % 2 == 0 else p.host)(n)
        p.compare("run / step alternated, piece %d" % k)
    snap = p.dev.get_state()
    first = p.tail()
    p.ora.run(p.policy, 10)
    p.compare("the tail")
    p.dev.set_state(snap)
    again = p.tail()
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    p.dev.close()


ORDERS = ["host_first", "runs_first"]


@pytest.mark.gpu
@pytest.mark.parametrize("config,route", ROUTES, ids=["%s-%s" % cr for cr in ROUTES])
@pytest.mark.parametrize("order", ORDERS)
def test_crafted_states_through_every_step_route(config, route, order, monkeypatch):
    force_impl(monkeypatch, route)
    _sequence(Pair(config), order)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["wave64", "agent8"])
@pytest.mark.parametrize("order", ORDERS)
def test_crafted_states_qos(kernel, order, monkeypatch):
    monkeypatch.setenv("ORL_AGENT_STEP", "1" if kernel == "agent8" else "0")
    _sequence(Pair("qos"), order)


# ---- the look-ahead window that holds not even one service -------------------------------------------------------------------------
def _overflow_states():
    """the batch of rmsa_25_100 with env 5 replaced: 100 rejected randint words behind the 8 fixed words of its service 3"""
    states, _info, cfg = crafted("rmsa_25_100")
    states = np.array(states)
    rn = cfg["hi"] + 1 - cfg["lo"]
    rb = mc.rand_bits_of(rn)
    base = mc.craft(300, [], 777)
    start = int(mc.draw_services(mc.py_rng(base), "RMSA", cfg, 3)["words"][2])
    outs = [mc.reject_word(rn, rb, k, low=k) for k in range(100)] + [mc.accept_word(rn, rb, 33)]
    states[5] = mc.craft(300, outs, 777, at=start + 8)
    w = mc.draw_services(mc.py_rng(states[5]), "RMSA", cfg, 5)["words"]
    assert w[2] == start and w[3] - w[2] == 8 + 100 + 1
    return states


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["wave64", "agent8"])
def test_a_service_longer_than_the_window_is_drawn_by_the_host_stepped_routes(route, monkeypatch):
    """their rejection loop has no window: the service of 109 words is produced like any other"""
    force_impl(monkeypatch, route)
    p = Pair("rmsa_25_100", states=_overflow_states())
    p.host(12)
    p.compare("12 host steps")
    p.dev.close()


@pytest.mark.gpu
def test_a_service_longer_than_the_window_is_reported_by_the_persistent_kernel(monkeypatch):
    """svc_generate cannot produce a service that does not fit its 96-word window: the env is flagged and the run reports it the way
    it reports an env that ran out of pending-release slots (OverflowError, sticky; flag bit 0) — the other 127 envs go on, equal
    to the oracle."""
    force_impl(monkeypatch, "persist")
    p = Pair("rmsa_25_100", states=_overflow_states())
    with pytest.raises(OverflowError):
        p.dev.run(p.policy, 20)
    p.ora.run(p.policy, 20)
    flags = p.dev.flags()
    assert flags[5] & 1 and not (np.delete(flags, 5) & 1).any()
    with pytest.raises(OverflowError):
        p.dev.check()
    p.compare("the other envs", envs=[i for i in range(N_ENVS) if i != 5])
    p.dev.close()


@pytest.mark.gpu
def test_mt_state_reaches_the_shards_of_a_multi_device_batch():
    """MultiDeviceBatch hands each shard its rows of mt_state: two shards on one device, cut inside a group of 8, against the oracle
    over the steps that draw the crafted services."""
    import optical_rl_gym_amd as orl
    from oracle.oracle import OracleBatch

    fam, kw, policy = CONFIGS["rmsa_25_100"]
    states = np.array(crafted("rmsa_25_100")[0][:44])
    multi = orl.make(fam, topology=TOPO, num_envs=44, device_ids=[0, 0], mt_state=states, **kw)
    ora = OracleBatch(fam, TOPO, mt_state=states, **kw)
    chk = _exact_bits("sharded")
    for t in range(HOST_STEPS):
        chk(t, "services", multi.services(), ora.services())
        a = ora.policy(policy)
        _o, r_d, _d, _i = multi.step(a, auto_reset=True)
        _o, r_o, _d, _i = ora.step(a, auto_reset=True)
        chk(t, "reward", r_d, r_o)
    chk(HOST_STEPS, "counters", multi.counters(), ora.counters())
    with pytest.raises(ValueError):
        orl.make(fam, topology=TOPO, num_envs=44, seeds=list(range(44)), mt_state=states, **kw)
    multi.close()
