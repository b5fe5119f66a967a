"""copy_envs on the device (include/orl.h, orl_batch_copy_envs; k_copy_envs in csrc/orl_copy.h): env dst[p] of one batch becomes a copy
of env src[p] of another batch or of the same one.

1. every section row of a snapshot, byte for byte, and untouched neighbours, on every family;
2. the copy continues as its source under every step route;
3. ... and as the CPU oracle seeded with the source's seed does;
4. in place, a whole group of 8 envs;
5. reseeded batches (second streams), and the refusal between a reseeded and a fresh batch;
6. keep_rng: the source's network state on the destination's own streams;
7. ordering with the source's stream, no host synchronisation in between;
8. refusals leave everything as it was;
9. MultiDeviceBatch;
10. the full-size batch.

Batches of 67 envs: not a multiple of 8, the group of envs one wavefront of the 8-lanes-per-env kernels owns.  Every comparison is
exact, floats as bit patterns."""
import os

import numpy as np
import pytest

from tests.helpers import IMPLS, _exact_bits, force_impl
from tests.test_gpu_parity import _need_devices

pytestmark = pytest.mark.gpu

N = 67
SRC = np.array([0, 66, 5, 5, 5, 33])
DST = np.array([66, 0, 6, 7, 8, 33])
SEC_SCAL, SEC_MT = 0, 5  # sections of the snapshot (state_layout): the scalar record, the random stream
ORL_FLAG_MT2 = 4

# (family, kwargs, heuristic).  The configurations of the step-route test are the benchmark's (bench.py): the two-wavefront form of
# the persistent kernel exists in specialisation libraries only, which the build makes for these.
CFG = {
    "rmsa": ("RMSA", dict(load=300, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=320, allow_rejection=False), "SAP_FF"),
    "deeprmsa": ("DeepRMSA", dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=1, episode_length=50), "SAP"),
    "deeprmsa_j3": ("DeepRMSA", dict(mean_service_holding_time=7.5, mean_service_inter_arrival_time=1.0 / 12.0, j=3, episode_length=50,
                                      allow_rejection=True), "SAP"),
    "rwa": ("RWA", dict(load=450, mean_service_holding_time=25, episode_length=200, allow_rejection=True), "SAP_FF"),
    "rmcsa": ("RMCSA", dict(load=1500, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=320, num_spatial_resources=7,
                            allow_rejection=True), "SAP_BM_FC_FF"),
    "rmcsa_hist": ("RMCSA", dict(load=250, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64, num_spatial_resources=7,
                                 allow_rejection=True, action_histograms=True), "SAP_BM_FC_FF"),
    "qos": ("QoSConstrainedRA", dict(load=1000, mean_service_holding_time=25, episode_length=200, num_spectrum_resources=40,
                                     num_service_classes=3, classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0],
                                     allow_rejection=True), "SAP_FF"),
    "rmsa_discrete": ("RMSA", dict(load=50, mean_service_holding_time=25, episode_length=100, num_spectrum_resources=64, allow_rejection=True,
                                   bit_rate_selection="discrete"), "SAP_FF"),
    "rmsa_tiny5": ("RMSA", dict(load=10, mean_service_holding_time=25, episode_length=50, num_spectrum_resources=64), "SAP_FF"),
}


def _make(name, n=N, seed0=1000, **extra):
    import optical_rl_gym_amd as orl

    fam, kw, _pol = CFG[name]
    topo = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny5_k3.npz") if name == "rmsa_tiny5" else "nsfnet_chen"
    return orl.make(fam, topology=topo, num_envs=n, seeds=list(range(seed0, seed0 + n)), **dict(kw, **extra))


def _pol(name):
    return CFG[name][2]


def _sections(env):
    """The snapshot of `env` cut into its sections: a list of [num_envs, row_bytes] uint8 arrays."""
    buf, out, o = env.get_state(), [], 0
    for row in env.state_layout():
        out.append(buf[o:o + env.num_envs * row].reshape(env.num_envs, row))
        o += env.num_envs * row
    assert o == buf.size
    return out


def _readbacks(env):
    """What the host can read of every env, by name."""
    out = dict(counters=env.counters(), services=env.services(), active=env.active(), flags=env.flags())
    if env.ENV_TYPE == 4:
        out["spectrum"] = np.stack([env.spectrum(i) for i in range(env.num_envs)])
        out["link_stats"] = np.stack([env.link_stats(i) for i in range(env.num_envs)])
    else:
        out.update(slots_packed=env.slots_packed(), link_stats_all=env.link_stats_all(), net_stats_all=env.net_stats_all())
    if env.obs_dim:
        out["observation"] = env.observation().copy()
    return out


def _pending_sorted(env, i):
    t, rec = env.pending(i)
    order = np.lexsort(tuple(rec.T[::-1]) + (t,))
    return t[order], rec[order]


def _same_envs(tag, a, ia, d, idd, pending=(0, 2, 5)):
    """Envs `idd` of batch d equal envs `ia` of batch a on every read-back, and the pending releases of a few pairs."""
    chk = _exact_bits(tag)
    ra, rd = _readbacks(a), _readbacks(d)
    for k in ra:
        chk(0, k, rd[k][idd], ra[k][ia])
    for p in pending:
        ta, ca = _pending_sorted(a, int(ia[p]))
        td, cd = _pending_sorted(d, int(idd[p]))
        chk(p, "pending release times", td, ta)
        chk(p, "pending release records", cd, ca)


# ---- 1. byte for byte ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rmsa", "deeprmsa_j3", "rwa", "rmcsa_hist", "qos", "rmsa_discrete", "rmsa_tiny5"])
def test_rows_are_copied_byte_for_byte_and_neighbours_stay(name):
    A, D = _make(name, seed0=1000), _make(name, seed0=5000)
    A.run(_pol(name), 150)
    D.run(_pol(name), 150)
    layout = D.state_layout()
    assert layout == A.state_layout() and layout[SEC_SCAL] == 256 and layout[SEC_MT] == 624 * 4 and layout[1] == 8
    assert len(layout) >= 10 and sum(layout) * N == D.lib.orl_batch_state_bytes(D._h)
    if name == "rmsa_tiny5":
        assert any(r % 16 for r in layout)  # sections that are not made of 16-byte chunks
    a0, d0 = _sections(A), _sections(D)
    rates_a, rates_d = A.rates(), D.rates()
    assert any(not np.array_equal(x[SRC], y[DST]) for x, y in zip(a0, d0))

    D.copy_envs(SRC, DST, source=A)
    a1, d1 = _sections(A), _sections(D)
    others = np.setdiff1d(np.arange(N), DST)
    assert {1, 9, 65} <= set(others)
    for s, (x0, x1, y0, y1) in enumerate(zip(a0, a1, d0, d1)):
        assert np.array_equal(x1, x0), "section %d of the source changed" % s
        assert np.array_equal(y1[DST], x0[SRC]), "section %d: destination rows differ from the source rows" % s
        assert np.array_equal(y1[others], y0[others]), "section %d: a row that is no destination changed" % s
    if D.obs_dim:
        _exact_bits(name)(0, "observation", D.observation()[DST], A.observation()[SRC])
    for got, want in zip(A.rates() + D.rates(), rates_a + rates_d):
        assert np.array_equal(got, want)
    D.check()
    A.close()
    D.close()


# ---- 2. every step route -----------------------------------------------------------------------------------------------------------
def _flow(name, A, D):
    pol = _pol(name)
    A.run(pol, 150)
    D.run(pol, 150)
    D.copy_envs(SRC, DST, source=A)
    A.run(pol, 150)
    D.run(pol, 150)
    for _t in range(20):
        A.policy_step(pol, auto_reset=True, fetch=False)
        D.policy_step(pol, auto_reset=True, fetch=False)
    A.check()
    D.check()


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", ["rmsa", "deeprmsa", "rwa", "rmcsa"])
def test_the_copy_continues_as_its_source_under_every_step_route(name, impl, monkeypatch):
    force_impl(monkeypatch, impl)
    A, D = _make(name, seed0=1000), _make(name, seed0=5000)
    _flow(name, A, D)
    _same_envs("%s, %s" % (name, impl), A, SRC, D, DST)
    assert not np.array_equal(A.slots_packed()[1], D.slots_packed()[1])  # (the envs that were not copied are other envs)
    A.close()
    D.close()


@pytest.mark.parametrize("agent", ["0", "1"])
def test_the_copy_continues_as_its_source_qos(agent, monkeypatch):
    """QoSConstrainedRA through its two step kernels: one wavefront per env, and 8 lanes per env (forced; the library's choice from
    20 480 envs)."""
    for k in ("ORL_STEP_IMPL", "ORL_PERSIST", "ORL_LIB_VARIANT", "ORL_PERSIST_VARIANT", "ORL_PERSIST_INNER", "ORL_PERSIST_RW", "ORL_JIT_SPEC"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ORL_AGENT_STEP", agent)
    A, D = _make("qos", seed0=1000), _make("qos", seed0=5000)
    assert int(A.lib.orl_batch_debug_step_kernel(A._h)) == (2 if agent == "1" else 0)
    _flow("qos", A, D)
    _same_envs("qos, agent step %s" % agent, A, SRC, D, DST)
    A.close()
    D.close()


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rmsa", "rwa", "rmcsa"])
def test_the_copy_equals_the_oracle_on_the_sources_seed(name):
    from oracle.oracle import OracleBatch

    fam, kw, pol = CFG[name]
    A, D = _make(name, seed0=1000), _make(name, seed0=5000)
    A.run(pol, 150)
    D.run(pol, 150)
    D.copy_envs(SRC, DST, source=A)
    D.run(pol, 150)
    seeds = list(range(5000, 5000 + N))
    for s, d in zip(SRC, DST):
        seeds[d] = 1000 + int(s)
    ora = OracleBatch(fam, "nsfnet_chen", seeds, **kw)
    ora.run(pol, 300)
    chk = _exact_bits(name + " against the oracle")
    chk(0, "counters", D.counters(), ora.counters())
    chk(0, "services", D.services(), ora.services())
    chk(0, "active", D.active(), ora.active())
    chk(0, "slot maps", D.slots_packed(), ora.slots_packed())
    chk(0, "link statistics", D.link_stats_all(), ora.link_stats_all())
    chk(0, "network statistics", D.net_stats_all(), ora.net_stats_all())
    assert not D.flags().any()
    A.close()
    D.close()


# ---- 4. in place -----------------------------------------------------------------------------------------------------------------
def test_fan_out_in_place_over_a_whole_group():
    name = "rmsa"
    A = _make(name)
    A.run(_pol(name), 150)
    dst = np.arange(10, 18)
    A.copy_envs(3, dst)  # (a scalar source: the fork)
    A.run(_pol(name), 100)
    _same_envs("in place", A, np.full(8, 3), A, dst)
    maps = A.slots_packed()
    assert not np.array_equal(maps[3], maps[9]) and not np.array_equal(maps[3], maps[18])
    A.close()


# ---- 5. reseeded batches ---------------------------------------------------------------------------------------------------------
def test_reseeded_batches(monkeypatch):
    force_impl(monkeypatch, "wave64")
    name = "rmsa"
    A, D = _make(name, seed0=1000), _make(name, seed0=5000)
    mask = (np.arange(N) % 2 == 0).astype(np.uint8)  # (0, 66 reseeded; 5 not and its destinations 6, 8 are: the mark travels)
    A.seed(list(range(90000, 90000 + N)), mask=mask)
    D.seed(list(range(95000, 95000 + N)), mask=mask)
    assert len(D.state_layout()) == 11 and D.state_layout()[-1] == 624 * 4
    _flow(name, A, D)
    _same_envs("reseeded", A, SRC, D, DST)
    a, d = _sections(A), _sections(D)
    assert np.array_equal(d[-1][DST], a[-1][SRC])  # the second streams
    want = np.where(mask, ORL_FLAG_MT2, 0)
    want[DST] = want[SRC]
    assert np.array_equal(D.flags(), want)
    A.close()
    D.close()


def test_reseeded_and_fresh_batches_do_not_mix():
    from optical_rl_gym_amd._lib import OrlError

    name = "rmsa"
    R, F = _make(name, seed0=1000), _make(name, seed0=5000)
    R.seed(list(range(90000, 90000 + N)), mask=(np.arange(N) % 2 == 0).astype(np.uint8))
    R.run(_pol(name), 40)
    F.run(_pol(name), 40)
    r0, f0 = R.get_state(), F.get_state()
    for dst, src in ((R, F), (F, R)):
        with pytest.raises(OrlError, match="seed\\(\\) the other batch first"):
            dst.copy_envs(SRC, DST, source=src)
    assert np.array_equal(R.get_state(), r0) and np.array_equal(F.get_state(), f0)
    F.seed(list(range(N)), mask=np.zeros(N, np.uint8))  # allocates the second streams, reseeds no env
    assert not F.flags().any()
    F.copy_envs(SRC, DST, source=R)
    R.run(_pol(name), 40)
    F.run(_pol(name), 40)
    _same_envs("fresh batch after seed(mask = 0)", R, SRC, F, DST)
    R.close()
    F.close()


# ---- 6. keep_rng ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,reseed", [("rmsa", False), ("rwa", False), ("rmsa", True)])
def test_keep_rng_takes_the_state_and_keeps_the_streams(name, reseed, monkeypatch):
    if reseed:
        force_impl(monkeypatch, "wave64")
    pol = _pol(name)
    A, D, D2 = _make(name, seed0=1000), _make(name, seed0=5000), _make(name, seed0=5000)
    if reseed:
        mask = (np.arange(N) % 2 == 0).astype(np.uint8)
        A.seed(list(range(90000, 90000 + N)), mask=mask)
        for b in (D, D2):
            b.seed(list(range(95000, 95000 + N)), mask=(np.arange(N) % 3 == 0).astype(np.uint8))
    for b in (A, D, D2):
        b.run(pol, 150)
    d0 = _sections(D)
    flags0 = D.flags()
    D.copy_envs(SRC, DST, source=A, keep_rng=True)
    chk = _exact_bits("%s keep_rng" % name)
    for what in ("slots_packed", "link_stats_all", "net_stats_all", "counters", "active", "services"):
        chk(0, what, getattr(D, what)()[DST], getattr(A, what)()[SRC])
    d1, a1 = _sections(D), _sections(A)
    rng_sections = [SEC_MT] + ([len(d1) - 1] if reseed else [])
    for s in rng_sections:
        assert np.array_equal(d1[s], d0[s]), "stream section %d changed" % s
    for s in range(len(d1)):
        if s not in rng_sections and s != SEC_SCAL:
            assert np.array_equal(d1[s][DST], a1[s][SRC]), "section %d" % s
    # the scalar record: the source's but for the stream positions (high halves of words 18 and 22) and the reseeded mark
    rec_d0, rec_d1, rec_a = (x[SEC_SCAL].view(np.uint64) for x in (d0, d1, a1))
    keep = np.zeros(32, np.uint64)
    keep[18] = keep[22] = 0xFFFFFFFF00000000
    keep[20] = ORL_FLAG_MT2 << 32
    assert np.array_equal(rec_d1[DST], (rec_a[SRC] & ~keep) | (rec_d0[DST] & keep))
    assert np.array_equal(D.flags()[DST] & ORL_FLAG_MT2, flags0[DST] & ORL_FLAG_MT2)
    assert np.array_equal(d1[SEC_SCAL][np.setdiff1d(np.arange(N), DST)], d0[SEC_SCAL][np.setdiff1d(np.arange(N), DST)])
    differ = 0
    for m in range(1, 41):
        D.policy_step(pol, auto_reset=True, fetch=False)
        D2.policy_step(pol, auto_reset=True, fetch=False)
        s1, s2 = D.services(), D2.services()
        # holding time (bits), source, destination, bit rate: drawn from the env's own stream at the position it had
        chk(m, "services drawn after the copy", s1[DST][:, 1:5], s2[DST][:, 1:5])
        differ += int(not np.array_equal(D.slots_packed()[DST], D2.slots_packed()[DST]))
    assert differ == 40  # (on the source's network state, not on the one the twin kept)
    for b in (A, D, D2):
        b.check()
        b.close()


# ---- 7. stream ordering --------------------------------------------------------------------------------------------------------------
def test_the_copy_is_ordered_with_the_sources_stream(monkeypatch):
    for k in ("ORL_STEP_IMPL", "ORL_PERSIST", "ORL_AGENT_STEP", "ORL_LIB_VARIANT", "ORL_PERSIST_VARIANT", "ORL_PERSIST_INNER", "ORL_PERSIST_RW",
              "ORL_JIT_SPEC"):
        monkeypatch.delenv(k, raising=False)
    name, n = "rmsa", 2048
    pol = _pol(name)
    A, T30, T60, D = _make(name, n=n), _make(name, n=n), _make(name, n=n), _make(name, n=n, seed0=50000)
    assert int(A.lib.orl_batch_debug_step_kernel(A._h)) == 2  # k_agent
    every = np.arange(n)
    for _t in range(30):
        A.policy_step(pol, auto_reset=True, fetch=False)
    D.copy_envs(every, every, source=A)
    for _t in range(30):
        A.policy_step(pol, auto_reset=True, fetch=False)
    A.sync()
    D.sync()
    for _t in range(60):
        T60.policy_step(pol, auto_reset=True, fetch=False)
        if _t < 30:
            T30.policy_step(pol, auto_reset=True, fetch=False)
    chk = _exact_bits("stream ordering")
    for what in ("counters", "services", "slots_packed", "link_stats_all", "net_stats_all", "active"):
        chk(30, what + " of the copy", getattr(D, what)(), getattr(T30, what)())
        chk(60, what + " of the source", getattr(A, what)(), getattr(T60, what)())
    assert np.array_equal(D.get_state(), T30.get_state())
    for b in (A, T30, T60, D):
        b.check()
        b.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was():
    from optical_rl_gym_amd._lib import OrlError

    A, D = _make("rmsa_discrete", seed0=1000), _make("rmsa_discrete", seed0=5000)
    others = {
        "num_spectrum_resources": _make("rmsa_discrete", num_spectrum_resources=128),
        "env family": _make("rwa"),
        "action_histograms": _make("rmsa_discrete", action_histograms=True),
        "event capacity": _make("rmsa_discrete", load=1000),
    }
    for b in [A, D] + list(others.values()):
        b.run("SAP_FF", 30)
    a0, d0 = A.get_state(), D.get_state()
    for src, dst, word in (([-1], [0], "source index -1"), ([N], [0], "source index"), ([0], [-1], "destination index -1"),
                           ([0], [N], "destination index"), ([1, 2], [5, 5], "occurs twice")):
        for source in (A, None):
            with pytest.raises(OrlError, match=word):
                D.copy_envs(src, dst, source=source)
    for src, dst in (([0, 1], [1, 2]), ([0, 1], [1, 0])):
        with pytest.raises(OrlError, match="scratch batch"):
            D.copy_envs(src, dst)
    for word, other in others.items():
        o0 = other.get_state()
        with pytest.raises(OrlError, match=word):
            D.copy_envs(SRC, DST, source=other)
        with pytest.raises(OrlError, match=word):
            other.copy_envs(SRC, DST, source=D)
        assert np.array_equal(other.get_state(), o0), word
    for bad in (([0.5], [1]), ([[0]], [[1]]), ([0, 1], [1]), (["a"], [1])):
        with pytest.raises(ValueError):
            D.copy_envs(*bad)
    with pytest.raises(ValueError):
        D.copy_envs([0], [1], source="A")
    D.copy_envs([], [])  # nothing to do
    D.copy_envs([4, 9], [4, 9])  # no-ops
    assert np.array_equal(A.get_state(), a0) and np.array_equal(D.get_state(), d0)
    for b in [A, D] + list(others.values()):
        b.close()


# ---- 9. MultiDeviceBatch ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devs", [pytest.param((0,), id="one_gpu"), pytest.param((0, 1), id="two_gpus")])
def test_multi_device_batch(devs):
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    _need_devices(devs)
    name = "rmsa"
    fam, kw, pol = CFG[name]
    if len(devs) == 1:
        # two shards on one GPU: pairs inside a shard and between the shards give what the unsharded batch gives
        m = MultiDeviceBatch.from_shards([_make(name, n=N, seed0=1000), _make(name, n=61, seed0=1000 + N)])
        whole = _make(name, n=N + 61, seed0=1000)
        m.run(pol, 150)
        whole.run(pol, 150)
        src = np.array([0, 0, 66, 70, 127, 100, 40])
        dst = np.array([1, 67, 2, 71, 3, 126, 40])  # inside shard 0, 0 -> 1, 0 -> 0, inside shard 1, 1 -> 0, inside shard 1, a no-op
        m.copy_envs(src, dst)
        whole.copy_envs(src, dst)
        m.run(pol, 100)
        whole.run(pol, 100)
        chk = _exact_bits("sharded copy")
        chk(0, "counters", m.counters(), whole.counters())
        chk(0, "services", m.services(), whole.services())
        chk(0, "slot maps", np.concatenate([s.slots_packed() for s in m.shards]), whole.slots_packed())
        chk(0, "network statistics", np.concatenate([s.net_stats_all() for s in m.shards]), whole.net_stats_all())
        chk(0, "copies", whole.counters()[dst], whole.counters()[src])
        with pytest.raises(ValueError, match="source of another"):
            m.copy_envs([0, 67], [67, 5])
        with pytest.raises(ValueError, match="outside"):
            m.copy_envs([0], [N + 61])
        whole.close()
    else:
        n = 2 * N
        m = orl.make(fam, topology="nsfnet_chen", num_envs=n, seeds=list(range(1000, 1000 + n)), device_ids=list(devs), **kw)
        m.run(pol, 150)
        before = [s.get_state() for s in m.shards]
        with pytest.raises(ValueError, match="pair 1 \\(3 -> %d\\)" % (N + 1)):
            m.copy_envs([0, 3], [1, N + 1])  # the pair inside shard 0 is listed first and must not have been applied
        for s, b in zip(m.shards, before):
            assert np.array_equal(s.get_state(), b)
        m.copy_envs([0, N], [1, N + 1])  # inside each shard
        chk = _exact_bits("two devices")
        chk(0, "counters", m.counters()[[1, N + 1]], m.counters()[[0, N]])
    m.close()


# ---- 10. full size -----------------------------------------------------------------------------------------------------------------
def test_full_size_identity_copy_into_a_second_batch():
    from bench import WORKLOADS

    import optical_rl_gym_amd as orl

    fam, topo, kw, pol = WORKLOADS["cfg2"]
    n = 65536
    A = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(10, 10 + n)), **kw)
    D = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(10 + n, 10 + 2 * n)), **kw)
    A.run(pol, 300)
    every = np.arange(n)
    D.copy_envs(every, every, source=A)
    A.run(pol, 100)
    D.run(pol, 100)
    chk = _exact_bits("65 536 envs")
    chk(0, "counters", D.counters(), A.counters())
    chk(0, "slot maps", D.slots_packed(), A.slots_packed())
    chk(0, "network statistics", D.net_stats_all(), A.net_stats_all())
    assert not D.flags().any()
    A.close()
    D.close()
