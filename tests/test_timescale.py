"""The time-scale table (tests/timescale.py) on the CPU oracle alone: multiplying both mean times by 2^k leaves every integer and
every quotient of two times as it was and multiplies every time by 2^k, bit for bit — the lever the GPU tests lean on, proved on
plain doubles and a heap — and every case shows, in the oracle's recorded service stream, the condition it exists for."""
import functools

import numpy as np
import pytest

from tests import timescale as ts
from tests.helpers import _exact_bits

N_ENVS, STEPS, WARM = 16, 300, 150
CASES = [(f, c) for f in ts.FAMILIES for c in ts.ks_of(f) + ts.PLAIN]
IDS = ["%s-%s" % (f, ts.case_id(c)) for f, c in CASES]


@functools.lru_cache(maxsize=None)
def walk(fam, case):
    """300 host-driven steps of 16 oracle envs under the family's heuristic -> what every step left, [steps][envs][..]:
    the service before the step and the one drawn by it, action, reward, done, info, counters, pending releases, slot maps
    (QoSConstrainedRA: free units per link), link and network statistics, observation; the action histograms at the end."""
    from oracle.oracle import OracleBatch

    b = ts.BASES[fam]
    ora = OracleBatch(fam, ts.TOPO, ts.seeds_of(fam, N_ENVS), **ts.kwargs_of(fam, case))
    qos = fam == "QoSConstrainedRA"
    rec = {k: [] for k in ("svc", "actions", "reward", "done", "info", "counters", "active", "services", "maps", "link statistics",
                           "network statistics", "observation")}
    for _t in range(STEPS):
        rec["svc"].append(ora.services())
        a = ora.policy(b.policy).copy()
        obs, r, d, info = ora.step(a, auto_reset=True)
        rec["actions"].append(a)
        rec["reward"].append(r)
        rec["done"].append(d)
        rec["info"].append(info)
        rec["counters"].append(ora.counters())
        rec["active"].append(ora.active())
        rec["services"].append(ora.services())
        rec["maps"].append(np.array([ora.spectrum(i) for i in range(N_ENVS)]) if qos else ora.slots_packed())
        rec["link statistics"].append(ora.link_stats_all())
        rec["network statistics"].append(ora.net_stats_all())
        rec["observation"].append(ora.observation() if ora.obs_dim else np.zeros((N_ENVS, 0)))
    out = {k: np.array(v) for k, v in rec.items()}
    out["histograms"] = np.array([np.stack(ora.action_histograms_of(i)) for i in range(N_ENVS)]) if not qos else np.zeros(0)
    for v in out.values():
        v.setflags(write=False)
    return out


def stream(w):
    """The recorded service stream of a walk: clock[t] = arrival time of the service step t processes (the clock while it is
    provisioned), gap[t] = the clock's advance to the next service, ahead[t] = release time - clock of the service when it was
    accepted (nan when it was not), pending[t][e] = the release times still pending after step t — accepted services whose
    release time lies beyond the new clock; checked against the oracle's own count."""
    at, ht = w["svc"][..., 0], w["svc"][..., 1]
    clock_after = w["services"][..., 0]
    accepted = np.diff(np.concatenate([np.zeros((1, N_ENVS), np.int64), w["counters"][..., 1]]), axis=0) == 1
    pending = []
    cur = [[] for _ in range(N_ENVS)]
    for t in range(STEPS):
        for e in range(N_ENVS):
            if accepted[t, e]:
                cur[e].append(at[t, e] + ht[t, e])
            cur[e] = [x for x in cur[e] if x > clock_after[t, e]]
            assert len(cur[e]) == w["active"][t, e]
        pending.append([np.array(c) for c in cur])
    return dict(clock=at, after=clock_after, gap=clock_after - at, ahead=np.where(accepted, ht, np.nan), accepted=accepted, pending=pending)


@pytest.mark.parametrize("fam,k", [(f, k) for f in ts.FAMILIES for k in ts.ks_of(f)], ids=["%s-k%+d" % (f, k) for f in ts.FAMILIES for k in ts.ks_of(f)])
def test_scaling_both_means_by_a_power_of_two_scales_the_times_and_nothing_else(fam, k):
    base, w = walk(fam, 0), walk(fam, k)
    chk = _exact_bits("%s at 2^%d against the base scale" % (fam, k))
    for t in range(STEPS):
        for what in ("actions", "done", "counters", "active", "maps"):  # integers
            chk(t, what, w[what][t], base[what][t])
        for what in ("reward", "info", "observation"):  # quotients of two times, or no times at all: the same bits
            chk(t, what, w[what][t], base[what][t])
        for what in ("services", "link statistics", "network statistics"):  # the times among them: the base's times 2^k
            chk(t, what, w[what][t], ts.scaled(what, base[what][t], k))
        chk(t, "service before the step", w["svc"][t], ts.scaled("services", base["svc"][t], k))
    chk(STEPS, "action histograms", w["histograms"], base["histograms"])
    if k:  # (the times did change: the comparison above is not one of a run with itself)
        assert (w["services"][..., 0] != base["services"][..., 0]).all()


def _frac(mask, of=None):
    of = np.ones_like(mask, bool) if of is None else of
    return float((mask & of).sum()) / float(of.sum())


@pytest.mark.parametrize("fam,case", CASES, ids=IDS)
def test_each_case_shows_the_condition_it_exists_for(fam, case):
    """Conditions on the inputs (the oracle's stream), not measurements of the code under test: a case that misses one is
    changed in the table, the thresholds stay."""
    w = walk(fam, case)
    s = stream(w)
    acc = s["accepted"]
    cond = ts.scale_of(fam, case).cond if not isinstance(case, str) else ("ahead_most" if case == "h10800_load100" else None)
    assert acc.sum() > N_ENVS * STEPS // 4
    if not isinstance(case, str):  # every scaled case: more pending releases than the soon list's 40 entries
        assert (w["active"][WARM:].max(axis=0) > 40).all()
    if cond in ("ahead_most", "gap_both_sides", "gap_most_beyond", "gap_all_beyond"):  # the scales from "most pushes beyond" upwards, and 10 800 at load 100
        assert w["active"].max() >= 48
        assert _frac(s["ahead"] > ts.AHEAD, acc) >= 0.5
    if cond == "ahead_both_sides":
        assert _frac(s["ahead"] > ts.AHEAD, acc) >= 0.05 and _frac(s["ahead"] < ts.AHEAD, acc) >= 0.05
    if cond == "gap_both_sides":
        assert _frac(s["gap"] > ts.OVERDUE) >= 0.10 and _frac(s["gap"] < ts.OVERDUE) >= 0.10
    if cond in ("gap_most_beyond", "gap_all_beyond"):
        assert (s["gap"] > ts.OVERDUE).all() if cond == "gap_all_beyond" else _frac(s["gap"] > ts.OVERDUE) >= 0.99
        released = w["active"][:-1] + acc[1:] - w["active"][1:]
        assert (released >= 2).any()
    if cond == "one_quantum":
        for t in range(WARM, STEPS):
            for e in range(N_ENVS):
                assert (np.abs(s["pending"][t][e] - s["after"][t, e]) < ts.QUANTUM).all()
    if cond == "quantum_both_sides":
        same = differ = False
        for t in range(WARM, STEPS):
            for e in range(N_ENVS):
                q = np.floor((s["pending"][t][e] - s["after"][t, e]) * 4096.0)
                same |= len(np.unique(q)) < len(q)
                differ |= len(np.unique(q)) > 1
        assert same and differ


def test_the_table_names_a_constant_and_a_side_for_every_scale():
    assert [s.k for s in ts.SCALES][0] == 0 and len(set(ts.KS)) == len(ts.KS)
    assert all(s.constant and s.side for s in ts.SCALES) and all(abs(s.k) <= 40 for s in ts.SCALES)
    for fam in ts.FAMILIES:
        for k in ts.ks_of(fam):
            kw0, kw = ts.kwargs_of(fam, 0), ts.kwargs_of(fam, k)
            assert kw["mean_service_holding_time"] == kw0["mean_service_holding_time"] * 2.0 ** k
            if fam == "DeepRMSA":
                assert kw["mean_service_inter_arrival_time"] == kw0["mean_service_inter_arrival_time"] * 2.0 ** k
            else:
                assert kw["load"] == kw0["load"] == ts.BASES[fam].load


@pytest.mark.parametrize("fam", ts.FAMILIES)
def test_the_oracles_set_load_reproduces_the_reference_trace(fam):
    """The GPU tests move envs between scales with set_load and compare with the oracle's: the oracle's own set_load against
    the reference's recorded one (tests/golden/s1_*.npz)."""
    from oracle.oracle import OracleBatch
    from tests.helpers import S1, _exact, _replay_with_schedule, load_golden

    g = load_golden(S1[fam])
    kw = dict(g["meta"]["kwargs"])
    seed = kw.pop("seed")
    ora = OracleBatch(g["meta"]["env"], g["meta"]["topology"], [seed], **kw)
    _replay_with_schedule(ora, g, _exact("oracle, " + S1[fam]))
    after = g["after_change"][-1]
    assert ora.load == after[1] and ora.mean_service_holding_time == after[2]
