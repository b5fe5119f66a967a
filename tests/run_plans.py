"""The run-plan table: the small configurations, batch sizes, plans and forms under which device-resident runs are compared with the
CPU oracle, the case matrix made of them, the oracle behind one interface (one batch, or one env per batch where every env has a
load of its own) with a ledger of finished episodes, and the sequences the cases drive — shared by tests/test_run_plans.py (CPU:
the plan every (batch, plan) pair must give, the forms, and the conditions on the oracle's trajectories without which the GPU
checks would pass trivially) and tests/test_run_plans_gpu.py.  Helper module, no tests.

A plan is (chunk, parts): the steps per launch of the persistent kernel (ORL_PERSIST_CHUNK) and one stream or two halves on two
streams (ORL_PERSIST_PARTS), csrc/orl_run_plan.h.  The second half's per-env pointers are offset by hand (env_view,
csrc/orl_api.hip); the library takes two halves from 16 384 envs only, so nothing but these overrides reaches that code at a size
where every env can be compared after every piece."""
import math
from collections import namedtuple

import numpy as np

from tests.helpers import IMPLS, _exact_bits, _ran_pair_form

TOPO = "nsfnet_chen"
QOS = "QoSConstrainedRA"

# ---- configurations -------------------------------------------------------------------------------------------------------
# kw: what the batch and the oracle both take; dev_kw: the batch alone (opt-in arrays the oracle always keeps).  loads: a function
# of the batch size for the configuration with one load per env.  paths: the PATH_FF path column of env i.
Config = namedtuple("Config", "name fam kw dev_kw policy loads paths")


def _cfg(name, fam, policy, dev_kw=None, loads=None, paths=None, **kw):
    return Config(name, fam, kw, dev_kw or {}, policy, loads, paths)


def _loads(n):
    """one load per env, rising over the batch: the halves of every batch size share no value"""
    return [90.0 + 11.0 * i for i in range(n)]


def _paths(n):
    """PATH_FF: the path column (k = 5: 5 rejects).  Envs 16 apart — the same lane of the two halves of a 20-env batch — differ."""
    return [(7 * i + 3) % 6 for i in range(n)]


_RMSA = dict(num_spectrum_resources=32, allow_rejection=True, mean_service_holding_time=25.0)
CONFIGS = {c.name: c for c in [
    _cfg("rmsa", "RMSA", "SAP_FF", episode_length=14, load=260.0, **_RMSA),
    _cfg("rmsa_disc", "RMSA", "SAP_FF", dev_kw=dict(action_histograms=True), episode_length=16, load=200.0, bit_rate_selection="discrete", **_RMSA),
    _cfg("deeprmsa", "DeepRMSA", "SAP", j=2, num_spectrum_resources=32, allow_rejection=True, episode_length=12, mean_service_holding_time=7.5,
         mean_service_inter_arrival_time=7.5 / 260.0),
    _cfg("rwa", "RWA", "SAP_FF", num_spectrum_resources=8, allow_rejection=True, episode_length=20, load=260.0,
         mean_service_holding_time=25.0),
    _cfg("rmcsa", "RMCSA", "SAP_BM_FC_FF", num_spectrum_resources=64, num_spatial_resources=7, worst_xt=-84.7, allow_rejection=True, episode_length=13,
         load=1400.0, mean_service_holding_time=25.0),
    _cfg("rmsa_loads", "RMSA", "SAP_FF", loads=_loads, episode_length=18, **_RMSA),
    # parts 2 and 3 only
    _cfg("rmcsa_small", "RMCSA", "SAP_BM_FC_FF", dev_kw=dict(action_histograms=True), num_spectrum_resources=16, num_spatial_resources=2, worst_xt=-84.7,
         allow_rejection=True, episode_length=12, load=160.0, mean_service_holding_time=25.0),
    _cfg("rmsa_pathff", "RMSA", "PATH_FF", paths=_paths, episode_length=15, load=260.0, **_RMSA),
    _cfg("qos", QOS, "SAP_FF", num_spectrum_resources=4, num_service_classes=3, classes_arrival_probabilities=[0.2, 0.5, 0.3],
         classes_reward=[10.0, 2.0, 1.0], allow_rejection=True, episode_length=12, load=800.0, mean_service_holding_time=25.0),
]}
MATRIX_CONFIGS = ["rmsa", "rmsa_disc", "deeprmsa", "rwa", "rmcsa", "rmsa_loads"]


def steps_per_episode(cfg):
    """Steps of an episode that starts with a soft reset.  RMSA and DeepRMSA count a service at creation and again in the soft
    reset (rmsa_env.py:280, 314, 576), RMCSA at the decision and in the soft reset (rmcsa_env.py:293, 414): episode_length - 1
    steps (the first episode of a fresh RMCSA env has one more).  RWA and QoSConstrainedRA count at the decision."""
    el = cfg.kw["episode_length"]
    return el if cfg.fam in ("RWA", QOS) else el - 1


def seeds_of(cfg, n):
    return [5000 + 13 * i + 7 * len(cfg.name) for i in range(n)]


def dev_kwargs(cfg, n):
    kw = dict(cfg.kw, **cfg.dev_kw)
    if cfg.loads:
        kw["load"] = cfg.loads(n)
    return kw


def make_dev(cfg, n):
    import optical_rl_gym_amd as orl

    dev = orl.make(cfg.fam, topology=TOPO, num_envs=n, seeds=seeds_of(cfg, n), **dev_kwargs(cfg, n))
    if cfg.paths:
        dev.set_paths(cfg.paths(n))
    return dev


# ---- batch sizes, plans, forms -------------------------------------------------------------------------------------------
# envs -> (envs of the first half, envs of the second half) when two parts are asked for.  8 envs are one wavefront:
# ORL_PERSIST_PARTS=2 falls back to one part.
BATCHES = {20: (16, 4), 9: (8, 1), 64: (32, 32), 8: (8, 0)}
# (chunk, parts); L = steps_per_episode of the configuration
PLANS = [("128", 1), ("128", 2), ("1", 2), ("L", 2), ("L-1", 2), ("L+1", 1), ("7", 2)]
FORMS = ["persist", "persist_global", "persist_lds", "persist_pair", "persist_rd"]
PAIR_CONFIGS = ("rmsa", "deeprmsa")  # the two-wavefront form needs a specialisation build per configuration
assert set(FORMS) <= set(IMPLS)
# the forms a family is built in, where that is not all of them: RMCSA has neither the LDS-resident nor the rows-deferred form (asked
# for, the library's own choice runs), and its "persist_pair" is the one-wavefront kernel, specialised
FAMILY_FORMS = {"RMCSA": ("persist", "persist_global", "persist_pair")}


def forms_of_family(fam):
    return FAMILY_FORMS.get(fam, tuple(FORMS))


def chunk_of(plan, L):
    return {"128": 128, "1": 1, "L": L, "L-1": L - 1, "L+1": L + 1, "7": 7}[plan[0]]


def plan_id(plan):
    return "chunk%s-parts%d" % plan


def expected_split(n, plan):
    """(parts, half) the library must plan for `n` envs under `plan`: the table of BATCHES"""
    first, second = BATCHES[n]
    if plan[1] == 2 and second > 0:
        return 2, first
    return 1, n


def set_plan(monkeypatch, cfg, plan):
    monkeypatch.setenv("ORL_PERSIST_CHUNK", str(chunk_of(plan, steps_per_episode(cfg))))
    monkeypatch.setenv("ORL_PERSIST_PARTS", str(plan[1]))


Case = namedtuple("Case", "config form plan n")


def case_id(c):
    return "%s-%d-%s-%s" % (c.config, c.n, c.form, plan_id(c.plan))


def forms_of(config):
    return [f for f in FORMS if f != "persist_pair" or config in PAIR_CONFIGS]


def matrix():
    """RMSA continuous at 20 envs through every form and every plan; every other configuration through every plan twice, the forms
    and the batch sizes cycling against them (tests/test_run_plans.py checks what the subset must cover)."""
    cases = [Case("rmsa", f, p, 20) for f in FORMS for p in PLANS]
    sizes = [20, 9, 64, 8]
    for ci, name in enumerate(MATRIX_CONFIGS[1:]):
        forms = forms_of(name)
        for sweep in (0, 1):
            for pi, plan in enumerate(PLANS):
                n = sizes[(pi + ci + 2 * sweep) % 4]
                if n == 8 and plan[1] == 1:  # the one-wavefront batch is there for the fall-back from two parts
                    n = 9
                cases.append(Case(name, forms[(pi + ci + 3 * sweep) % len(forms)], plan, n))
    for n in sizes[1:]:  # RMSA continuous at the other sizes
        cases.append(Case("rmsa", "persist", ("7", 2), n))
    return list(dict.fromkeys(cases))


def expected_form(cfg, form):
    """The form number orl_batch_debug_persist_form must report after a run forced to `form` (helpers.IMPL_ENV), None where the
    library's own choice runs and only its pure restatement (persist_choice) is asserted: global state is form 0 (RMCSA, which is
    not built in the 4-wave forms: 1), the LDS-resident form of the cross-implementation build 2, rows deferred 7 for the single-core
    families."""
    rmcsa = cfg.fam == "RMCSA"
    return {"persist": None, "persist_global": 1 if rmcsa else 0, "persist_lds": None if rmcsa else 2, "persist_pair": None,
            "persist_rd": None if rmcsa else 7}[form]


def assert_form_ran(dev, cfg, form, what):
    got = int(dev.lib.orl_batch_debug_persist_form(dev._h))
    choice = dev.persist_choice(dev.num_envs, tuned=dev.specialised)
    assert choice is not None and got == choice[0], (what, got, choice)
    want = expected_form(cfg, form)
    assert want is None or got == want, (what, got, want)
    if form == "persist_pair":
        assert dev.specialised and _ran_pair_form(dev) == (cfg.fam != "RMCSA"), what


def assert_plan(dev, cfg, plan, n_steps, what):
    """orl_debug_run_plan under the environment the run is made in: the parts and the split point the case is there for, and the
    launch length asked for (the statistics log never shortens launches this short)"""
    parts, half = expected_split(dev.num_envs, plan)
    p = dict(zip(dev.RUN_PLAN_FIELDS, dev.run_plan(dev.num_envs, n_steps, tuned=dev.specialised)))
    assert p["persist"] == 1 and (p["parts"], p["half"]) == (parts, half), (what, p)
    assert p["chunk"] == chunk_of(plan, steps_per_episode(cfg)), (what, p)
    return p


# ---- the oracle behind one interface, with a ledger of finished episodes --------------------------------------------------
BULK = ("services", "counters", "active", "slots_packed", "link_stats_all", "net_stats_all", "observation")


class Ora:
    """`n` oracle envs of configuration `cfg`: one OracleBatch, or one per env where every env has a load of its own.  Read-backs
    come back in env order.  With ledger=True every run is stepped on the host with auto reset and the finished episodes of every
    env are kept: the accepted steps between two `done`s, and the float64 sum of the step rewards in step order from 0.0 — the
    reference of the episode log."""

    def __init__(self, cfg, n, ledger=False):
        from oracle.oracle import OracleBatch

        seeds = seeds_of(cfg, n)
        self.cfg, self.n = cfg, n
        if cfg.loads:
            self.groups = [([i], OracleBatch(cfg.fam, TOPO, [seeds[i]], load=ld, **cfg.kw)) for i, ld in enumerate(cfg.loads(n))]
        else:
            self.groups = [(list(range(n)), OracleBatch(cfg.fam, TOPO, seeds, **cfg.kw))]
        self.obs_dim = self.groups[0][1].obs_dim
        if cfg.paths:
            self.set_paths(cfg.paths(n))
        self.ledger = ledger
        self._acc, self._rew, self._steps = np.zeros(self.n, np.int64), np.zeros(self.n, np.float64), np.zeros(self.n, np.int64)
        self.start_ledger()

    def start_ledger(self):
        """Forget the finished episodes (where the batch's log is armed).  The running episode's accepted steps stay — the batch
        logs the env's own episode counter — so arm at an episode's start (after a soft reset) wherever reward sums are compared."""
        self.episodes = [[] for _ in range(self.n)]      # accepted steps of every finished episode
        self.episode_rewards = [[] for _ in range(self.n)]
        self.mixed = np.zeros(self.n, bool)              # the env finished an episode with accepted and rejected services
        self.rates_seen = [set() for _ in range(self.n)]  # the bit rates of the services the env was asked to place

    def _gather(self, fn):
        out = None
        for idx, o in self.groups:
            v = np.asarray(fn(o))
            if out is None:
                out = np.zeros((self.n,) + v.shape[1:], v.dtype)
            out[idx] = v
        return out

    def __getattr__(self, name):
        if name in BULK:
            return lambda: self._gather(lambda o: getattr(o, name)())
        raise AttributeError(name)

    def one(self, i, name):
        for idx, o in self.groups:
            if i in idx:
                return getattr(o, name)(idx.index(i))
        raise IndexError(i)

    def action_histograms_of(self, i):
        return self.one(i, "action_histograms_of")

    def set_paths(self, paths):
        for idx, o in self.groups:
            o.set_paths([paths[i] for i in idx])

    def policy(self, policy):
        return self._gather(lambda o: o.policy(policy))

    def step(self, actions, auto_reset=True):
        before = self.counters()[:, 1]
        if self.ledger:
            for i, rate in enumerate(self.services()[:, 4]):
                self.rates_seen[i].add(int(rate))
        actions = np.asarray(actions)
        res = [(idx, o.step(actions[idx], auto_reset=auto_reset)) for idx, o in self.groups]
        reward, done = np.zeros(self.n), np.zeros(self.n, np.uint8)
        info = np.zeros((self.n, res[0][1][3].shape[1]))
        for idx, (_o, r, d, i) in res:
            reward[idx], done[idx], info[idx] = r, d, i
        accepted = self.counters()[:, 1] - before
        for i in range(self.n):
            self._acc[i] += accepted[i]
            self._rew[i] = self._rew[i] + reward[i]
            self._steps[i] += 1
            if done[i]:
                self.episodes[i].append(int(self._acc[i]))
                self.episode_rewards[i].append(float(self._rew[i]))
                self.mixed[i] |= 0 < self._acc[i] < self._steps[i]
                self._acc[i], self._rew[i], self._steps[i] = 0, 0.0, 0
        return reward, done, info

    def run(self, policy, n_steps):
        if self.ledger:
            for _ in range(n_steps):
                self.step(self.policy(policy), auto_reset=True)
        else:
            for _idx, o in self.groups:
                o.run(policy, n_steps)

    def reset(self, full=False, mask=None):
        for idx, o in self.groups:
            o.reset(full=full, mask=None if mask is None else np.asarray(mask, np.uint8)[idx])
        sel = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self._acc[sel], self._rew[sel], self._steps[sel] = 0, 0.0, 0

    def set_load(self, load, mask):
        """per-env configuration only: env i goes on at load[i] where mask[i]"""
        for idx, o in self.groups:
            if mask[idx[0]]:
                o.set_load(load=float(load[idx[0]]))


# ---- what is compared after every piece ---------------------------------------------------------------------------------
def snapshot(b, fam, n, ora=None):
    """counters, pending service, pending releases, slot maps, link and network statistics and the observation of every env (one
    bulk read-back each); QoSConstrainedRA, which has no bulk read-backs of its state: free units, utilisation and last update per
    link of every env."""
    s = {"counters": b.counters(), "services": b.services(), "active": b.active()}
    if fam == QOS:
        get = (lambda i, name: getattr(b, name)(i)) if ora is None else ora.one
        s["spectrum"] = np.array([get(i, "spectrum") for i in range(n)])
        s["link statistics (qos)"] = np.array([get(i, "link_stats")[[0, 3]] for i in range(n)])
    else:
        s["slot maps"] = b.slots_packed()
        s["link statistics"] = b.link_stats_all()
        s["network statistics"] = b.net_stats_all()
        if b.obs_dim:
            s["observation"] = b.observation()
    return {what: np.array(v) for what, v in s.items()}


def half_of(i, n, plan):
    parts, half = expected_split(n, plan)
    return "the only part" if parts == 1 else ("first half" if i < half else "second half")


def compare(dev, ora, cfg, plan, tag, label):
    """every quantity of every env, floats as bit patterns; a difference names the envs and their half"""
    n = dev.num_envs
    got, ref = snapshot(dev, cfg.fam, n), snapshot(ora, cfg.fam, n, ora)
    for what in ref:
        g, r = got[what], ref[what]
        if g.dtype.kind == "f":
            g, r = np.ascontiguousarray(g, np.float64).view(np.uint64), np.ascontiguousarray(r, np.float64).view(np.uint64)
        if not np.array_equal(g, r):
            bad = [i for i in range(n) if not np.array_equal(g[i], r[i])]
            where = ", ".join("env %d (%s)" % (i, half_of(i, n, plan)) for i in bad[:8])
            _exact_bits("%s, %s: %s" % (tag, label, where))(0, what, got[what][bad[0]], ref[what][bad[0]])
    assert not dev.flags().any(), (tag, label)


def host_steps(dev, ora, cfg, n_steps, tag, auto_reset=True):
    """host-driven steps under the oracle's actions: reward, done and info of every env at every step"""
    chk = _exact_bits("%s, host steps" % tag)
    dones = []
    for t in range(n_steps):
        a = ora.policy(cfg.policy)
        _o, r_d, d_d, i_d = dev.step(a, auto_reset=auto_reset)
        r_o, d_o, i_o = ora.step(a, auto_reset=auto_reset)
        chk(t, "reward", r_d, r_o)
        chk(t, "done", d_d, d_o)
        chk(t, "info", i_d, i_o)
        dones.append(np.array(d_o))
    return np.array(dones)


def run_lengths(L):
    return [L, 1, L + 4, 2 * L]


def set_load_change(n):
    """the masked set_load of the per-env configuration: envs on both sides of every split move to another load"""
    mask = np.array([(i % 3 == 1) or i == n - 1 for i in range(n)], np.uint8)
    return [95.5 + 9.0 * (n - 1 - i) for i in range(n)], mask  # (the order reversed; no value of _loads among them)


def run_checked(dev, ora, cfg, form, plan, steps, tag, label=None):
    """One device-resident run of `steps` steps on the batch and on the oracle.  form / plan None: whatever route the batch takes
    (the one-wavefront kernels, QoSConstrainedRA); else the run asserts the plan it was made under — parts, split point and launch
    length from orl_debug_run_plan in this environment, at least ceil(steps / chunk) launches — and the form that ran.  Every env is
    compared afterwards."""
    label = label or "run of %d steps" % steps
    what = "%s, %s" % (tag, label)
    if plan is not None:
        p = assert_plan(dev, cfg, plan, steps, what)
    st = dev.run(cfg.policy, steps)
    if plan is not None:
        assert st.launches >= math.ceil(steps / chunk_of(plan, steps_per_episode(cfg))), (what, st.launches, p)
        assert [nm for nm, _ in st.kernels()] == ["k_persist"], what
        assert_form_ran(dev, cfg, form, what)
    ora.run(cfg.policy, steps)
    compare(dev, ora, cfg, plan or ("128", 1), tag, label)
    return st


def drive_case(dev, ora, cfg, form, plan, tag):
    """The sequence of one case: runs of L, 1, L + 4 and 2 L steps with a few host steps and — per-env loads — a masked set_load
    between them, everything compared after every piece.  -> the last snapshot of the batch."""
    lengths = run_lengths(steps_per_episode(cfg))
    shown = plan or ("128", 1)
    compare(dev, ora, cfg, shown, tag, "at construction")
    for k, steps in enumerate(lengths):
        if k == 2:
            host_steps(dev, ora, cfg, 3, tag)
            compare(dev, ora, cfg, shown, tag, "3 host steps")
        if k == 3 and cfg.loads:
            load, mask = set_load_change(dev.num_envs)
            dev.set_load(load=load, mask=mask)
            ora.set_load(load, mask)
            compare(dev, ora, cfg, shown, tag, "masked set_load")
        run_checked(dev, ora, cfg, form, plan, steps, tag, "run %d of %d steps" % (k, steps))
    return snapshot(dev, cfg.fam, dev.num_envs)


def drive_oracle(ora, cfg):
    """the pieces of drive_case on the oracle alone (tests/test_run_plans.py: what its trajectories must show)"""
    lengths = run_lengths(steps_per_episode(cfg))
    for k, steps in enumerate(lengths):
        if k == 2:
            for _ in range(3):
                ora.step(ora.policy(cfg.policy), auto_reset=True)
        if k == 3 and cfg.loads:
            ora.set_load(*set_load_change(ora.n))
        ora.run(cfg.policy, steps)


# ---- the episode log ------------------------------------------------------------------------------------------------------
SMALL_CAP = 2
GUARD = -77


def arm_log(dev, capacity):
    dev._ck(dev.lib.orl_batch_episode_log(dev._h, int(capacity)))


def read_log(dev, capacity):
    """(counts[n], accepted[n][capacity]) — and, QoSConstrainedRA, rewards[n][capacity] — read into buffers with a guard row behind
    them, which must come back untouched"""
    n = dev.num_envs
    counts = np.full(n + 1, GUARD, np.int32)
    acc = np.full((n + 1, capacity), GUARD, np.int32)
    dev._ck(dev.lib.orl_batch_get_episode_log(dev._h, counts.ctypes.data, acc.ctypes.data))
    assert counts[n] == GUARD and (acc[n] == GUARD).all()
    rew = None
    if dev.ENV_TYPE == 4:
        rew = np.full((n + 1, capacity), float(GUARD), np.float64)
        dev._ck(dev.lib.orl_batch_get_episode_rewards(dev._h, rew.ctypes.data))
        assert (rew[n] == float(GUARD)).all()
        rew = rew[:n]
    return counts[:n], acc[:n], rew


def expected_log(ora, capacity):
    """the log a batch armed with `capacity` when the ledger was started must hold: counts goes on counting, a row holds the
    first `capacity` episodes and zeros behind them"""
    counts = np.array([len(e) for e in ora.episodes], np.int32)
    acc = np.zeros((ora.n, capacity), np.int32)
    rew = np.zeros((ora.n, capacity), np.float64)
    for i in range(ora.n):
        k = min(capacity, len(ora.episodes[i]))
        acc[i, :k] = ora.episodes[i][:k]
        rew[i, :k] = ora.episode_rewards[i][:k]
    return counts, acc, rew


def compare_log(dev, ora, capacity, tag):
    chk = _exact_bits(tag)
    counts, acc, rew = read_log(dev, capacity)
    e_counts, e_acc, e_rew = expected_log(ora, capacity)
    chk(0, "episode counts", counts, e_counts)
    chk(0, "accepted per episode", acc, e_acc)
    if rew is not None:
        chk(0, "reward sum per episode", rew, e_rew)
    return e_counts


# ---- resets between runs ----------------------------------------------------------------------------------------------------
def reset_masks(n=20):
    """a mask with envs on both sides of the split of a 20-env batch, and exactly the second half"""
    first, _second = BATCHES[n]
    both = np.array([i in (2, 7, first - 1, first, n - 1) for i in range(n)], np.uint8)
    second = np.array([i >= first for i in range(n)], np.uint8)
    return both, second
