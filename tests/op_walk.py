"""Walks of interleaved state-changing calls on one batch, and the model that replays them on the CPU oracle — shared by
tests/test_op_walk.py (CPU: the model is exact on the oracle itself, the walks cover every ordered pair of kinds and reach what they
exist for) and tests/test_op_walk_gpu.py (the device under every step route).  Helper module, no tests.

A walk is BUILT, not drawn: the order of its state-changing ops is a piece of an Eulerian circuit of the complete directed graph
with loops over the kinds, so that over a family's walks every kind is immediately followed by every kind; only an op's arguments
(masks, seeds, loads, run lengths, which actions are replaced by random ones) come from np.random.default_rng.  Between the ops sit
queries, which must leave the state as it was; they rotate per kind, so that every query follows every kind.  An agent's actions are
those of the family's agent of tests/slot_agent.py (step_agent: RMSA, RWA, RMCSA) or uniformly random over the action space, column
by column, reject and busy choices included (step_async, and step_agent of DeepRMSA and QoSConstrainedRA, whose action is one integer).

The first seed() of a batch adds every env's second stream to its state, and a snapshot from before it is refused afterwards
(envs.set_state).  So a walk is either "fresh" (no seed op; three per family, together the whole circuit over the ten other kinds —
the only walks the device-resident loop forms run unreduced, since a reseeded batch of every family but RWA runs on the per-env kernel)
or opens with seed(mask = all zeros): "seeded" (seed before and after every other kind) and "named" (the sequences of the issue:
a copy into an env a masked full reset has just emptied, then set_load on it, then three launches of one step; a restore of a
snapshot from before an episode end, made after step_async; a reseed of the source between two copies).

The model keeps one oracle env (an OracleBatch of one env) per batch env, the env's current rates, and the list of entries the env
has seen since construction: ("make", seed), ("reset", full), ("seed", s), ("step", action), ("run", policy, n), ("rates", load,
holding time).  copy_envs gives the destination a copy of the source's list; set_state puts every list back as it stood at the snapshot
(cutting it to the snapshot's length would not do once a copy has replaced the list in between); in both cases the oracle env is
rebuilt by replaying its list from construction.  Rates are configuration: they do not travel with a copy or a restore, so the
rebuilt env gets its own current rates back as one more entry.  copy_envs(keep_rng=True) cannot be modelled by replay — the
destination keeps the position of its own streams — and stays with tests/test_copy_envs_gpu.py.

Two more walks per family, the "view walks" (further down), put the device choosers, the block table and the release horizons into
the same scheme: as queries, and — "step_device" — as a stepping kind whose action the device chose and left in its actions buffer.
The model restates the chooser's answer from the oracle's state and steps the oracle with it; the entry it records is a plain step."""
import functools
from collections import namedtuple

import numpy as np

from tests import slot_agent

TOPO = "nsfnet_chen"
KINDS = ("run", "step_heur", "step_agent", "policy_step", "step_async", "reset_soft", "reset_full", "seed", "set_load", "set_state",
         "copy_envs")
FRESH_KINDS = tuple(k for k in KINDS if k != "seed")
STEPPING = ("run", "step_heur", "step_agent", "policy_step", "step_async")
HEURISTIC = ("run", "step_heur", "policy_step")  # the action is a heuristic's: a service it does not place is blocked by the network
RUN_LENGTHS = (1, 2, 7, 20, 37)
MASKS = ("none", "one", "group", "half_group", "all_but_one")
MAX_OPS, MAX_STEPS = 45, 300
QOS = "QoSConstrainedRA"

Family = namedtuple("Family", "name fam kw dev_kw batch policy policies")


def _from_case(name, case, episode_length, batch):
    c = slot_agent.CASE_BY_NAME[case]
    return Family(name, c.fam, dict(c.kw, episode_length=episode_length), dict(c.dev_kw), batch, slot_agent.LOOP_POLICY[c.fam],
                  slot_agent.SAMPLED_POLICIES[c.fam])


# One configuration per family, at row-width edges, from the cases tests/slot_agent.py and tests/test_copy_envs_gpu.py use (the
# specialisation library of a configuration does not depend on episode_length).  27 envs: the fourth group of 8 is incomplete.
FAMILIES = {f.name: f for f in [
    _from_case("rmsa", "rmsa_s129", 22, 40),
    _from_case("deeprmsa", "deep_s129_j4", 21, 27),
    _from_case("rwa", "rwa_s65", 20, 40),
    # 65 wavelengths never run out in a walk (NO_NETWORK_BLOCKING below): the same family where they do, 27 envs
    Family("rwa_s8", "RWA", dict(load=400, num_spectrum_resources=8, allow_rejection=True, mean_service_holding_time=10.0, episode_length=20), {},
           27, "SAP_LF", slot_agent.SAMPLED_POLICIES["RWA"]),
    _from_case("rmcsa", "rmcsa_c7_s65", 23, 27),
    Family("qos", QOS, dict(load=1000, mean_service_holding_time=25, episode_length=25, num_spectrum_resources=12, num_service_classes=3,
                            classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0], allow_rejection=True), {}, 40,
           "SAP_FF", ("SP_FF", "SAP_FF", "LLP_FF")),
]}
# Loads (QoSConstrainedRA and rwa_s8: units and wavelengths per link too) are chosen so that the network itself blocks within a walk: a
# HEURISTIC finds no room for a service.  With 65 wavelengths RWA cannot get there at any load: every node of NSFNET has at least 3
# links, a step adds at most one service, so the 5 paths of a pair all hold a full link after 3 * 65 = 195 services through one node at
# the earliest — a walk has 300 steps over 14 nodes, with resets and restores in between.
NO_NETWORK_BLOCKING = ("rwa",)
PAIR_FAMILIES = tuple(n for n, case in (("rmsa", "rmsa_s129"), ("rmcsa", "rmcsa_c7_s65")) if case in slot_agent.PAIR_CASES)


def seeds_of(f):
    return [7000 + 11 * i + 3 * len(f.name) for i in range(f.batch)]


def base_rates(f):
    """(load, mean holding time) the configuration is constructed with (DeepRMSA: load = holding time / inter-arrival time)"""
    mht = f.kw["mean_service_holding_time"]
    return (mht / f.kw["mean_service_inter_arrival_time"] if f.fam == "DeepRMSA" else f.kw["load"]), mht


def capacity_needed(load):
    """the pending releases the library gives an env at `load` Erlang room for (include/orl.h, event_capacity == 0)"""
    return int(load + 10.0 * np.sqrt(load) + 64.0)


def load_range(f):
    """the loads set_load may ask for: from half the configuration's load up to the largest its event capacity has room for"""
    load, _ = base_rates(f)
    cap, hi = capacity_needed(load), load
    while capacity_needed(hi + 1.0) <= cap:
        hi += 1.0
    return 0.5 * load, float(hi)


def action_bounds(f):
    """exclusive upper bound per action column (envs.action_bounds; DeepRMSA: k * j + 1, the reject action included)"""
    K, S = 5, f.kw["num_spectrum_resources"]
    rej = 1 if f.kw.get("allow_rejection") else 0
    return {"RMSA": (K + 1, S + 1), "DeepRMSA": (K * f.kw.get("j", 1) + 1,), "RWA": (K + rej, S + rej),
            "RMCSA": (K + 1, 6 + 1, f.kw.get("num_spatial_resources", 1) + 1, S + 1), QOS: (K + rej,)}[f.fam]


AGENTS = {"RMSA": "rmsa_s129", "RWA": None, "RMCSA": "rmcsa_c7_s65"}  # family -> the case whose tables its agent reads (RMCSA)


def agent_actions(f, slots_packed, services, t, seed):
    """The actions of the family's agent of tests/slot_agent.py on the oracle's state: boundary-seeking provisions, and what no
    heuristic does — RMSA: a block that ends at S; RWA: busy pairs; RMCSA: high cores, other modulations, every kind of refused
    and partly rejecting action."""
    from tests.mask_restate import row_words, unpack_slots

    topo, rng = slot_agent.topology(), np.random.RandomState(seed)
    S, C = f.kw["num_spectrum_resources"], f.kw.get("num_spatial_resources", 1)
    avail = unpack_slots(slots_packed, C * topo.n_links, S, row_words(S))
    if f.fam == "RMSA":
        return slot_agent.agent_actions(avail, services, topo, t, rng, S)
    if f.fam == "RWA":
        return slot_agent.rwa_agent_actions(avail, services, topo, t, rng, S)[0]
    tab = slot_agent.rmcsa_tables(AGENTS[f.fam])
    return slot_agent.rmcsa_agent_actions(avail.reshape(len(services), C, topo.n_links, S), services, topo, tab, t, rng, S, C)[0]


def queries_of(f):
    """the query kinds of the family, in the order they rotate"""
    q = ["get_state", "rates", "pending"] + ["policy:" + p for p in f.policies]
    if f.fam == QOS:
        return q + ["matrix_observation_with_paths"]
    q += {"RMSA": ["mask:joint", "mask:path"], "RWA": ["mask:joint", "mask:path"], "DeepRMSA": ["mask:joint", "observation"],
          "RMCSA": ["mask:path_modulation", "mask:core_slot", "complete_actions"]}[f.fam]
    return q + ["path_features", "link_features", "matrix_observation"]


# ---- the order of the ops ---------------------------------------------------------------------------------------------------
def euler_circuit(k):
    """A closed walk over nodes 0 .. k - 1 that takes every ordered pair (a, b), a == b included, exactly once: k * k + 1 nodes."""
    unused = {a: list(range(k)) for a in range(k)}
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


def cut(seq, length):
    """pieces of at most `length` items; each begins with the last item of the one before, so that no pair is lost at a cut"""
    out, lo = [], 0
    while lo < len(seq) - 1:
        out.append(seq[lo:lo + length])
        lo += length - 1
    return out


def pairs_of(kinds):
    return set(zip(kinds[:-1], kinds[1:]))


# ---- the arguments of the ops -------------------------------------------------------------------------------------------------
class _Builder:
    """Draws the arguments of a family's ops; the counters that make the variants rotate run on over the family's walks."""

    def __init__(self, f, seed, segments=None):
        self.f, self.n = f, f.batch
        self.rng = np.random.default_rng(seed)
        self.segments = segments or ((0, f.batch),)  # copies stay inside a segment (the shards of a sharded batch)
        self.count = {}
        self.qcount = {k: 0 for k in KINDS}
        self.queries = queries_of(f)

    def turn(self, what, n):
        c = self.count.get(what, 0)
        self.count[what] = c + 1
        return c % n

    def mask(self, which=None):
        n, rng = self.n, self.rng
        which = MASKS[self.turn("mask", len(MASKS))] if which is None else which
        if which == "none":
            return None
        m = np.zeros(n, np.uint8)
        if which == "one":
            m[rng.integers(n)] = 1
        elif which == "all_but_one":
            m[:] = 1
            m[rng.integers(n)] = 0
        else:
            g, h = int(rng.integers(n // 8)), int(rng.integers(2))  # a complete group, or one of its halves
            if which == "group":
                m[8 * g:8 * g + 8] = 1
            else:
                m[8 * g + 4 * h:8 * g + 4 * h + 4] = 1
        return m

    def whole_groups(self):
        return [g for g in range(self.n // 8) if any(lo <= 8 * g and 8 * g + 8 <= hi for lo, hi in self.segments)]

    def segment_of(self, i):
        return next((lo, hi) for lo, hi in self.segments if lo <= i < hi)

    def copy(self, walk_state):
        rng = self.rng
        variant = ("fan_out", "pairs", "chain")[self.turn("copy", 3)]
        if variant == "chain" and not walk_state["copied"]:
            variant = "pairs"
        if variant == "fan_out":  # one env into a whole group of 8
            g = int(rng.choice(self.whole_groups()))
            dst = np.arange(8 * g, 8 * g + 8)
            lo, hi = self.segment_of(8 * g)
            src = int(rng.choice(np.setdiff1d(np.arange(lo, hi), dst)))
            src = np.full(8, src)
        elif variant == "pairs":  # single pairs across groups
            src, dst = [], []
            for _ in range(3):
                s = int(rng.integers(self.n))
                lo, hi = self.segment_of(s)
                cand = [d for d in range(lo, hi) if d // 8 != s // 8 and d not in dst and d not in src]
                d = int(rng.choice(cand))
                if s not in dst:
                    src.append(s)
                    dst.append(d)
            src, dst = np.array(src), np.array(dst)
        else:  # the source was itself a destination earlier
            s = int(walk_state["copied"][-1])
            lo, hi = self.segment_of(s)
            src, dst = np.array([s]), np.array([int(rng.choice(np.setdiff1d(np.arange(lo, hi), [s])))])
        walk_state["copied"].extend(int(d) for d in dst)
        return dict(kind="copy_envs", src=src, dst=dst, variant=variant)

    def set_load(self, mask="rotate"):
        n, rng = self.n, self.rng
        lo, hi = load_range(self.f)
        variant = self.turn("set_load", 4)
        per_env = variant in (2, 3)
        load = np.round(rng.uniform(lo, hi, n), 1) if per_env else float(np.round(rng.uniform(lo, hi), 1))
        mht = rng.choice([5.0, 7.5, 10.0, 20.0, 25.0], n) if per_env else float(rng.choice([5.0, 7.5, 10.0, 20.0, 25.0]))
        return dict(kind="set_load", load=None if variant == 1 else load, mht=None if variant in (0, 2) else mht,
                    mask=self.mask() if isinstance(mask, str) else mask)

    def op(self, kind, walk_state, **fixed):
        n, rng, f = self.n, self.rng, self.f
        if kind == "run":
            return dict(kind=kind, n=fixed.get("n", RUN_LENGTHS[self.turn("run", len(RUN_LENGTHS))]), policy=f.policy)
        if kind in ("step_heur", "policy_step"):
            return dict(kind=kind, policy=f.policies[self.turn("policy", len(f.policies))])
        if kind == "step_agent" and f.fam in AGENTS:  # the family's agent of tests/slot_agent.py, its goals rotating with t
            return dict(kind=kind, policy=f.policy, agent_t=self.turn("agent_t", 1 << 30), agent_seed=int(rng.integers(1 << 31)))
        if kind in ("step_agent", "step_async"):  # every column of every env: with probability 0.4 uniform over its range
            return dict(kind=kind, policy=f.policy, pick=rng.random((n, 4)) < 0.4, u=rng.random((n, 4)))
        if kind in ("reset_soft", "reset_full"):
            return dict(kind=kind, mask=fixed["mask"] if "mask" in fixed else self.mask())
        if kind == "seed":
            return dict(kind=kind, seeds=[int(s) for s in rng.integers(0, 2 ** 31, n)], mask=fixed["mask"] if "mask" in fixed else self.mask())
        if kind == "set_load":
            return self.set_load(fixed.get("mask", "rotate"))
        if kind == "set_state":
            return dict(kind=kind, snapshot=fixed.get("snapshot", int(rng.integers(walk_state["snapshots"]))))
        assert kind == "copy_envs"
        if "src" in fixed:
            walk_state["copied"].extend(int(d) for d in fixed["dst"])
            return dict(kind=kind, src=np.asarray(fixed["src"]), dst=np.asarray(fixed["dst"]), variant="named")
        return self.copy(walk_state)

    def query(self, name):
        rng, f, n = self.rng, self.f, self.n
        q = dict(q=name)
        if name == "path_features":
            q["j"] = (1, 2, 4, 8)[self.turn("pf_j", 4)]
        elif name == "pending":
            q["envs"] = [int(e) for e in rng.choice(n, 3, replace=False)]
        elif name == "mask:core_slot":
            q["given"] = np.stack([rng.integers(0, 5, n), rng.integers(0, 6, n)], axis=1).astype(np.int32)
        elif name == "complete_actions":
            g = self.turn("complete", 4)
            C = f.kw["num_spatial_resources"]
            q["g"] = g
            q["given"] = np.stack([rng.integers(0, 5, n), rng.integers(0, 6, n), rng.integers(0, C, n)], axis=1).astype(np.int32)[:, :g] if g else None
        return q

    def walk(self, name, kinds, fresh, fixed=None):
        """-> Walk: after the opening (seed(mask = 0) unless fresh) a snapshot; after every op two queries, rotating per kind"""
        fixed = fixed or {}
        state = dict(snapshots=0, copied=[])
        items = []
        if not fresh:
            items.append(("op", self.op("seed", state, mask=np.zeros(self.n, np.uint8))))
        items.append(("q", self.query("get_state")))
        state["snapshots"] = 1
        for i, kind in enumerate(kinds):
            items.append(("op", self.op(kind, state, **fixed.get(i, {}))))
            for _ in range(2):
                qn = self.queries[self.qcount[kind] % len(self.queries)]
                self.qcount[kind] += 1
                items.append(("q", self.query(qn)))
                state["snapshots"] += qn == "get_state"
        return Walk(name, fresh, items)


class Walk(namedtuple("Walk", "name fresh items")):
    def kinds(self):
        return [it["kind"] for what, it in self.items if what == "op"]

    def steps(self):
        return sum(it.get("n", 1) for what, it in self.items if what == "op" and it["kind"] in STEPPING + ("step_device",))


def _seeded_kinds():
    """seed before and after every other kind, and after itself; then stepping, so that the walk crosses episode ends"""
    kinds = []
    for k in FRESH_KINDS:
        kinds += ["seed", k]
    return kinds + ["seed", "seed", "run", "set_state", "run", "copy_envs", "run", "reset_soft", "run"]


def _named(b):
    n = b.n
    lo, hi = b.segments[-1]
    d, s, d1, d2 = lo + 1, hi - 1, lo + 2, lo + 3  # (one segment; s in another group than d)
    one = lambda i: np.array([j == i for j in range(n)], np.uint8)
    kinds = ["run", "run", "run", "copy_envs",                                    # a copy out of a network 111 steps in use
             "run", "reset_full", "copy_envs", "set_load", "run", "run", "run",  # into the emptied env d, then three launches of one step
             "run", "step_async", "set_state",                                    # back before an episode end, after step_async
             "run", "copy_envs", "seed", "copy_envs", "run", "step_agent", "run"]  # the source reseeded between two copies
    fixed = {0: dict(n=37), 1: dict(n=37), 2: dict(n=37),
             4: dict(n=20), 5: dict(mask=one(d)), 6: dict(src=[s], dst=[d]), 7: dict(mask=one(d)), 8: dict(n=1), 9: dict(n=1), 10: dict(n=1),
             11: dict(n=37), 13: dict(snapshot=0), 14: dict(n=7), 15: dict(src=[s], dst=[d1]), 16: dict(mask=one(s)),
             17: dict(src=[s], dst=[d2]), 18: dict(n=20), 20: dict(n=37)}
    return kinds, fixed


@functools.lru_cache(maxsize=None)
def walks_of(name, segments=None):
    """the family's walks: fresh0 .. fresh2 (the circuit over the ten kinds but seed), seeded, named"""
    f = FAMILIES[name]
    b = _Builder(f, 1000 + len(name) + 17 * f.batch, segments)
    order = list(b.rng.permutation(len(FRESH_KINDS)))
    circuit = [FRESH_KINDS[order[v]] for v in euler_circuit(len(FRESH_KINDS))]
    warm = {0: dict(n=37), 1: dict(n=37)}  # every walk begins with two long runs: the ops that follow meet a network in use
    walks = [b.walk("fresh%d" % i, ["run", "run"] + piece, True, warm) for i, piece in enumerate(cut(circuit, 35))]
    walks.append(b.walk("seeded", ["run", "run"] + _seeded_kinds(), False, warm))
    kinds, fixed = _named(b)
    walks.append(b.walk("named", kinds, False, fixed))
    return tuple(walks)


def walk_of(name, walk, segments=None):
    return next(w for w in walks_of(name, segments) + (view_walks_of(name, segments) if walk in VIEW_WALK_NAMES else ()) if w.name == walk)


WALK_NAMES = ("fresh0", "fresh1", "fresh2", "seeded", "named")


# ---- the device choosers, the block table and the release horizons inside the walks ---------------------------------------------------
# Two more walks per family that has them (every family but QoSConstrainedRA), built by a builder of their own — its own generator
# and counters, so that the five walks above stay what they are (tests/test_op_walk.py pins their digests).  The five newer device calls
# are QUERIES here (view_queries_of: one after every op, rotating per preceding kind, beside the two of the rotation above), and the
# choosers that leave an action on the device also make a stepping kind: "step_device" — the chooser call(s) with fetch=False, then
# step(None) or step_async(None) + step_wait().  A walk is  run 37, run 37, F, F,  then  k, F  for every kind k (so that F immediately
# precedes and follows every kind, a device-resident run and itself included), then the kinds again without F until every view query
# has followed every kind.  F = step_device; on DeepRMSA, which has no chooser that writes an action, F = step_agent.
VIEW_WALK_NAMES = ("views_fresh", "views_seeded")
ENV_TYPE = {"RMSA": 0, "DeepRMSA": 1, "RWA": 2, "RMCSA": 3}
HORIZON_J, TABLE_J = (1, 3, 8), (1, 2, 4, 8)
SPECTRUM_VARIANTS = ("route_spectrum", "assign_host", "policy_assign", "select_host", "select_buffer")
CORE_VARIANTS = ("route_cores_host", "complete_route_cores", "select_host", "select_buffer")
PAIRS_PER_QUERY = 3  # (rule, route) pairs one route_spectrum / route_cores query asks: a walk has fewer such queries than there are pairs
FIXED = "fixed"      # RMCSA modulation: route_cores_cases.fixed_modulation of the state the call is made on


def view_queries_of(f):
    """the view query kinds of the family, in the order they rotate"""
    if f.fam == QOS:
        return []
    q = ["release_horizons", "block_table"]
    if f.fam in ("RMSA", "RWA"):
        q += ["assign_spectrum", "route_spectrum", "select_blocks"]
    if f.fam == "RMCSA":
        q += ["route_cores", "select_blocks"]
    return q


def chooser_variants_of(f):
    """the ways the family's step_device chooses its action on the device"""
    return {"RMSA": SPECTRUM_VARIANTS, "RWA": SPECTRUM_VARIANTS, "RMCSA": CORE_VARIANTS}.get(f.fam, ())


def view_walk_names(name):
    return VIEW_WALK_NAMES if view_queries_of(FAMILIES[name]) else ()


def rule_route_pairs(f):
    from tests import route_cores_restate, route_restate

    m = route_cores_restate if f.fam == "RMCSA" else route_restate
    return [(rule, route) for rule in m.RULES for route in m.ROUTES]


class Restated:
    """The restatements of the choosers and the block table on ONE state (slot maps and pending services, the oracle's or the device's
    read-back), each prepared once however many queries of the state ask for it."""

    def __init__(self, f, slots_packed, services):
        from tests.rmcsa_mask_restate import unpack_cores

        self.f, self.topo, self.services = f, slot_agent.topology(), services
        self.S, self.C = f.kw["num_spectrum_resources"], f.kw.get("num_spatial_resources", 1)
        self.K, self.n = self.topo.k_paths, len(services)
        self.env_type = ENV_TYPE[f.fam]
        self.avail = unpack_cores(slots_packed, self.C, self.topo.n_links, self.S)  # bool [n, C, links, S]
        self.tab = slot_agent.rmcsa_tables(AGENTS[f.fam]) if f.fam == "RMCSA" else None
        self._made = {}

    def once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    def modulation(self, mod):
        from tests import route_cores_cases

        if mod != FIXED:
            return mod
        return self.once("fixed", lambda: int(route_cores_cases.fixed_modulation(self.services, self.topo, self.tab)))

    # -- RMSA / RWA
    def prep(self):
        from tests import assign_restate

        return self.once("prep", lambda: assign_restate.Prepared(self.env_type, self.avail[:, 0], self.services, self.topo, self.K, self.S))

    def assign(self, rule, paths):
        from tests import assign_restate

        return assign_restate.assign(self.prep(), rule, 0 if paths is None else 1, paths)

    def route_spectrum(self, rule, route):
        """(action, table)"""
        from tests import route_restate

        links = self.once("links", lambda: route_restate.Links(self.avail[:, 0], self.services, self.topo))
        tab = self.once(("route_table", rule), lambda: route_restate.table(self.prep(), links, rule))
        return route_restate.route(tab, route, self.K, self.S), tab

    # -- RMCSA
    def pv(self):
        from tests.rmcsa_mask_restate import prov_all

        return self.once("pv", lambda: prov_all(self.avail, self.services, self.topo, self.tab))

    def complete(self, g, given):
        from tests import complete_restate

        return complete_restate.complete(self.pv(), self.services, self.topo, self.tab, g, given)

    def route_cores(self, rule, route, given, mod):
        """(action, table); given: int [n, g] or None; mod: None, FIXED or a modulation"""
        from tests import route_cores_restate as rc

        mod = self.modulation(mod)
        prep = self.once(("core_prep", mod), lambda: rc.Prepared(self.avail, self.services, self.topo, self.tab, modulation=mod, pv=self.pv()))
        tab = self.once(("core_table", rule, mod), lambda: rc.table(prep, rule))
        return rc.route(prep, tab, route, given), tab

    # -- block actions
    def rows(self, mod=None):
        from tests import block_restate

        mod = self.modulation(mod)
        return self.once(("rows", mod), lambda: block_restate.Rows(self.env_type, self.avail, self.services, self.topo, self.tab, mod))

    def block_table(self, j, mod=None):
        """(table, mask)"""
        from tests import block_restate

        rows = self.rows(mod)
        return block_restate.table(rows, j), block_restate.mask(rows, j, bool(self.f.kw.get("allow_rejection")))

    def select(self, it):
        """(indices, actions) of a select_blocks query or step_device variant: the indices are drawn on THIS state"""
        from tests import block_restate

        rows = self.rows(it["mod"])
        idx = block_restate.draw_indices(rows, it["j"], np.random.default_rng(it["seed"]))
        return idx, block_restate.select(rows, it["j"], idx, it["placement"])

    def chosen(self, op, policy):
        """-> (the restated action int32 [n, 4] of a step_device op, what the device side needs beside the op: indices, modulation);
        policy(name) -> the heuristic's actions on the same state"""
        v, extra = op["variant"], {}
        if v == "route_spectrum":
            a = self.route_spectrum(op["rule"], op["route"])[0]
        elif v == "assign_host":
            a = self.assign(op["rule"], op["paths"])
        elif v == "policy_assign":  # column 0 of the heuristic's action is the path
            a = self.assign(op["rule"], policy(op["policy"])[:, 0])
        elif v in ("select_host", "select_buffer"):
            extra["indices"], a = self.select(op)
            extra["modulation"] = self.modulation(op["mod"])
        elif v == "route_cores_host":
            a = self.route_cores(op["rule"], op["route"], op["given"], op["mod"])[0]
            extra["modulation"] = self.modulation(op["mod"])
        else:
            assert v == "complete_route_cores"  # columns 0 and 2 of the completion: (path, core)
            done = self.complete(2, op["given"])
            a = self.route_cores(op["rule"], op["route"], done[:, [0, 2]], None)[0]
        return a.astype(np.int32), extra

    @property
    def reject(self):
        return (self.K, len(self.tab["lmax_xt"]), self.C, self.S) if self.f.fam == "RMCSA" else (self.K, self.S, 0, 0)


class _ViewBuilder(_Builder):
    """The arguments of the view walks: a generator and counters of its own"""

    def __init__(self, f, seed, segments=None):
        super().__init__(f, seed, segments)
        self.qcount["step_device"] = 0
        self.views = view_queries_of(f)
        self.vcount = {k: 0 for k in self.qcount}
        self.pairs = rule_route_pairs(f)
        self.filler = "step_device" if chooser_variants_of(f) else "step_agent"

    def mod(self, what):
        return (None, FIXED)[self.turn(what, 2)] if self.f.fam == "RMCSA" else None

    def given(self, what):
        """a prefix of route_cores_cases.draw_given, g = 0, 1, 2 in rotation (g = 0: None)"""
        from tests import route_cores_cases

        g = self.turn(what, 3)
        return route_cores_cases.draw_given(self.n, 5, self.f.kw["num_spatial_resources"], g, shift=self.turn(what + "_shift", 1 << 30)) if g else None

    def host_paths(self):
        """a path per env in [0, k); k itself, a negative one and an in-range one at three envs drawn for it"""
        p = self.rng.integers(0, 5, self.n).astype(np.int32)
        at = self.rng.choice(self.n, 3, replace=False)
        p[at] = (5, -1 - int(self.rng.integers(3)), int(self.rng.integers(5)))
        return p

    def blocks(self, what):
        c = self.turn(what, 1 << 30)  # every (placement, modulation) pair, j moving against them
        return dict(j=TABLE_J[(c // 4 + c) % 4], placement=("first", "last")[c % 2], mod=(None, FIXED)[(c // 2) % 2] if self.f.fam == "RMCSA" else None,
                    seed=int(self.rng.integers(1 << 31)))

    def op(self, kind, walk_state, **fixed):
        if kind == "set_state" and "snapshot" not in fixed:
            fixed["snapshot"] = walk_state["snapshots"] - 1
        if kind != "step_device":
            return super().op(kind, walk_state, **fixed)
        from tests import assign_restate

        f, variants = self.f, chooser_variants_of(self.f)
        c = self.turn("step_device", 1 << 30)  # every variant under both forms of the step
        v = variants[c % len(variants)]
        op = dict(kind=kind, variant=v, form=("step", "step_async")[(c // len(variants)) % 2], policy=f.policy)
        if v in ("route_spectrum", "route_cores_host", "complete_route_cores"):
            op["rule"], op["route"] = self.pairs[(4 * self.turn("sd_pair", 1 << 30)) % len(self.pairs)]  # (4: coprime to 21 and 25)
        if v in ("assign_host", "policy_assign"):
            op["rule"] = assign_restate.RULES[self.turn("sd_rule", len(assign_restate.RULES))]
        if v == "assign_host":
            op["paths"] = self.host_paths()
        elif v == "policy_assign":
            op["policy"] = f.policies[self.turn("sd_policy", len(f.policies))]
        elif v in ("select_host", "select_buffer"):
            op.update(self.blocks("sd_blocks"))
        elif v == "route_cores_host":
            op["given"], op["mod"] = self.given("sd_given"), self.mod("sd_mod")
        elif v == "complete_route_cores":
            op["given"] = np.stack([self.rng.integers(0, 5, self.n), self.rng.integers(0, 6, self.n)], axis=1).astype(np.int32)
        return op

    def view_query(self, name):
        from tests import assign_restate

        q = dict(q=name)
        if name == "release_horizons":
            q["j"], q["mod"] = HORIZON_J[self.turn("rh_j", 3)], self.mod("rh_mod")
        elif name == "block_table":
            c = self.turn("bt", 1 << 30)
            q["j"], q["mod"] = TABLE_J[c % 4], (None, FIXED)[(c // 4) % 2] if self.f.fam == "RMCSA" else None
        elif name == "assign_spectrum":
            q["rule"] = assign_restate.RULES[self.turn("as_rule", len(assign_restate.RULES))]
            q["source"] = ("none", "host", "buffer")[self.turn("as_source", 3)]
            q["paths"] = None if q["source"] == "none" else self.host_paths()
        elif name in ("route_spectrum", "route_cores"):
            c = self.turn("pairs", 1 << 30)
            q["pairs"] = [self.pairs[(PAIRS_PER_QUERY * c + i) % len(self.pairs)] for i in range(PAIRS_PER_QUERY)]
            if name == "route_cores":
                q["given"], q["mod"] = self.given("rc_given"), self.mod("rc_mod")
        else:
            assert name == "select_blocks"
            q.update(self.blocks("sb"))
        return q

    def walk(self, name, kinds, fresh, fixed=None):
        """as _Builder.walk, with one query of the view rotation after the two of the other"""
        w = super().walk(name, kinds, fresh, fixed)
        items, last = [], None
        for k, (what, it) in enumerate(w.items):
            items.append((what, it))
            if what == "op":
                last = it["kind"]
            closes = k + 1 == len(w.items) or w.items[k + 1][0] == "op"
            if what == "q" and closes and last is not None and not (last == "seed" and k == 1):  # (not after the opening snapshot)
                items.append(("q", self.view_query(self.views[self.vcount[last] % len(self.views)])))
                self.vcount[last] += 1
        return Walk(name, fresh, items)


def _view_kinds(b, fresh):
    """-> (kinds, fixed) of a view walk"""
    n = b.n
    F, Q = b.filler, len(b.views)
    kinds = FRESH_KINDS if fresh else FRESH_KINDS + ("seed",)
    first = ["run", "run", F, F]
    fixed = {0: dict(n=37), 1: dict(n=37)}
    for k in kinds:
        first += [k, F]
    again = []
    if fresh:  # twice more without the filler: with the seeded walk's two, five of every kind
        again = list(kinds) * 2
    else:      # once more — "run" closes the walk instead —, and seed until it has been followed by every view query
        rest = [k for k in kinds if k not in ("run", "seed")]
        for i, k in enumerate(rest):
            again += [k] + (["seed"] if i % 2 == 0 and again.count("seed") < max(Q - 1, 1) else [])
        again += ["run"] * 4  # across episode ends
    seq = first + again
    at = lambda kind: [i for i, k in enumerate(seq) if k == kind]
    # the first restore goes back to the walk's first snapshot, across episode ends; the later ones to the latest, which loses least
    fixed[at("set_state")[0]] = dict(snapshot=0)
    # the first resets by a mask that selects some envs and spares others
    fixed[at("reset_soft")[0]] = dict(mask=b.mask("group"))
    fixed[at("reset_full")[0]] = dict(mask=b.mask("half_group"))
    if not fresh:
        for i in at("run")[-4:]:
            fixed[i] = dict(n=20)
    return seq, fixed


@functools.lru_cache(maxsize=None)
def view_walks_of(name, segments=None):
    """the family's view walks: views_fresh (no seed op), views_seeded (opens with seed(mask = 0); seed among the kinds)"""
    f = FAMILIES[name]
    if not view_queries_of(f):
        return ()
    b = _ViewBuilder(f, 5000 + len(name) + 17 * f.batch, segments)
    walks = []
    for wname, fresh in zip(VIEW_WALK_NAMES, (True, False)):
        kinds, fixed = _view_kinds(b, fresh)
        walks.append(b.walk(wname, kinds, fresh, fixed))
    return tuple(walks)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def lambdas(load, mht):
    """(lambda_arrival, lambda_holding) as set_load derives them (optical_network_env.py:92-94, rmsa_env.py:548-553)"""
    miat = 1 / float(float(load) / float(mht))
    return 1 / miat, 1 / float(mht)


@functools.lru_cache(maxsize=None)
def _tables():
    from oracle.oracle import load_topology_tables

    return load_topology_tables(TOPO)


class Model:
    """One oracle env per batch env, its list and its current rates.  apply(op) drives an op and returns what the device needs to
    make the same call and what it must answer.  ledger=True: runs are stepped on the host, so that finished episodes are counted
    (what the walks reach, tests/test_op_walk.py); a rebuild always replays a run as one oracle run."""

    def __init__(self, name, ledger=False):
        self.f = f = FAMILIES[name]
        self.n, self.ledger = f.batch, ledger
        self.bounds = action_bounds(f)
        self.rates = [base_rates(f)] * self.n
        self.lists = [[("make", s)] for s in seeds_of(f)]
        self.envs = [self.rebuild(i) for i in range(self.n)]
        self.snaps = []
        self.episodes = np.zeros(self.n, np.int64)   # finished in the env's present history (ledger); travels with the list
        self.blocked = np.zeros(self.n, bool)        # a heuristic found no room for a service of the env at some op of the walk
        self.reach = dict(copy_into_pending=0, copy_from_64=0, restore_across_episode=0, set_load_on_pending=0)
        # what the step_device ops and the view queries of the view walks reach (counted by op / query)
        self.reach.update(chooser_provisions=0, chooser_rejects=0, chooser_differs_from_loop=0, chooser_after_copy=0, chooser_after_masked_reset=0,
                          chooser_after_new_rates=0, chooser_after_restore_across_episode=0, table_row_of_0_blocks=0, table_row_of_j_blocks=0,
                          horizon_over_64_pending=0)
        self.prev = {}  # what the previous op did to some env: copy, masked_reset, new_rates, restore_across_episode

    # -- one entry on one oracle env: the only way an oracle env is ever changed
    def do(self, o, e, replay=True):
        what = e[0]
        if what == "reset":
            o.reset(full=e[1])
        elif what == "seed":
            o.seed([e[1]])
        elif what == "rates":
            o.set_load(load=e[1], mean_service_holding_time=e[2])
        elif what == "step":
            return o.step(np.array([e[1]], np.int32), auto_reset=True)
        elif what == "run":
            if replay or not self.ledger:
                o.run(e[1], e[2])
            else:
                return sum(int(o.step(o.policy(e[1]), auto_reset=True)[2][0]) for _ in range(e[2]))
        else:
            raise ValueError(what)

    def rebuild(self, i, lst=None):
        from oracle.oracle import OracleBatch

        lst = self.lists[i] if lst is None else lst
        o = OracleBatch(self.f.fam, _tables(), [lst[0][1]], **self.f.kw)
        for e in lst[1:]:
            self.do(o, e)
        return o

    def add(self, i, e):
        self.lists[i].append(e)
        out = self.do(self.envs[i], e, replay=False)
        if e[0] == "run" and out:
            self.episodes[i] += out
        return out

    def selected(self, mask):
        return range(self.n) if mask is None else [i for i in range(self.n) if mask[i]]

    def reseeded(self):
        return np.array([any(e[0] == "seed" for e in lst) for lst in self.lists])

    def policy(self, policy):
        return np.concatenate([o.policy(policy) for o in self.envs])

    def _step(self, actions):
        outs = [self.add(i, ("step", tuple(int(v) for v in actions[i]))) for i in range(self.n)]
        obs = None if outs[0][0] is None else np.concatenate([o[0] for o in outs])
        done = np.concatenate([o[2] for o in outs])
        self.episodes += done != 0
        return obs, np.concatenate([o[1] for o in outs]), done, np.concatenate([o[3] for o in outs])

    def apply(self, op):
        kind, rec = op["kind"], dict(op)
        refused = self._refused() if kind in HEURISTIC else None
        prev, self.prev = self.prev, {}
        if kind == "step_device":
            R = self.restated()
            a, extra = R.chosen(op, self.policy)
            loop = self.policy(self.f.policy).astype(np.int32)
            rec.update(extra)
            rec["actions"], rec["out"] = a, self._step(a)
            width = len(self.bounds)
            self.reach["chooser_provisions"] += bool((rec["out"][1] > 0).any())
            self.reach["chooser_rejects"] += bool((a == np.array(R.reject, np.int32)).all(axis=1).any())
            self.reach["chooser_differs_from_loop"] += bool((a[:, :width] != loop[:, :width]).any())
            for what in ("copy", "masked_reset", "new_rates", "restore_across_episode"):
                self.reach["chooser_after_" + what] += bool(prev.get(what))
        elif kind == "run":
            for i in range(self.n):
                self.add(i, ("run", op["policy"], op["n"]))
        elif kind in STEPPING:
            a = self.policy(op["policy"]).astype(np.int32)
            if "agent_t" in op:
                state = self.readback()
                a = agent_actions(self.f, state["slots_packed"], state["services"], op["agent_t"], op["agent_seed"]).astype(np.int32)
            if "pick" in op:
                for c, hi in enumerate(self.bounds):
                    a[:, c] = np.where(op["pick"][:, c], (op["u"][:, c] * hi).astype(np.int32), a[:, c])
            rec["actions"], rec["out"] = a, self._step(a)
        elif kind in ("reset_soft", "reset_full"):
            for i in self.selected(op["mask"]):
                self.add(i, ("reset", kind == "reset_full"))
            self.prev["masked_reset"] = op["mask"] is not None and 0 < int(np.sum(op["mask"])) < self.n
        elif kind == "seed":
            for i in self.selected(op["mask"]):
                self.add(i, ("seed", op["seeds"][i]))
        elif kind == "set_load":
            changed = 0
            for i in self.selected(op["mask"]):
                load, mht = self.rates[i]
                new = (load if op["load"] is None else float(np.broadcast_to(op["load"], (self.n,))[i]),
                       mht if op["mht"] is None else float(np.broadcast_to(op["mht"], (self.n,))[i]))
                changed += new != self.rates[i]  # (the env's pending service was drawn at the rates it leaves)
                self.rates[i] = new
                self.add(i, ("rates",) + new)
            self.reach["set_load_on_pending"] += changed > 0
            self.prev["new_rates"] = changed > 0
        elif kind == "set_state":
            lists, episodes = self.snaps[op["snapshot"]]
            # back across an episode end: the snapshot is the env's own past (a prefix of its list) and an episode has ended since
            own = [tuple(self.lists[i][:len(lists[i])]) == lists[i] for i in range(self.n)]
            self.prev["restore_across_episode"] = any(own[i] and self.episodes[i] > episodes[i] for i in range(self.n))
            self.reach["restore_across_episode"] += self.prev["restore_across_episode"]
            for i in range(self.n):
                if tuple(self.lists[i]) != lists[i]:
                    self.lists[i] = list(lists[i])
                    self._rebuilt(i)
            self.episodes = episodes.copy()
        else:
            assert kind == "copy_envs"
            active = self.readback()["active"]
            self.reach["copy_into_pending"] += bool((active[op["dst"]] > 0).any())
            self.reach["copy_from_64"] += bool((active[op["src"]] > 64).any())
            new = {int(d): list(self.lists[int(s)]) for s, d in zip(op["src"], op["dst"])}
            for d, lst in new.items():
                self.lists[d] = lst
                self._rebuilt(d)
            self.episodes[op["dst"]] = self.episodes[op["src"]]
            self.prev["copy"] = len(op["dst"]) > 0
        if refused is not None:
            self.blocked |= self._refused() > refused
        return rec

    def _refused(self):
        cnt = np.concatenate([o.counters() for o in self.envs])
        return cnt[:, 0] - cnt[:, 1]  # services processed and not accepted

    def _rebuilt(self, i):
        self.envs[i] = self.rebuild(i)
        self.add(i, ("rates",) + self.rates[i])

    def restated(self):
        """the restatements on the oracle's present state"""
        state = self.readback()
        return Restated(self.f, state["slots_packed"], state["services"])

    def view_reach(self, q):
        """counts what a view query of a view walk finds in the oracle's present state"""
        from tests import block_restate

        if q["q"] == "block_table":
            rows = self.restated().rows(q["mod"])
            blocks = [len(block_restate.blocks_of(rows, i, r)) for i in range(rows.n) for r in range(rows.R)]  # (a row the service cannot use: 0)
            self.reach["table_row_of_0_blocks"] += any(b == 0 for b in blocks)
            self.reach["table_row_of_j_blocks"] += any(b >= q["j"] for b in blocks)
        elif q["q"] == "release_horizons":
            self.reach["horizon_over_64_pending"] += bool((self.readback()["active"] > 64).any())

    def snapshot(self):
        self.snaps.append(([tuple(lst) for lst in self.lists], self.episodes.copy()))

    def lambdas(self):
        la, lh = zip(*(lambdas(*r) for r in self.rates))
        return np.array(la), np.array(lh)

    def readback(self, envs=None):
        """every compared quantity of every env, by the name of the batch's read-back"""
        envs = self.envs if envs is None else envs
        cat = lambda fn: np.concatenate([fn(o) for o in envs])
        out = dict(counters=cat(lambda o: o.counters()), services=cat(lambda o: o.services()), active=cat(lambda o: o.active()))
        if self.f.fam == QOS:
            out["spectrum"] = np.stack([o.spectrum(0) for o in envs])
            out["link_stats"] = np.stack([o.link_stats(0)[[0, 3]] for o in envs])
        else:
            out.update(slots_packed=cat(lambda o: o.slots_packed()), link_stats_all=cat(lambda o: o.link_stats_all()),
                       net_stats_all=cat(lambda o: o.net_stats_all()))
        if envs[0].obs_dim:
            out["observation"] = cat(lambda o: o.observation())
        return out


def drive_oracle(name, walk, ledger=True):
    """the walk on the model alone -> the model"""
    m = Model(name, ledger=ledger)
    for what, it in walk.items:
        if what == "op":
            m.apply(it)
        elif it["q"] == "get_state":
            m.snapshot()
        elif it["q"] in ("block_table", "release_horizons"):
            m.view_reach(it)
    return m
