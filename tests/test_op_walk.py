"""The walks and the model of tests/op_walk.py on the oracle alone, before any device is involved: a rebuild by replay is exact on the
oracle itself; over a family's walks every ordered pair of state-changing kinds occurs and every query kind follows every kind;
and the walks reach what they exist for (episode ends, blocking, copies into and out of busy envs, restores across an episode end,
set_load on envs whose pending service was drawn at the old rates).  tests/test_op_walk_gpu.py drives the same walks on the device.

The view walks (the device choosers as a stepping kind, the five newer device calls as queries) are held to the same, and the five
walks from before them are pinned by digest: adding the view walks changed no op, query or drawn argument of theirs."""
import functools
import hashlib

import numpy as np
import pytest

from tests import op_walk as ow
from tests.helpers import _exact_bits

FAMILY_NAMES = sorted(ow.FAMILIES)
# RMCSA: reach limits refuse about 45 % of the services whatever chooses the action (tests/slot_agent.py: acceptance 0.58 under its
# agent, the same under SAP_BM_FC_FF here), so 64 pending releases need more than 200 steps in a row without a full reset even at the
# largest load the configuration's event capacity admits: outside a walk's budget of steps
# rwa_s8: 8 wavelengths on 22 links hold 70 to 80 services when nothing more fits (76 after 111 steps of SAP_FF from construction,
# the maximum over 16 envs), and no walk leaves an env that many steps without a full reset or a restore
NO_64_PENDING = ("rmcsa", "rwa_s8")
VIEW_FAMILIES = [n for n in FAMILY_NAMES if ow.view_walk_names(n)]
CHOOSER_FAMILIES = [n for n in VIEW_FAMILIES if ow.chooser_variants_of(ow.FAMILIES[n])]
# the view walks leave most envs of rwa_s8 without a full reset or a restore for longer than the five walks above do: there some env
# does hold more than 64 pending releases at a horizon query; RMCSA stays out for the reason given above
VIEWS_NO_64_PENDING = ("rmcsa",)
# sha256 of the canonical serialisation (_feed) of walks_of(name) — fresh0, fresh1, fresh2, seeded, named: names, ops, queries and every
# drawn argument, arrays as dtype, shape and bytes — computed on the commit before the view walks were added
WALK_DIGESTS = {
    "deeprmsa": "226ee9ae922349f50057f9c5769ef0dcaff10fdd0d1409cc444dcfad9af0709d",
    "qos": "4d614e75da7496f33d820eaf7e5a516a46e826147f95ad9fb4810e29760488df",
    "rmcsa": "b234ab754a56aaab27a111edcdb7f1cd9cbb4ad88675f6ecd2044ef06b7c325d",
    "rmsa": "923c6b54db8b9e404cf05243529ffe4f8a439f168b824ca74a83aa8eab537453",
    "rwa": "293507b99dd6be26c69372764ab3acc6edf13a2a39e6bd45b6ad182ff20f11c6",
    "rwa_s8": "debceacc37b5a0d1bcb9c09ccaa06daa9abdfb6ba44464754cfb2b501625987d",
}


@functools.lru_cache(maxsize=None)
def driven(name):
    """every walk of the family on the model, finished episodes counted"""
    return [ow.drive_oracle(name, w, ledger=True) for w in ow.walks_of(name)]


def test_the_circuit_takes_every_ordered_pair_once():
    for k in (1, 2, 5, 10, 11):
        c = ow.euler_circuit(k)
        assert len(c) == k * k + 1 and c[0] == c[-1]
        assert len(ow.pairs_of(c)) == k * k
    pieces = ow.cut(list(range(101)), 35)
    assert [len(p) for p in pieces] == [35, 35, 33] and all(a[-1] == b[0] for a, b in zip(pieces, pieces[1:]))


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_walks_stay_inside_their_budget_and_the_api(name):
    f = ow.FAMILIES[name]
    lo, hi = ow.load_range(f)
    cap = ow.capacity_needed(ow.base_rates(f)[0])
    assert ow.capacity_needed(hi) <= cap < ow.capacity_needed(hi + 1.0) and lo < hi
    walks = ow.walks_of(name)
    assert [w.name for w in walks] == list(ow.WALK_NAMES)
    assert any(w.fresh for w in walks) and any(not w.fresh for w in walks)
    lengths = set()
    for w in walks:
        kinds = w.kinds()
        assert len(kinds) <= ow.MAX_OPS and w.steps() <= ow.MAX_STEPS, (w.name, len(kinds), w.steps())
        ops = [it for what, it in w.items if what == "op"]
        if w.fresh:
            assert "seed" not in kinds
        else:  # the second streams exist before the first snapshot is taken
            assert w.items[0][0] == "op" and kinds[0] == "seed" and not ops[0]["mask"].any()
        assert w.items[0 if w.fresh else 1] == ("q", dict(q="get_state"))
        snapshots = 0
        for what, it in w.items:
            if what == "q":
                snapshots += it["q"] == "get_state"
                continue
            if it["kind"] == "run":
                lengths.add(it["n"])
            if it["kind"] == "set_state":
                assert 0 <= it["snapshot"] < snapshots
            if it["kind"] == "set_load":
                for v in (it["load"], it["mht"]):
                    assert v is None or (np.all(np.asarray(v) > 0) and np.asarray(v).shape in ((), (f.batch,)))
                assert it["load"] is None or np.all(ow.capacity_needed(np.max(it["load"])) <= cap)
            if it["kind"] == "copy_envs":
                src, dst = it["src"], it["dst"]
                assert len(src) == len(dst) and len(set(dst)) == len(dst) and not set(src) & set(dst)
                assert min(src) >= 0 and min(dst) >= 0 and max(src) < f.batch and max(dst) < f.batch
    assert lengths == set(ow.RUN_LENGTHS)
    copies = [it["variant"] for w in walks for what, it in w.items if what == "op" and it["kind"] == "copy_envs"]
    assert {"fan_out", "pairs", "chain", "named"} <= set(copies)
    masks = [it["mask"] for w in walks for what, it in w.items if what == "op" and "mask" in it]
    sums = {None if m is None else int(m.sum()) for m in masks}
    assert {None, 0, 1, 4, 8, f.batch - 1} <= sums


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_every_pair_of_kinds_and_every_query_after_every_kind(name):
    walks = ow.walks_of(name)
    pairs = set().union(*(ow.pairs_of(w.kinds()) for w in walks))
    missing = [(a, b) for a in ow.KINDS for b in ow.KINDS if (a, b) not in pairs]
    assert not missing, missing
    fresh = set().union(*(ow.pairs_of(w.kinds()) for w in walks if w.fresh))
    assert not [(a, b) for a in ow.FRESH_KINDS for b in ow.FRESH_KINDS if (a, b) not in fresh]  # (what the loop forms run unreduced)
    after = set()
    for w in walks:
        last = None
        for what, it in w.items:
            if what == "op":
                last = it["kind"]
            elif last is not None:
                after.add((last, it["q"]))
    missing = [(k, q) for k in ow.KINDS for q in ow.queries_of(ow.FAMILIES[name]) if (k, q) not in after]
    assert not missing, missing


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_rebuild_by_replay_is_exact_on_the_oracle(name):
    """the env that was driven op by op (runs stepped on the host, rebuilt at every copy and restore) against one replayed from
    its list in one go (runs as oracle runs)"""
    moved = 0
    for w, m in zip(ow.walks_of(name), driven(name)):
        chk = _exact_bits("%s, walk %s" % (name, w.name))
        twins = [m.rebuild(i) for i in range(m.n)]
        got, want = m.readback(twins), m.readback()
        assert set(got) == set(want) and {"counters", "services", "active"} < set(want)
        for what in want:
            for i in range(m.n):
                chk(i, what, got[what][i], want[what][i])
        assert all(lst[0][0] == "make" for lst in m.lists)
        moved += sum(lst[0][1] != s for lst, s in zip(m.lists, ow.seeds_of(m.f)))
    assert moved  # (a copy took its source's construction with it)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_what_the_walks_reach(name):
    models = driven(name)
    episodes = np.concatenate([m.episodes for m in models])
    blocked = np.concatenate([m.blocked for m in models])
    reach = {k: sum(m.reach[k] for m in models) for k in models[0].reach}
    print(name, "two episodes: %.2f, blocked: %.2f" % ((episodes >= 2).mean(), blocked.mean()), reach)
    assert (episodes >= 2).mean() >= 0.5
    # blocked: a heuristic's own action was not provisioned (run, step with the heuristic's actions, policy_step); an agent's refused
    # actions do not count.  An exception is asserted as one, so that it goes when it is no longer true
    if name in ow.NO_NETWORK_BLOCKING:
        assert not blocked.any()
    else:
        assert blocked.mean() >= 0.25
    assert reach["copy_into_pending"] >= 1
    if name in NO_64_PENDING:
        assert reach["copy_from_64"] == 0
    else:
        assert reach["copy_from_64"] >= 1
    assert reach["restore_across_episode"] >= 1
    assert reach["set_load_on_pending"] >= 1
    named = models[-1]  # the reseeded source and the copy made after the reseed carry the mark, the copy made before does not
    assert named.reach["copy_into_pending"] >= 1 and named.reseeded().sum() == 2


def test_a_restore_puts_back_the_list_a_copy_replaced():
    """snapshot, copy 0 -> 9, restore: env 9 is its own past again, not a prefix of env 0's"""
    m = ow.Model("rwa")
    m.apply(dict(kind="run", policy="SAP_FF", n=7))
    m.snapshot()
    before = m.readback()
    m.apply(dict(kind="run", policy="SAP_FF", n=3))
    m.apply(dict(kind="copy_envs", src=np.array([0]), dst=np.array([9])))
    assert m.lists[9][0] == m.lists[0][0]
    m.apply(dict(kind="set_state", snapshot=0))
    after = m.readback()
    for what in before:
        _exact_bits("restore")(0, what, after[what], before[what])


# ---- the view walks: the device choosers as a stepping kind, the five newer device calls as queries ------------------------------------
def _feed(h, v):
    """a value of a walk into the hash, by type: arrays as dtype, shape and bytes; dicts by sorted key; floats by their hex form"""
    if isinstance(v, np.ndarray):
        h.update(b"A" + v.dtype.str.encode() + repr(tuple(v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        h.update(b"D%d" % len(v))
        for k in sorted(v):
            _feed(h, k), _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"L%d" % len(v))
        for x in v:
            _feed(h, x)
    elif v is None:
        h.update(b"N")
    elif isinstance(v, (bool, np.bool_)):
        h.update(b"B%d" % int(v))
    elif isinstance(v, (int, np.integer)):
        h.update(b"I" + str(int(v)).encode())
    elif isinstance(v, (float, np.floating)):
        h.update(b"F" + float(v).hex().encode())
    else:
        assert isinstance(v, str), type(v)
        h.update(b"S" + v.encode())
    h.update(b";")


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_the_five_walks_are_what_they_were_before_the_view_walks(name):
    assert sorted(WALK_DIGESTS) == FAMILY_NAMES
    ow.view_walks_of(name)  # (built first: they must not move the other builder's generator or counters)
    h = hashlib.sha256()
    _feed(h, [(w.name, w.fresh, w.items) for w in ow.walks_of(name)])
    assert h.hexdigest() == WALK_DIGESTS[name]
    assert ow.KINDS == ("run", "step_heur", "step_agent", "policy_step", "step_async", "reset_soft", "reset_full", "seed", "set_load", "set_state",
                        "copy_envs")


@functools.lru_cache(maxsize=None)
def driven_views(name):
    return [ow.drive_oracle(name, w, ledger=True) for w in ow.view_walks_of(name)]


def _ops(w):
    return [it for what, it in w.items if what == "op"]


def _queries_after(walks):
    """{(kind, query)}, [the queries between two ops, per op]"""
    after, groups = set(), []
    for w in walks:
        last = None
        for what, it in w.items:
            if what == "op":
                last = it["kind"]
                groups.append([])
            elif last is not None:
                after.add((last, it["q"]))
                groups[-1].append(it["q"])
    return after, groups


def test_only_qos_is_without_view_walks():
    assert [n for n in FAMILY_NAMES if n not in VIEW_FAMILIES] == ["qos"] and ow.view_walks_of("qos") == ()
    assert [n for n in VIEW_FAMILIES if n not in CHOOSER_FAMILIES] == ["deeprmsa"]
    assert ow.view_queries_of(ow.FAMILIES["rmsa"]) == ["release_horizons", "block_table", "assign_spectrum", "route_spectrum", "select_blocks"]
    assert ow.view_queries_of(ow.FAMILIES["rwa_s8"]) == ow.view_queries_of(ow.FAMILIES["rwa"]) == ow.view_queries_of(ow.FAMILIES["rmsa"])
    assert ow.view_queries_of(ow.FAMILIES["rmcsa"]) == ["release_horizons", "block_table", "route_cores", "select_blocks"]
    assert ow.view_queries_of(ow.FAMILIES["deeprmsa"]) == ["release_horizons", "block_table"]


@pytest.mark.parametrize("name", VIEW_FAMILIES)
def test_view_walks_stay_inside_the_budget_and_cover_what_they_exist_for(name):
    f = ow.FAMILIES[name]
    walks = ow.view_walks_of(name)
    assert [w.name for w in walks] == list(ow.VIEW_WALK_NAMES) == [ow.walk_of(name, n).name for n in ow.VIEW_WALK_NAMES]
    fresh, seeded = walks
    assert fresh.fresh and "seed" not in fresh.kinds()
    assert not seeded.fresh and seeded.kinds()[0] == "seed" and not _ops(seeded)[0]["mask"].any() and seeded.kinds().count("seed") >= 2
    for w in walks:
        kinds, ops = w.kinds(), _ops(w)
        assert len(kinds) <= ow.MAX_OPS and w.steps() <= ow.MAX_STEPS, (w.name, len(kinds), w.steps())
        first = 0 if w.fresh else 1
        assert w.items[first] == ("q", dict(q="get_state"))
        assert [(it["kind"], it["n"]) for it in ops[first:first + 2]] == [("run", 37), ("run", 37)]
        snapshots = 0
        for what, it in w.items:
            if what == "q":
                snapshots += it["q"] == "get_state"
            elif it["kind"] == "set_state":
                assert 0 <= it["snapshot"] < snapshots
    assert [it["n"] for it in _ops(seeded)[-4:]] == [20] * 4  # (runs across episode ends close the seeded walk)
    # the filler: step_device, or step_agent where the family has no chooser that writes an action
    variants = ow.chooser_variants_of(f)
    F = "step_device" if variants else "step_agent"
    assert ("step_device" in fresh.kinds()) == bool(variants)
    pairs = set().union(*(ow.pairs_of(w.kinds()) for w in walks))
    assert not [k for k in ow.KINDS + (F,) if (F, k) not in pairs or (k, F) not in pairs]
    in_fresh = ow.pairs_of(fresh.kinds())  # (what the loop forms run unreduced)
    assert not [k for k in ow.FRESH_KINDS + (F,) if (F, k) not in in_fresh or (k, F) not in in_fresh]
    # every op carries two queries of the other walks' rotation and one of the view rotation; every view query follows every kind
    views, old = ow.view_queries_of(f), ow.queries_of(f)
    after, groups = _queries_after(walks)
    opening = [g for g in groups if not g or g == ["get_state"]]
    assert len(opening) <= 1  # (the opening seed of the seeded walk: the snapshot alone)
    assert all(len(g) == 3 and g[0] in old and g[1] in old and g[2] in views for g in groups if g not in opening)
    kinds = ow.KINDS + (("step_device",) if variants else ())
    assert not [(k, q) for k in kinds for q in views if (k, q) not in after]
    queries = [it for w in walks for what, it in w.items if what == "q"]
    of = lambda q: [it for it in queries if it["q"] == q]
    mods = {None, ow.FIXED} if f.fam == "RMCSA" else {None}
    assert {it["j"] for it in of("release_horizons")} == set(ow.HORIZON_J) and {it["mod"] for it in of("release_horizons")} == mods
    assert {it["j"] for it in of("block_table")} == set(ow.TABLE_J) and {it["mod"] for it in of("block_table")} == mods
    if f.fam == "DeepRMSA":
        assert f.kw["j"] in {it["j"] for it in of("block_table")}
    if variants:
        assert {(it["placement"], it["mod"]) for it in of("select_blocks")} == {(p, m) for p in ("first", "last") for m in mods}
        asked = {tuple(p) for it in of("route_cores" if f.fam == "RMCSA" else "route_spectrum") for p in it["pairs"]}
        assert asked == set(ow.rule_route_pairs(f)) and len(asked) == (25 if f.fam == "RMCSA" else 21)
    if f.fam == "RMCSA":
        assert {None if it["given"] is None else it["given"].shape[1] for it in of("route_cores")} == {None, 1, 2}
        assert {it["mod"] for it in of("route_cores")} == mods
    elif variants:
        from tests import assign_restate

        assert {(it["rule"]) for it in of("assign_spectrum")} == set(assign_restate.RULES)
        assert {it["source"] for it in of("assign_spectrum")} == {"none", "host", "buffer"}
        for it in of("assign_spectrum"):
            p = it["paths"]
            assert (p is None) == (it["source"] == "none")
            assert p is None or ((p == 5).any() and (p < 0).any() and ((p >= 0) & (p < 5)).any())
    # every chooser variant, stepped both ways; on the fresh and on the reseeded batch
    for w in walks:
        sd = [it for it in _ops(w) if it["kind"] == "step_device"]
        assert {(it["variant"], it["form"]) for it in sd} >= {(v, form) for v in variants for form in ("step", "step_async")} or w is seeded
        assert {it["variant"] for it in sd} == set(variants)
    sd = [it for w in walks for it in _ops(w) if it["kind"] == "step_device"]
    if f.fam == "RMCSA":
        hosts = [it for it in sd if it["variant"] == "route_cores_host"]
        assert {None if it["given"] is None else it["given"].shape[1] for it in hosts} == {None, 1, 2} and {it["mod"] for it in hosts} == mods
    if variants:
        assert {it["placement"] for it in sd if it["variant"].startswith("select_")} == {"first", "last"}


@pytest.mark.parametrize("name", VIEW_FAMILIES)
def test_rebuild_by_replay_is_exact_on_the_oracle_with_the_chooser_steps(name):
    """as test_rebuild_by_replay_is_exact_on_the_oracle: a step_device entry is replayed as a plain step with the recorded action"""
    for w, m in zip(ow.view_walks_of(name), driven_views(name)):
        chk = _exact_bits("%s, walk %s" % (name, w.name))
        twins = [m.rebuild(i) for i in range(m.n)]
        got, want = m.readback(twins), m.readback()
        assert set(got) == set(want) and {"counters", "services", "active"} < set(want)
        for what in want:
            for i in range(m.n):
                chk(i, what, got[what][i], want[what][i])
        assert any(e[0] == "step" for lst in m.lists for e in lst)


@pytest.mark.parametrize("name", VIEW_FAMILIES)
def test_what_the_view_walks_reach(name):
    models = driven_views(name)
    reach = {k: sum(m.reach[k] for m in models) for k in models[0].reach}
    print(name, reach)
    episodes = np.concatenate([m.episodes for m in models])
    assert (episodes >= 2).mean() >= 0.5
    assert reach["restore_across_episode"] >= 1 and reach["copy_into_pending"] >= 1 and reach["set_load_on_pending"] >= 1
    assert models[1].reseeded().any()
    # block_table: a state with a row without a block and one with a row of at least j.  An exception is asserted as one: with 65
    # wavelengths no path of RWA runs out of them within a walk (ow.NO_NETWORK_BLOCKING); the same family at 8 wavelengths gets there
    assert reach["table_row_of_j_blocks"] >= 1
    assert (reach["table_row_of_0_blocks"] == 0) if name in ow.NO_NETWORK_BLOCKING else (reach["table_row_of_0_blocks"] >= 1)
    if name in VIEWS_NO_64_PENDING:
        assert reach["horizon_over_64_pending"] == 0
    else:
        assert reach["horizon_over_64_pending"] >= 1
    chooser = [k for k in reach if k.startswith("chooser_")]
    assert len(chooser) == 7
    for k in chooser:
        for m in models:  # (each walk by itself: the fresh one is what the loop forms run, the seeded one the reseeded batch)
            assert (m.reach[k] >= 1) if name in CHOOSER_FAMILIES else (m.reach[k] == 0), (name, k)
