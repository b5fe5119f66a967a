"""capacity_after on the device (include/orl.h, orl_batch_capacity_after; k_capacity_after in csrc/orl_capacity_after.h) against the numpy
restatement (tests/capacity_after_restate.py: the window taken out of the dense maps, then tests/capacity_restate.py's counts — no delta):
every source and both layouts on every env with ==, from slots_packed() of that moment — at construction, after a warm-up under the
family's heuristic and after slot_agent's boundary-seeking agent steps — over the row widths, core counts and topologies at which the
kernel can go wrong, the shapes of tests/capacity_cases.py among them; `given` candidates at the word edges and every kind of absent
one; the argmin stepped through select_blocks / route_cores; graph capture; every way of stepping; two shards; the refusals.  That
the states are not ones on which no placement changes anything is asserted on the oracle in tests/test_capacity_after.py."""
import numpy as np
import pytest

from tests import capacity_after_restate as car
from tests import capacity_cases as cc
from tests import capacity_restate as cap
from tests import horizon_model as hm
from tests import slot_agent
from tests import test_network_capacity_gpu as ncg

pytestmark = pytest.mark.gpu

MAX_Q = 1024
# name -> envs (the restatement's path rows are what costs the time: RMCSA at 31 cores and germany50 run few)
ENVS = {"rmsa_nsf_s64": 8, "rmsa_nsf_s65": 8, "rmsa_nsf_s129": 8, "rmsa_nsf_s321": 6, "rmsa_nsf_s512": 6, "rwa_nsf_s129": 8, "rmsa_ger_s128": 2,
        "rmcsa_c2_s129": 6, "rmcsa_c7_s64": 3, "rmcsa_c31_s64": 2, "tiny5_k3": 8}
ENVELOPE = {"ring10c8_k9_rmsa": 6, "k6full_k64_rmsa": 4, "star65_rmsa": 2, "ring31_rmsa": 4, "s512_w64_rmsa": 6, "nsf_s64_r65": 6, cc.UNSTAGED: 2}
MEMO = {}
LAYOUTS = ("classes", "total")


def cores_of(fam, C):
    return C if fam == "RMCSA" else 1


def route_cands(env, fam, S, rule="first", route="ksp"):
    """The route / core table of this moment, written by the call the source reads -> the candidates the restatement works from"""
    tab = env.route_cores(rule, route, table=True)[1] if fam == "RMCSA" else env.route_spectrum(rule, route, table=True)[1]
    return car.route_candidates(tab, S)


def block_cands(env, j, placement, S):
    return car.block_candidates(env.block_table(j)[0], j, placement, S)


def random_cands(env, fam, C, S, rng, Q=7):
    """Q given candidates per env: rows from -1 to k C' (both absent), windows that hang over both ends among those that do not"""
    R = env.k_paths * cores_of(fam, C)
    c = np.stack([rng.randint(-1, R + 1, (env.num_envs, Q)), rng.randint(-2, S, (env.num_envs, Q)), rng.randint(0, 12, (env.num_envs, Q))], axis=2)
    return c.astype(np.int64)


def check(env, fam, C, S, need, what, source, cands, j=1, placement="first", chunk=car.CHUNK, limit=None, full_envs=1):
    """Both layouts of `source` against the restatement of cands on slots_packed() of this moment, every env and every candidate, with ==;
    the baseline row is network_capacity("counts"); "total" the row sums of "classes"; get_state() and flags() as before.
    `limit` is for the two shapes whose restatement costs seconds per env and source (RMCSA at 31 cores: 155 rows of 31 x 22 link rows
    each; germany50 RMCSA at 10 cores of 512 slots: 60 MB of path rows per candidate) and for nothing else: there the first `full_envs`
    envs are still restated in full, and of every other env `limit` present candidates, evenly spread over the present ones, with the
    other rows held to being present.  Returns the restatement [n, Q + 1, n_cls], -1 in the rows it did not work out."""
    n, n_cls, Q = env.num_envs, need.shape[3], cands.shape[1]
    src, dst = car.pending_pairs(env)
    ok = car.present(cands, env.topology, src, dst, cores_of(fam, C), S)
    takes = []
    for e in range(n):
        pres = np.flatnonzero(ok[e])
        if limit is not None and e >= full_envs and len(pres) > limit:
            pres = pres[np.unique(np.linspace(0, len(pres) - 1, limit).astype(np.int64))]
        takes.append(pres)
    m = max(1, max(len(t) for t in takes))
    sub, sel = np.zeros((n, m, 3), np.int64), np.full((n, m), -1, np.int64)
    for e, take in enumerate(takes):
        sel[e, :len(take)], sub[e, :len(take)] = take, cands[e, take]
    part, _ = car.after(hm.avail_of(env, cores_of(fam, C), S), env.topology, need, src, dst, sub, chunk=chunk, memo=MEMO)
    want = np.full((n, Q + 1, n_cls), -1, np.int32)
    known = np.concatenate([~ok, np.ones((n, 1), bool)], axis=1)  # absent rows and the baseline; then the rows worked out
    want[:, Q] = part[:, m]
    for e in range(n):
        t = sel[e] >= 0
        want[e, sel[e, t]] = part[e, :m][t]
        known[e, sel[e, t]] = True
    before = (env.get_state(), env.flags().copy())
    counts = env.network_capacity("counts")[:, :n_cls]
    kw = dict(source=source, j=j, placement=placement, candidates=cands.astype(np.int32) if source == "given" else None)
    got = {}
    for layout in LAYOUTS:
        width = n_cls if layout == "classes" else 1
        dim = (Q + 1) * width
        assert env.capacity_after_shape(source, layout, j, Q if source == "given" else 0) == (Q, width, dim, (dim + 3) // 4 * 4), (what, source, layout)
        got[layout] = g = env.capacity_after(layout=layout, **kw)
        assert g.shape == (n, dim) and g.dtype == np.int32, (what, source, layout)
        g3 = g.reshape(n, Q + 1, width)
        w3 = want if layout == "classes" else car.total(want)[:, :, None]
        bad = np.argwhere(((g3 != w3).any(axis=2) & known) | ((g3 < 0).any(axis=2) & ~known))
        if len(bad):
            e, q = (int(x) for x in bad[0])
            raise AssertionError("%s, %s, %s: %d rows differ; env %d candidate %d %r: got %r, want %r"
                                 % (what, source, layout, len(bad), e, q, cands[e, min(q, Q - 1)].tolist(), g3[e, q].tolist(), w3[e, q].tolist()))
    assert np.array_equal(got["classes"].reshape(n, Q + 1, n_cls)[:, Q], counts), (what, source)
    assert np.array_equal(got["total"], car.total(got["classes"].reshape(n, Q + 1, n_cls))), (what, source)
    assert np.array_equal(env.get_state(), before[0]) and np.array_equal(env.flags(), before[1]), (what, source)
    return want


def check_sources(env, fam, C, S, need, what, rng, js=((1, "first"), (4, "last")), deep=False, chunk=car.CHUNK, limit=None, full_envs=1):
    """Every source of this family on the present state; returns the largest loss per env over all of them.  limit, full_envs: check()'s,
    for the two slow shapes alone; there the envs restated in full are so under "route" and "given", and sampled like the others under
    "blocks", whose rows are the same windows several times over"""
    loss = np.zeros(env.num_envs, np.int64)
    runs = []
    if not deep:
        runs.append(("route", route_cands(env, fam, S), 1, "first"))
    for j, placement in js:
        runs.append(("blocks", block_cands(env, j, placement, S), j, placement))
    runs.append(("given", random_cands(env, fam, C, S, rng), 1, "first"))
    for source, cands, j, placement in runs:
        t = car.total(check(env, fam, C, S, need, what, source, cands, j, placement, chunk, limit, full_envs if source != "blocks" else 0))
        loss = np.maximum(loss, np.where(t[:, :-1] >= 0, t[:, :-1] - t[:, -1:], 0).max(axis=1))
    return loss


@pytest.mark.parametrize("name", list(ENVS))
def test_every_source_equals_the_restatement_on_the_shapes(name):
    env, fam, tab, C, S = ncg.make(name, n=ENVS[name])
    need, pol, rng = ncg.need_of(name), hm.HEURISTIC[fam], np.random.RandomState(len(name) + S)
    js = ((1, "first"), (4, "last"))
    # (31 cores: 155 rows, 620 blocks at j = 4: env 0 is restated in full after the warm-up, under "route" and "given")
    limit = 6 if name == "rmcsa_c31_s64" else None
    check_sources(env, fam, C, S, need, name + ", construction", rng, js, limit=limit, full_envs=0)
    env.run(pol, ncg.SHAPES[name][1])
    loss = check_sources(env, fam, C, S, need, name + ", warm-up", rng, js, limit=limit)
    print(name, "largest loss per env after the warm-up", list(loss))
    # (the oracle's conditions, tests/test_capacity_after.py: the same seeds, loads and steps)
    at_least = {"rmsa_nsf_s65": 3, "rmsa_nsf_s129": 3, "rwa_nsf_s129": 1, "rmcsa_c2_s129": 2}.get(name, 0)
    assert int((loss > 0).sum()) >= at_least, (name, loss)
    if name == "tiny5_k3":
        for _ in range(ncg.AGENT_STEPS):
            env.policy_step(pol, auto_reset=True, fetch=False)
    else:
        ncg.agent_steps(env, fam, tab, C, S, ncg.AGENT_STEPS, np.random.RandomState(S + C))
    check_sources(env, fam, C, S, need, name + ", agent steps", rng, js, limit=limit, full_envs=0)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("name", list(ENVELOPE))
def test_envelope_shapes_equal_the_restatement(name, tmp_path):
    """tests/capacity_cases.py's shapes after their warm-up: the second k8 word (k = 9), k = 64, N > 64 with n_paths < k, 30 hops, n = 64
    at W = 8, more than 64 classes, and the slot maps left in global memory (germany50 RMCSA, 10 cores of 512 slots)"""
    shape = cc.SHAPE_BY_NAME[name]
    env, need, C, S = ncg.make_envelope(shape, tmp_path, n=ENVELOPE[name])
    fam = cc.need_family(shape)
    env.run(shape.policy, shape.warm)
    rng = np.random.RandomState(len(name))
    unstaged = name == cc.UNSTAGED
    js = ((1, "first"),) if unstaged or shape.k > 16 else ((1, "first"), (4, "last"))
    limit = 3 if unstaged else None  # (env 0 is restated in full all the same)
    loss = check_sources(env, fam, C, S, need, name, rng, js, deep=shape.fam == "DeepRMSA", chunk=1 if unstaged else car.CHUNK, limit=limit)
    print(name, "largest loss per env", list(loss))
    env.check()
    env.close()


def test_the_per_path_array_is_refused_on_a_real_batch(tmp_path):
    from optical_rl_gym_amd._lib import OrlError

    shape = cc.SHAPE_BY_NAME["star129_rmsa"]
    env, need, C, S = ncg.make_envelope(shape, tmp_path, n=2)
    env.route_spectrum("first", "ksp", fetch=False)
    snap = env.get_state()
    for call in (lambda: env.capacity_after("route"), lambda: env.capacity_after("route", "classes", fetch=False), lambda: env.capacity_after_shape("route", "total")):
        with pytest.raises(OrlError, match="per-path array of 129 x 129 pairs x 5 paths"):
            call()
    with pytest.raises(OrlError, match=r"call capacity_after\("):
        env.device_tensor("capacity_after_total")
    assert np.array_equal(env.get_state(), snap)
    env.close()


def deep_batch(n=8):
    import optical_rl_gym_amd as orl

    case = slot_agent.CASE_BY_NAME["deep_s129_j4"]
    env = orl.make("DeepRMSA", topology=slot_agent.TOPOLOGY, num_envs=n, seeds=list(range(100, 100 + n)), **dict(case.kw, mean_service_inter_arrival_time=10.0 / 260))
    return env, cap.need_table("RMSA", env.topology, cap.class_rates("RMSA", {}))


def test_deeprmsa_blocks_with_its_own_j_and_another_and_given():
    from optical_rl_gym_amd._lib import OrlError

    env, need = deep_batch()
    env.run("SAP", 700)
    loss = check_sources(env, "RMSA", 1, 129, need, "deep_s129_j4", np.random.RandomState(4), js=((4, "first"), (2, "last")), deep=True)
    print("deep_s129_j4 largest loss per env", list(loss))
    assert (loss > 0).any()
    with pytest.raises(OrlError, match="DeepRMSA has no such table"):
        env.capacity_after("route")
    env.close()


@pytest.mark.parametrize("name", ["rmsa_nsf_s65", "rmsa_nsf_s129", "rmsa_nsf_s512"])
def test_given_candidates_at_the_edges(name):
    """Windows at the word edges of S = 65, 129 and 512, the same candidate twice, a window over taken slots, and every kind of absent
    candidate but p >= n_paths, which NSFNET's pairs of k paths each cannot show (test_a_path_the_pair_does_not_have_is_absent)"""
    env, fam, tab, C, S = ncg.make(name, n=6)
    need, K = ncg.need_of(name), env.k_paths
    env.run("SAP_FF", ncg.SHAPES[name][1])
    n = env.num_envs
    avail = hm.avail_of(env, 1, S)
    src, dst = car.pending_pairs(env)
    taken = np.zeros(n, np.int64)  # per env a slot of path 0's first link that is taken (0 where the link is empty)
    for e in range(n):
        busy = np.flatnonzero(~avail[e, 0, env.topology.path_links[src[e], dst[e], 0, 0]])
        taken[e] = busy[0] if len(busy) else 0
    windows = [(0, 1), (S - 1, 1), (63, 2), (64, min(64, S - 64)), (0, S), (1, 64), (0, 1)]
    rows = [[(q % 2, s, k) for q, (s, k) in enumerate(windows)] + [(0, int(taken[e]), 1)] +
            [(-1, 0, 1), (K, 0, 1), (K + 3, 0, 1), (0, -1, 2), (0, S - 1, 2), (0, 3, 0), (0, 3, -4), (0, S, 1)]
            for e in range(n)]
    cands = np.array(rows, np.int64)
    want = check(env, fam, C, S, need, name + ", edges", "given", cands)
    Q = len(windows)
    assert np.array_equal(want[:, 0], want[:, Q - 1]) and (want[:, 0] >= 0).all()  # the same candidate twice
    busy = np.array([not avail[e, 0, env.topology.path_links[src[e], dst[e], 0, 0], taken[e]] for e in range(n)])
    assert (want[:, Q + 1:Q + 9] == -1).all() and (want[:, Q + 9] >= 0).all() and want.shape[1] == Q + 10
    assert (want[:, 4] >= want[:, -1]).all() and (want[:, 4] > want[:, -1]).any()  # the whole row of a path costs something somewhere
    assert busy.any() and all(np.array_equal(want[e, Q], want[e, -1]) for e in np.flatnonzero(busy) if env.topology.path_hops[src[e], dst[e], 0] == 1)
    env.close()


@pytest.mark.parametrize("name", ["tiny5_k3", "star65_rmsa"])
def test_a_path_the_pair_does_not_have_is_absent(name, tmp_path):
    """Topologies with n_paths < k: for every env whose pending pair has fewer than k paths the candidate on row n_paths (0 <= row < k, so
    only p >= n_paths makes it absent) gives -1, the one on row n_paths - 1 is present, and so is row k - 1 exactly where the pair has k"""
    if name == "tiny5_k3":
        env, fam, tab, C, S = ncg.make(name, n=8)
        need = ncg.need_of(name)
        env.run("SAP_FF", 200)
    else:
        shape = cc.SHAPE_BY_NAME[name]
        env, need, C, S = ncg.make_envelope(shape, tmp_path, n=4)
        fam = cc.need_family(shape)
        env.run(shape.policy, shape.warm)
    K = env.k_paths
    src, dst = car.pending_pairs(env)
    npaths = env.topology.n_paths[src, dst].astype(np.int64)
    assert (npaths >= 1).all() and (npaths < K).any()
    cands = np.array([[(min(int(p), K - 1), 0, 1), (int(p) - 1, 0, 1), (K - 1, 1, 2)] for p in npaths], np.int64)
    want = check(env, fam, C, S, need, name + ", p >= n_paths", "given", cands)
    short = npaths < K
    assert (want[short, 0] == -1).all() and (want[short, 2] == -1).all() and (want[~short, 0] >= 0).all() and (want[:, 1] >= 0).all()
    env.close()


def test_the_cap_on_the_candidates():
    from optical_rl_gym_amd._lib import OrlError

    env, fam, tab, C, S = ncg.make("tiny5_k3", n=3)
    need = ncg.need_of("tiny5_k3")
    env.run("SAP_FF", 200)
    rng = np.random.RandomState(1)
    cands = np.stack([rng.randint(0, 3, (3, MAX_Q)), rng.randint(0, S, (3, MAX_Q)), rng.randint(1, 9, (3, MAX_Q))], axis=2).astype(np.int64)
    check(env, fam, C, S, need, "tiny5_k3 at the cap", "given", cands)
    more = np.zeros((3, MAX_Q + 1, 3), np.int32)
    for call in (lambda: env.capacity_after("given", candidates=more), lambda: env.capacity_after_shape("given", "total", 1, MAX_Q + 1),
                 lambda: env.capacity_after("given", candidates=more[:, :0])):
        with pytest.raises(OrlError, match="1 .. 1024 candidates"):
            call()
    env.close()


@pytest.mark.parametrize("name", ["rmsa_nsf_s65", "rwa_nsf_s129", "rmcsa_c7_s64"])
def test_blocks_at_every_j_and_the_argmin_steps(name):
    """j = 1, 4 and 8 under both placements; then the argmin over "total" of the present candidates, written into column 0 of the actions
    buffer on the device, goes through select_blocks(blocks=None) and a step, and is accepted wherever a block exists"""
    import torch

    env, fam, tab, C, S = ncg.make(name, n=3 if name == "rmcsa_c7_s64" else 6)  # (280 candidates per env at j = 8 on 7 cores)
    need = ncg.need_of(name)
    env.run(hm.HEURISTIC[fam], ncg.SHAPES[name][1])
    for j in (1, 4, 8):
        for placement in ("first", "last"):
            check(env, fam, C, S, need, "%s, j = %d" % (name, j), "blocks", block_cands(env, j, placement, S), j, placement)
    j, placement = 4, "last"
    mask = env.block_table(j)[1]
    env.capacity_after("blocks", "total", j=j, placement=placement, fetch=False)
    with torch.cuda.stream(env.torch_stream()):
        t = env.device_tensor("capacity_after_total")[:, :-1]
        best = torch.argmin(torch.where(t >= 0, t, torch.full_like(t, 2 ** 30)), dim=1).to(torch.int32)
        env.device_tensor("actions")[:, 0] = best
    acts = env.select_blocks(blocks=None, j=j, placement=placement)
    env.sync()
    best = best.cpu().numpy()
    exists = mask[:, :-1].any(axis=1)
    assert exists.any() and mask[np.arange(env.num_envs), best][exists].all()
    rew = np.asarray(env.step(None, auto_reset=True)[1]).copy()
    assert np.array_equal(rew > 0, exists), (rew, exists)
    assert not (env.flags() & 2).any()
    K = env.k_paths
    assert (acts[exists, 0] < K).all() and (acts[~exists, 0] == K).all()
    env.check()
    env.close()


@pytest.mark.parametrize("rule", ["first", "last", "best"])
def test_route_after_route_spectrum_under_the_rules(rule):
    import torch

    name = "rmsa_nsf_s129"
    env, fam, tab, C, S = ncg.make(name, n=6)
    need = ncg.need_of(name)
    env.run("SAP_FF", ncg.SHAPES[name][1])
    cands = route_cands(env, fam, S, rule, "ksp")
    want = car.total(check(env, fam, C, S, need, "%s, %s" % (name, rule), "route", cands))
    # the argmin path and its slot, written as (path, slot) into the actions buffer on the device, then stepped
    env.capacity_after("route", "total", fetch=False)
    with torch.cuda.stream(env.torch_stream()):
        t = env.device_tensor("capacity_after_total")[:, :-1]
        best = torch.argmin(torch.where(t >= 0, t, torch.full_like(t, 2 ** 30)), dim=1)
        table = env.device_tensor("assign_table").view(env.num_envs, -1, 4)
        a = env.device_tensor("actions")
        a[:, 0] = torch.where(t.max(dim=1).values >= 0, best, torch.full_like(best, env.k_paths)).to(torch.int32)
        a[:, 1] = table[torch.arange(env.num_envs, device=t.device), best, 0]
    env.sync()
    fits = (want[:, :-1] >= 0).any(axis=1)
    masked = np.where(want[:, :-1] >= 0, want[:, :-1], 2 ** 30)
    assert fits.any() and np.array_equal(best.cpu().numpy()[fits], masked.argmin(axis=1)[fits])
    rew = env.step(None, auto_reset=True)[1]
    assert np.array_equal(np.asarray(rew) > 0, fits)
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


def test_route_after_route_cores_and_the_argmin_through_n_given_2():
    import torch

    name = "rmcsa_c2_s129"
    env, fam, tab, C, S = ncg.make(name, n=6)
    need = ncg.need_of(name)
    env.run(hm.HEURISTIC[fam], ncg.SHAPES[name][1])
    for rule, route in (("first", "best"), ("last", "ksp")):
        want = car.total(check(env, fam, C, S, need, "%s, %s" % (name, rule), "route", route_cands(env, fam, S, rule, route)))
    env.route_cores("first", "ksp", fetch=False)
    env.capacity_after("route", "total", fetch=False)
    with torch.cuda.stream(env.torch_stream()):
        t = env.device_tensor("capacity_after_total")[:, :-1]
        best = torch.argmin(torch.where(t >= 0, t, torch.full_like(t, 2 ** 30)), dim=1).to(torch.int32)
        a = env.device_tensor("actions")
        a[:, 0] = best // C
        a[:, 2] = best % C
    acts = env.route_cores("first", "ksp", n_given=2)
    first = car.total(check(env, fam, C, S, need, name + ", first", "route", route_cands(env, fam, S, "first", "ksp")))
    fits = (first[:, :-1] >= 0).any(axis=1)
    masked = np.where(first[:, :-1] >= 0, first[:, :-1], 2 ** 30)
    assert fits.any() and np.array_equal((acts[:, 0] * C + acts[:, 2])[fits], masked.argmin(axis=1)[fits])
    env.close()


def test_route_and_view_captured_in_one_graph_and_read_in_place():
    """{route_spectrum(fetch=False); capacity_after(fetch=False) x 2; step(None)} captured after a first pass and replayed; after
    further steps outside the graph one more replay, and the tensors are the restatement of the state that replay saw"""
    import torch

    name = "rmsa_nsf_s65"
    env, fam, tab, C, S = ncg.make(name, n=12)
    need = ncg.need_of(name)
    env.run("SAP_FF", ncg.SHAPES[name][1])
    s = env.torch_stream()

    def chain(e, step):
        e.route_spectrum("first", "ksp", fetch=False)
        e.capacity_after("route", "total", fetch=False)
        e.capacity_after("route", "classes", fetch=False)
        if step:
            e.step(None, auto_reset=True, fetch=False)

    with torch.cuda.stream(s):
        chain(env, False)
    torch.cuda.synchronize()
    graphs = []
    for step in (True, False):
        g = torch.cuda.CUDAGraph()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=s):
            chain(env, step)
        torch.cuda.synchronize()
        graphs.append(g)
    for _ in range(10):
        graphs[0].replay()
    torch.cuda.synchronize()
    for _ in range(5):
        env.policy_step("SAP_FF", auto_reset=True, fetch=False)
    env.sync()
    graphs[1].replay()  # (the chain without the step: the tensors then describe the present state)
    torch.cuda.synchronize()
    src, dst = car.pending_pairs(env)
    cands = car.route_candidates(env.device_tensor("assign_table").cpu().numpy().reshape(env.num_envs, -1, 4), S)
    want, _ = car.after(hm.avail_of(env, 1, S), env.topology, need, src, dst, cands, memo=MEMO)
    tot, cls = env.device_tensor("capacity_after_total"), env.device_tensor("capacity_after_classes")
    assert tot.shape == (12, 6) and tot.stride() == (8, 1) and cls.shape == (12, 6 * 76) and tot.dtype == torch.int32
    assert np.array_equal(cls.cpu().numpy(), want.reshape(12, -1)) and np.array_equal(tot.cpu().numpy(), car.total(want))
    assert not (env.flags() & 2).any()
    env.check()
    env.close()


@pytest.mark.parametrize("name", ["rmsa_nsf_s65", "rmcsa_c7_s64"])
def test_the_view_follows_every_way_of_stepping(name):
    env, fam, tab, C, S = ncg.make(name, n=6)
    need, pol, rng = ncg.need_of(name), hm.HEURISTIC[fam], np.random.RandomState(7)
    here = lambda what: check(env, fam, C, S, need, "%s, %s" % (name, what), "route", route_cands(env, fam, S))
    env.run(pol, ncg.SHAPES[name][1])
    here("run")
    for _ in range(4):
        env.step(env.policy(pol), auto_reset=True)
    here("step")
    for _ in range(4):
        env.policy_step(pol, auto_reset=True, fetch=False)
    here("policy_step")
    for _ in range(4):
        env.step_async(env.policy(pol), auto_reset=True)
        env.step_wait()
    here("step_async")
    check(env, fam, C, S, need, name + ", given", "given", random_cands(env, fam, C, S, rng))
    env.check()
    env.close()


def test_two_shards_on_one_device():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    name, n, cut = "rmsa_nsf_s65", 10, 3
    whole = ncg.make(name, n=n)[0]
    fam, topo, kw, S = ncg.config(name)
    seeds = [hm.SEED0 + e for e in range(n)]
    mk = lambda sd: orl.make(fam, topology=topo, num_envs=len(sd), seeds=sd, **kw)
    multi = MultiDeviceBatch.from_shards([mk(seeds[:cut]), mk(seeds[cut:])])
    for _ in range(150):
        a = whole.policy("SAP_FF")
        whole.step(a, auto_reset=True)
        multi.step(a, auto_reset=True)
    need = ncg.need_of(name)
    cands = route_cands(whole, fam, S)
    multi.route_spectrum("first", "ksp", fetch=False)
    want = check(whole, fam, 1, S, need, "unsharded", "route", cands)
    given = random_cands(whole, fam, 1, S, np.random.RandomState(2))
    wg = check(whole, fam, 1, S, need, "unsharded", "given", given)
    assert multi.capacity_after_shape("route", "classes") == whole.capacity_after_shape("route", "classes")
    assert np.array_equal(multi.capacity_after("route", "classes"), want.reshape(n, -1))
    assert np.array_equal(multi.capacity_after("route", "total"), car.total(want))
    assert np.array_equal(multi.capacity_after("given", "total", candidates=given.astype(np.int32)), car.total(wg))
    assert multi.capacity_after("route", fetch=False) is None
    out = np.empty((n, 6), np.int32)
    assert multi.capacity_after("route", out=out) is out and np.array_equal(out, car.total(want))
    multi.close()
    whole.close()


def test_the_one_env_facades():
    import optical_rl_gym_amd as orl

    one = orl.RMSAEnv(topology=slot_agent.TOPOLOGY, seed=3, num_spectrum_resources=65, load=200)
    one.reset()
    one.batch.run("SAP_FF", 200)
    one.batch.route_spectrum("first", "ksp", fetch=False)
    cls, tot = one.capacity_after("route", "classes"), one.capacity_after("route", "total")
    assert cls.shape == (6, 76) and tot.shape == (6,) and np.array_equal(np.where((cls == -1).all(axis=1), -1, cls.sum(axis=1)), tot)
    assert np.array_equal(cls[5], one.network_capacity("counts")[0])
    g = one.capacity_after("given", "total", candidates=[[0, 0, 2], [9, 0, 2]])
    assert g.shape == (3,) and g[1] == -1 and g[0] >= g[2] >= 0
    one.close()


def test_refusals_leave_the_batch_as_it_was():
    import optical_rl_gym_amd as orl
    from optical_rl_gym_amd._lib import OrlError

    qos = orl.make("QoSConstrainedRA", topology=slot_agent.TOPOLOGY, num_envs=16, seeds=list(range(16)), load=10)
    for call in (lambda: qos.capacity_after("blocks"), lambda: qos.capacity_after("route", fetch=False), lambda: qos.capacity_after_shape("route")):
        with pytest.raises(OrlError, match="QoSConstrainedRA"):
            call()
    qos.close()
    env = ncg.make("rmsa_nsf_s65", n=5)[0]
    env.run("SAP_FF", 30)
    snap, flags = env.get_state(), env.flags().copy()
    for what, kw in (("source", dict(source="table")), ("layout", dict(layout="counts")), ("placement", dict(source="blocks", placement="middle"))):
        with pytest.raises(ValueError, match=what + " must be one of"):
            env.capacity_after(**kw)
    for args, msg in (((3, 1, 0, 1, None, 0, None), "unknown capacity_after source"), ((0, 1, 0, 2, None, 0, None), "unknown capacity_after layout"),
                      ((1, 1, 2, 1, None, 0, None), "unknown block placement"), ((1, 9, 0, 1, None, 0, None), "j = 1 .. 8")):
        assert env.lib.orl_batch_capacity_after(env._h, *args) != 0, args
        with pytest.raises(OrlError, match=msg):
            env._ck(env.lib.orl_batch_capacity_after(env._h, *args))
    with pytest.raises(OrlError, match=r"call orl_batch_route_spectrum \(route_spectrum\) first"):
        env.capacity_after("route")
    with pytest.raises(OrlError, match=r"call orl_batch_block_table \(block_table\) with j = 1 first"):
        env.capacity_after("blocks")
    env.block_table(2, fetch=False)
    with pytest.raises(OrlError, match=r"block_table\) with j = 4 first"):
        env.capacity_after("blocks", j=4)
    for bad in (np.zeros((5, 4, 2), np.int32), np.zeros((4, 4, 3), np.int32), np.zeros((5, 12), np.int32), np.zeros((5, 4, 3), np.float32)):
        with pytest.raises(ValueError, match="candidates must be an int array"):
            env.capacity_after("given", candidates=bad)
    with pytest.raises(ValueError, match="needs candidates"):
        env.capacity_after("given")
    with pytest.raises(ValueError, match="belong to the \"given\" source"):
        env.capacity_after("blocks", j=2, candidates=np.zeros((5, 4, 3), np.int32))
    for dev in ("capacity_after_classes", "capacity_after_total"):  # nothing was queued, no buffer exists
        with pytest.raises(OrlError, match=r"call capacity_after\("):
            env.device_tensor(dev)
    for out in (np.empty((5, 2), np.int32), np.empty((5, 3), np.int64), np.empty((4, 3), np.int32)):
        with pytest.raises(ValueError, match="out must be"):
            env.capacity_after("blocks", j=2, out=out)
    assert np.array_equal(env.get_state(), snap) and np.array_equal(env.flags(), flags)
    out = np.empty((5, 11), np.int32)
    assert env._capacity_after_last(0) == (0, 0) and env._capacity_after_last(1) == (0, 0)
    assert env.capacity_after("blocks", j=2, out=out) is out and (out[:, -1] >= 0).all()
    # the device rows are the last call's, whatever its Q: more candidates move to a larger buffer, fewer stay in it
    assert env._capacity_after_last(1) == (11, 12) and env._capacity_after_last(0) == (0, 0)
    small = env.device_tensor("capacity_after_total")
    assert small.shape == (5, 11) and small.stride() == (12, 1) and np.array_equal(small.cpu().numpy(), out)
    big = env.capacity_after("given", candidates=np.tile(np.array([[0, 0, 2]], np.int32), (5, 30, 1)))
    wide = env.device_tensor("capacity_after_total")
    assert wide.shape == (5, 31) and wide.stride() == (32, 1) and wide.data_ptr() != small.data_ptr() and np.array_equal(wide.cpu().numpy(), big)
    assert np.array_equal(env.capacity_after("blocks", j=2), out)
    again = env.device_tensor("capacity_after_total")
    assert again.shape == (5, 11) and again.data_ptr() == wide.data_ptr() and np.array_equal(again.cpu().numpy(), out)
    assert np.array_equal(small.cpu().numpy(), out)  # (the buffer that was replaced lives on with the batch)
    rm = ncg.make("rmcsa_c7_s64", n=3)[0]
    with pytest.raises(OrlError, match=r"call orl_batch_route_cores \(route_cores\) first"):
        rm.capacity_after("route")
    rm.close()
    env.close()
