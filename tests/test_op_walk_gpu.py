"""Interleaved state-changing calls on one batch against the oracle: the walks of tests/op_walk.py (every ordered pair of run, step
with the heuristic's and with an agent's actions, policy_step, step_async + step_wait, masked soft and full reset, seed, set_load,
set_state, copy_envs) on the device under every step route, with the queries (heuristics, action masks, path and link features,
completions, matrix observations, snapshots, rates, pending releases) between them.

After every state-changing op EVERY env equals the model's oracle env, bit for bit, on every read-back, and a stepping op's reward,
done, info and observation equal the oracle's; after every query its result equals the numpy restatement of the view computed
from the device's read-back state (or the oracle's answer), and the snapshot of the batch is byte for byte what it was before; at
the end of a walk check() passes and the pending releases of three envs equal those of one-env twin batches driven only by the
replayed lists of those envs.  No tolerance anywhere.

The view walks (ow.view_walks_of) put the five newer device calls inside the same walks: assign_spectrum, route_spectrum, route_cores,
block_table / select_blocks and release_horizons as queries, and "step_device" — the chooser call(s) with fetch=False, then step(None)
or step_async(None) + step_wait() — as a stepping kind, before and after every other kind, on the fresh and on the reseeded batch.
The release horizons are restated from pending() of EVERY env and, independently of it, held against the oracle's slot maps.

Every walk of every family runs on every route (the whole file takes about 90 s on an MI355X); RWA twice, at 65 wavelengths
(two-word rows, which never run out within a walk) and at 8 (where the heuristics find no free wavelength).  What a route means for a
walk: host-driven steps go through the forced step kernel and device-resident runs through the forced form of the persistent
kernel as long as the batch is fresh; a reseeded batch of every family but RWA runs on the per-env kernel whatever is forced, so
the three fresh walks are the ones that take the loop forms through every pair of kinds."""
import numpy as np
import pytest

from tests import complete_restate as cr
from tests import horizon_restate as hr
from tests import link_features_restate as lf
from tests import op_walk as ow
from tests import path_features_restate as pf
from tests import qos_obs_restate as qr
from tests import rmcsa_mask_restate as rr
from tests.helpers import IMPL_ENV, _exact_bits, _ran_pair_form, force_impl
from tests.mask_restate import restate_fast as mask_restate_fast
from tests.run_plans import expected_form, forms_of_family
from tests.test_copy_envs_gpu import _pending_sorted

pytestmark = pytest.mark.gpu

ORL_FLAG_MT2 = 4  # csrc/orl_device.h: the env was reseeded and draws its bit rates from its construction-time stream
HOST_ROUTES = ("wave64", "agent8", "split2")
QOS_ROUTES = ("qos_wave64", "qos_agent8")  # QoSConstrainedRA's two step kernels (tests/test_gpu_parity.py, qos_impl)
STEP_KERNEL = {"wave64": 0, "agent8": 2, "qos_wave64": 0, "qos_agent8": 2}  # the library's debug query: one wavefront / 8 lanes per env
SC_EV = 19  # word of the scalar record (section 0 of a snapshot, 32 words per env): high-water mark | count << 32 of the release table
VIEW_QUERIES = ("release_horizons", "block_table", "assign_spectrum", "route_spectrum", "route_cores", "select_blocks")


def routes_of(name):
    f = ow.FAMILIES[name]
    if f.fam == ow.QOS:
        return QOS_ROUTES
    loop = [r for r in forms_of_family(f.fam) if r != "persist_pair"] + (["persist_pair"] if name in ow.PAIR_FAMILIES else [])
    return HOST_ROUTES + tuple(loop)


def cases():
    """(family, walk, route): every walk on every route of the family"""
    return [(name, w, route) for name in sorted(ow.FAMILIES) for route in routes_of(name) for w in ow.WALK_NAMES + ow.view_walk_names(name)]


def force_route(monkeypatch, route):
    if route in QOS_ROUTES:
        for k in IMPL_ENV["wave64"]:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("ORL_AGENT_STEP", "1" if route == "qos_agent8" else "0")
    else:
        force_impl(monkeypatch, route)


def make(f, seeds, n=None):
    import optical_rl_gym_amd as orl

    return orl.make(f.fam, topology=ow.TOPO, num_envs=len(seeds) if n is None else n, seeds=list(seeds), **dict(f.kw, **f.dev_kw))


class Dev:
    """A batch (`b`) — or the shards of a sharded one — with the read-backs and the snapshot a sharded batch does not have itself."""

    def __init__(self, batch):
        self.b = batch
        self.shards = list(getattr(batch, "shards", [batch]))
        self.first = self.shards[0]

    def cat(self, name):
        return np.concatenate([getattr(s, name)() for s in self.shards])

    def get_state(self):
        return [s.get_state() for s in self.shards]

    def set_state(self, bufs):
        for s, buf in zip(self.shards, bufs):
            s.set_state(buf)

    def step_sync(self, actions):
        """the synchronous entry point where the batch has it by itself"""
        if hasattr(self.b, "step_sync_abi"):
            return self.b.step_sync_abi(actions, auto_reset=True)
        return self.b.step(actions, auto_reset=True)

    def sync(self):
        for s in self.shards:
            s.sync()

    def actions(self):
        """the actions buffer of every shard, read back once everything queued has run"""
        self.sync()
        return np.concatenate([s.device_tensor("actions").cpu().numpy() for s in self.shards])

    def write_actions(self, cols, values):
        """values [n, len(cols)] into columns `cols` of the actions buffer, every other column -9, queued on the batch's stream: what an
        agent on the GPU does before a chooser that reads its prefix from the buffer"""
        import torch

        lo = 0
        for s in self.shards:
            rows = np.full((s.num_envs, 4), -9, np.int32)
            rows[:, cols] = values[lo:lo + s.num_envs]
            lo += s.num_envs
            acts = s.device_tensor("actions")
            with torch.cuda.stream(s.torch_stream()):
                acts.copy_(torch.as_tensor(rows, device=acts.device))

    def holes(self):
        """envs whose release table has a hole: the high-water mark above the count (tests/test_release_horizons_gpu.py)"""
        count = 0
        for s in self.shards:
            assert s.state_layout()[0] == 256
            ev = s.get_state()[:s.num_envs * 256].view(np.uint64).reshape(s.num_envs, 32)[:, SC_EV]
            count += int(((ev & np.uint64(0xffffffff)) > (ev >> np.uint64(32))).sum())
        return count

    def readback(self):
        out = dict(counters=self.b.counters(), services=self.b.services(), active=self.b.active())
        if self.first.ENV_TYPE == 4:
            out["spectrum"] = np.stack([self.b.spectrum(i) for i in range(self.b.num_envs)])
            out["link_stats"] = np.stack([self.b.link_stats(i)[[0, 3]] for i in range(self.b.num_envs)])
        else:
            out.update(slots_packed=self.cat("slots_packed"), link_stats_all=self.cat("link_stats_all"), net_stats_all=self.cat("net_stats_all"))
        if self.first.obs_dim:
            out["observation"] = np.array(self.b.observation())
        return out


def same_state(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def compare(tag, k, kind, got, want):
    """every field of every env; a difference names walk, op index, op kind, env and field"""
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for what in want:
        g, w = np.asarray(got[what]), np.asarray(want[what])
        assert g.shape == w.shape, "%s: op %d (%s): %s has shape %r, the oracle's %r" % (tag, k, kind, what, g.shape, w.shape)
        if g.dtype.kind == "f" or w.dtype.kind == "f":
            gb, wb = (np.ascontiguousarray(x, np.float64).view(np.uint64) for x in (g, w))
        else:
            gb, wb = g, w
        if not np.array_equal(gb, wb):
            bad = [i for i in range(len(gb)) if not np.array_equal(gb[i], wb[i])]
            _exact_bits("%s: op %d (%s): env %d (%d envs differ: %r)" % (tag, k, kind, bad[0], len(bad), bad[:8]))(k, what, g[bad[0]], w[bad[0]])


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pending_is_the_slot_map(tag, dev, e, t, rec, avail):
    """The pending releases of env e hold exactly the services that occupy its slot maps: every record's block, on the links of
    its path in its core, laid into an empty map gives the device's map, no slot twice (avail: bool [C, links, S], True = free)."""
    topo = dev.first.topology
    C, E, S = avail.shape
    busy = np.zeros((C, E, S), np.int64)
    for r in rec:
        src, dst = divmod(int(r[0]), topo.n_nodes)
        p, lo, n, c = int(r[1]), int(r[2]), max(int(r[3]), 1), int(r[4])  # (RWA: one wavelength)
        assert p < int(topo.n_paths[src, dst]) and lo + n <= S and c < C, (tag, e, r)
        busy[c, topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])], lo:lo + n] += 1
    assert np.array_equal(busy, (~avail).astype(np.int64)), "%s: env %d: the pending releases are not what the slot map holds" % (tag, e)


def _same(tag, what, got, want):
    """ints and bools as they are, float32 on the bit patterns"""
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, what, got.dtype, got.shape, want.dtype, want.shape)
    g, w = (_u32(got), _u32(want)) if want.dtype == np.float32 else (got, want)
    if not np.array_equal(g, w):
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        e = int(bad[0])
        col = int(np.flatnonzero((g[e] != w[e]).ravel())[0])
        raise AssertionError("%s: %s: %d envs differ (%r); env %d, column %d: got %r, want %r"
                             % (tag, what, len(bad), bad[:8], e, col, got[e].ravel()[col], want[e].ravel()[col]))


def check_horizons(tag, dev, model, q, R, last, seen):
    """Both layouts against the restatement from pending() of every env, and — independently of pending() — against the oracle's state:
    H > 0 exactly on the busy slots of the oracle's AND-rows, 0 on the free ones, -1 on the rows of paths the pair does not have, the
    oracle's holding time in the last column, and nothing pending in envs a full reset has just emptied"""
    b, topo = dev.b, R.topo
    n, K, C, S = R.n, R.K, R.C, R.S
    pend = [b.pending(e) for e in range(n)]
    for e, (t, rec) in enumerate(pend):
        assert len(t) == len(rec) == model.envs[e].active()[0] and np.isfinite(t).all(), (tag, e)
        pending_is_the_slot_map(tag, dev, e, t, rec, R.avail[e])
    H = hr.slots_layout(pend, R.services, topo, C, S)
    got = b.release_horizons("slots")
    _same(tag, "slots", got, H)
    j, mod = q["j"], R.modulation(q["mod"])
    assert b.release_horizons_shape("blocks", j)[:3] == (K * C, 2 * j, K * C * 2 * j + 1)
    _same(tag, "blocks, j = %d, modulation %r" % (j, mod), b.release_horizons("blocks", j, mod), hr.blocks_layout(H, R.rows(q["mod"]), j, R.services))
    state = model.readback()
    oracle = ow.Restated(model.f, state["slots_packed"], state["services"])
    body = got[:, :-1].reshape(n, K * C, S)
    emptied = last is not None and last["kind"] == "reset_full"
    for e in range(n):
        src, dst = int(oracle.services[e, 2]), int(oracle.services[e, 3])
        live = int(topo.n_paths[src, dst])
        for p in range(live):
            links = topo.path_links[src, dst, p, :int(topo.path_hops[src, dst, p])]
            for c in range(C):
                free = oracle.avail[e, c][links, :].all(axis=0)
                row = body[e, p * C + c]
                assert np.array_equal(row > 0, ~free) and (row[free] == 0).all(), (tag, e, p, c)
        assert (body[e, live * C:] == -1.0).all() and not (body[e, :live * C] == -1.0).any(), (tag, e)
        if emptied and (last["mask"] is None or last["mask"][e]):
            assert (body[e, :live * C] == 0).all() and len(pend[e][0]) == 0, (tag, e)
    assert np.array_equal(_u32(got[:, -1]), _u32(oracle.services[:, 1].astype(np.float32))), tag
    if seen is not None:
        seen["horizon queries"] = seen.get("horizon queries", 0) + 1
        seen["envs with a hole"] = seen.get("envs with a hole", 0) + dev.holes()
        seen["over 64 pending"] = seen.get("over 64 pending", 0) + int(max(len(t) for t, _ in pend) > 64)


def check_view_query(tag, dev, model, q, last, seen):
    """a view query on the device against its restatement from the device's read-back state: actions and tables, bit for bit"""
    f, b, name = model.f, dev.b, q["q"]
    R = ow.Restated(f, dev.cat("slots_packed"), b.services())
    if name == "release_horizons":
        check_horizons(tag, dev, model, q, R, last, seen)
    elif name == "block_table":
        j, mod = q["j"], R.modulation(q["mod"])
        tab, msk = b.block_table(j, mod)
        want_tab, want_msk = R.block_table(j, q["mod"])
        _same(tag, "table, j = %d, modulation %r" % (j, mod), tab, want_tab)
        _same(tag, "mask, j = %d, modulation %r" % (j, mod), msk, want_msk)
        if f.fam == "DeepRMSA" and j == f.kw["j"]:
            _same(tag, "mask against action_mask(joint)", msk, b.action_mask("joint"))
    elif name == "assign_spectrum":
        if q["source"] == "buffer":
            dev.write_actions([0], q["paths"][:, None])
            got = b.assign_spectrum(q["rule"], paths=None, n_given=1)
        else:
            got = b.assign_spectrum(q["rule"], paths=q["paths"])
        _same(tag, "%s, paths from %s" % (q["rule"], q["source"]), got, R.assign(q["rule"], q["paths"]))
        _same(tag, "the actions buffer", dev.actions(), got)
    elif name == "route_spectrum":
        for rule, route in q["pairs"]:
            acts, tab = b.route_spectrum(rule, route, table=True)
            want, want_tab = R.route_spectrum(rule, route)
            _same(tag, "%s, %s: table" % (rule, route), tab, want_tab)
            _same(tag, "%s, %s: actions" % (rule, route), acts, want)
    elif name == "route_cores":
        g, mod = q["given"], R.modulation(q["mod"])
        paths, cores = (None if g is None else g[:, 0]), (None if g is None or g.shape[1] < 2 else g[:, 1])
        for rule, route in q["pairs"]:
            acts, tab = b.route_cores(rule, route, paths=paths, cores=cores, modulation=mod, table=True)
            want, want_tab = R.route_cores(rule, route, g, q["mod"])
            what = "%s, %s, prefix of %d, modulation %r" % (rule, route, 0 if g is None else g.shape[1], mod)
            _same(tag, what + ": table", tab, want_tab)
            _same(tag, what + ": actions", acts, want)
    else:
        assert name == "select_blocks"
        idx, want = R.select(q)
        mod = R.modulation(q["mod"])
        _same(tag, "j = %d, %s, modulation %r" % (q["j"], q["placement"], mod), b.select_blocks(idx, q["j"], mod, q["placement"]), want)


def check_query(tag, k, dev, model, q, last=None, seen=None):
    """the query (after op k) on the device against its restatement from the device's read-back state, or against the oracle's answer"""
    f, b, name = model.f, dev.b, q["q"]
    topo = dev.first.topology
    if name == "get_state":
        return
    if name in VIEW_QUERIES:
        check_view_query(tag, dev, model, q, last, seen)
        return
    if name == "rates":
        la, lh = b.rates()
        want_a, want_h = model.lambdas()
        compare(tag, k, name, dict(lambda_arrival=la, lambda_holding=lh), dict(lambda_arrival=want_a, lambda_holding=want_h))
        return
    if name == "pending":
        active = b.active()
        qos = dev.first.ENV_TYPE == 4
        if not qos:
            avail = rr.unpack_cores(dev.cat("slots_packed"), dev.first.num_spatial_resources, topo.n_links, dev.first.num_spectrum_resources)
        for e in q["envs"]:
            t, rec = b.pending(e)
            assert len(t) == len(rec) == active[e] == model.envs[e].active()[0], (tag, name, e)
            assert np.isfinite(t).all(), (tag, name, e)
            if not qos:
                pending_is_the_slot_map(tag, dev, e, t, rec, avail[e])
        return
    if name.startswith("policy:"):
        compare(tag, k, name, dict(actions=np.array(b.policy(name[7:]))), dict(actions=model.policy(name[7:])))
        return
    if name == "observation":
        compare(tag, k, name, dict(observation=np.array(b.observation())), dict(observation=model.readback()["observation"]))
        return
    services = b.services()
    if name == "matrix_observation_with_paths":
        spectrum = np.stack([b.spectrum(i) for i in range(b.num_envs)])
        want = qr.restate_fast(spectrum, services[:, 2:5].astype(np.int64), topo, f.kw["num_spectrum_resources"], 5)
        got = b.matrix_observation_with_paths()
        assert got.dtype == np.uint8 and np.array_equal(got, want), (tag, name, np.flatnonzero((got != want).any(axis=1))[:8])
        return
    S, C = dev.first.num_spectrum_resources, dev.first.num_spatial_resources
    avail = rr.unpack_cores(dev.cat("slots_packed"), C, topo.n_links, S)  # bool [n, C, links, S]
    env_type = dev.first.ENV_TYPE
    if name == "matrix_observation":
        want = np.concatenate([o.matrix_observation() for o in model.envs])
        got = b.matrix_observation()
        assert got.shape == want.shape and np.array_equal(got, want), (tag, name, np.flatnonzero((got != want).any(axis=1))[:8])
        from_state = np.concatenate([np.zeros((b.num_envs, 2 * topo.n_nodes), np.uint8), avail.reshape(b.num_envs, -1).astype(np.uint8)], axis=1)
        assert np.array_equal(got[:, 2 * topo.n_nodes:], from_state[:, 2 * topo.n_nodes:]), (tag, name)
    elif name == "path_features":
        tables = rr.tables_of(dev.first) if env_type == 3 else None
        want = np.float32(pf.restate_fast(env_type, avail, services, topo, q["j"], tables, -1))
        got = b.path_features(q["j"])
        assert got.dtype == np.float32 and got.shape == want.shape, (tag, name)
        assert np.array_equal(_u32(got), _u32(want)), (tag, name, q["j"], np.flatnonzero((_u32(got) != _u32(want)).any(axis=1))[:8])
    elif name == "link_features":
        want = np.float32(lf.restate_fast(env_type, avail, services, topo, dev.cat("link_stats_all")))
        got = b.link_features()
        assert got.dtype == np.float32 and got.shape == want.shape, (tag, name)
        assert np.array_equal(_u32(got), _u32(want)), (tag, name, np.flatnonzero((_u32(got) != _u32(want)).any(axis=1))[:8])
    elif name in ("mask:joint", "mask:path"):
        layout = name[5:]
        want = mask_restate_fast(env_type, avail[:, 0], services, topo, 5, S, f.kw.get("j", 1), 50.0 if env_type == 2 else 12.5,
                                 bool(f.kw.get("allow_rejection")), layout)
        got = b.action_mask(layout)
        assert got.dtype == np.bool_ and got.shape == want.shape, (tag, name)
        assert np.array_equal(got, want), (tag, name, np.flatnonzero((got != want).any(axis=1))[:8])
    else:
        tab = rr.tables_of(dev.first)
        pv = rr.prov_all(avail, services, topo, tab)
        if name == "complete_actions":
            want = cr.complete(pv, services, topo, tab, q["g"], q["given"])
            got = b.complete_actions(given=q["given"], n_given=q["g"])
            assert got.dtype == np.int32 and got.shape == want.shape, (tag, name)
        else:
            layout = name[5:]
            given = q.get("given")
            want = rr.restate_rmcsa_fast(None, None, topo, tab, layout, given=given, allow_rejection=bool(f.kw.get("allow_rejection")), pv=pv)
            got = b.action_mask(layout, given=given)
            assert got.dtype == np.bool_ and got.shape == want.shape, (tag, name)
        assert np.array_equal(got, want), (tag, name, q.get("g"), np.flatnonzero((got != want).any(axis=1))[:8])


def run_on_route(tag, k, b, rec, fam, route):
    """a device-resident run; on a batch that was never reseeded (route given) it went the way the route says: no launch of the
    persistent kernel on the per-env routes, else k_persist alone, in the form asked for where the family is built in it (not
    "persist_lds": where the LDS-resident form does not fit the configuration the library's default form runs)"""
    st = b.run(rec["policy"], rec["n"])
    if route is None or route in QOS_ROUTES:
        return
    what = "%s: op %d (run of %d)" % (tag, k, rec["n"])
    names, form = [n for n, _ in st.kernels()], int(b.lib.orl_batch_debug_persist_form(b._h))
    if route in ("wave64", "split2"):
        assert names == [] and form == -1, (what, names, form)
        return
    assert names == ["k_persist"] and form >= 0, (what, names, form)
    choice = b.persist_choice(b.num_envs, tuned=b.specialised)
    assert choice is not None and form == choice[0], (what, form, choice)
    if route in ("persist_global", "persist_rd"):
        assert form == expected_form(fam, route), (what, form)
    if route == "persist_pair":
        assert b.specialised and _ran_pair_form(b) == (fam.fam != "RMCSA"), (what, form)


def choose_on_device(dev, rec):
    """the chooser call(s) of a step_device op: the action stays on the device"""
    b, v = dev.b, rec["variant"]
    if v == "route_spectrum":
        out = b.route_spectrum(rec["rule"], rec["route"], fetch=False)
    elif v == "assign_host":
        out = b.assign_spectrum(rec["rule"], paths=rec["paths"], fetch=False)
    elif v == "policy_assign":  # the path through column 0
        assert b.policy(rec["policy"], fetch=False) is None
        out = b.assign_spectrum(rec["rule"], paths=None, n_given=1, fetch=False)
    elif v == "select_host":
        out = b.select_blocks(rec["indices"], rec["j"], rec["modulation"], rec["placement"], fetch=False)
    elif v == "select_buffer":  # the index through column 0
        dev.write_actions([0], rec["indices"][:, None])
        out = b.select_blocks(None, rec["j"], rec["modulation"], rec["placement"], fetch=False)
    elif v == "route_cores_host":
        g = rec["given"]
        paths, cores = (None if g is None else g[:, 0]), (None if g is None or g.shape[1] < 2 else g[:, 1])
        out = b.route_cores(rec["rule"], rec["route"], paths=paths, cores=cores, modulation=rec["modulation"], fetch=False)
    else:  # path and core through columns 0 and 2
        assert v == "complete_route_cores" and b.complete_actions(given=rec["given"], n_given=2, fetch=False) is None
        out = b.route_cores(rec["rule"], rec["route"], n_given=2, fetch=False)
    assert out is None


def apply_op(tag, k, dev, rec, route=None):
    """the op on the device, as the model made it; a stepping op's answers against the oracle's"""
    b, kind = dev.b, rec["kind"]
    if kind == "step_device":
        a, (obs, reward, done, info) = rec["actions"], rec["out"]
        choose_on_device(dev, rec)
        compare(tag, k, "%s (%s): the actions buffer before the step" % (kind, rec["variant"]), dict(actions=dev.actions()), dict(actions=a))
        if rec["form"] == "step":
            out = b.step(None, auto_reset=True)
        else:
            b.step_async(None, auto_reset=True)
            out = b.step_wait()
        got, want = dict(reward=out[1], done=out[2], info=out[3]), dict(reward=reward, done=done, info=info)
        if obs is not None:
            got["observation of the step"], want["observation of the step"] = out[0], obs
        compare(tag, k, "%s (%s, %s)" % (kind, rec["variant"], rec["form"]), got, want)
        if route is not None and route[1] in STEP_KERNEL:
            assert int(b.lib.orl_batch_debug_step_kernel(b._h)) == STEP_KERNEL[route[1]], (tag, k, rec["variant"])
    elif kind == "run" and route is not None:
        run_on_route(tag, k, b, rec, route[0], route[1])
    elif kind == "run":
        b.run(rec["policy"], rec["n"])
    elif kind in ow.STEPPING:
        a, (obs, reward, done, info) = rec["actions"], rec["out"]
        width = 4 if dev.first.ENV_TYPE == 3 else (1 if dev.first.ENV_TYPE in (1, 4) else 2)
        got = {}
        if kind == "step_heur":  # the heuristic's actions are the device's own
            got["actions"] = np.array(b.policy(rec["policy"]))
            out = b.step(got["actions"][:, :width], auto_reset=True)
        elif kind == "step_agent":
            out = dev.step_sync(a[:, :width])
        elif kind == "step_async":
            b.step_async(a[:, :width], auto_reset=True)
            out = b.step_wait()
        else:
            out = b.policy_step(rec["policy"], auto_reset=True)
            got["actions"], out = np.array(out[0]), out[1:]
        got.update(reward=out[1], done=out[2], info=out[3])
        want = dict(reward=reward, done=done, info=info)
        if "actions" in got:
            want["actions"] = a
        if obs is not None:
            got["observation of the step"], want["observation of the step"] = out[0], obs
        compare(tag, k, kind, got, want)
    elif kind in ("reset_soft", "reset_full"):
        b.reset(full=kind == "reset_full", mask=rec["mask"])
    elif kind == "seed":
        b.seed(rec["seeds"], mask=rec["mask"])
    elif kind == "set_load":
        b.set_load(load=rec["load"], mean_service_holding_time=rec["mht"], mask=rec["mask"])
    elif kind == "copy_envs":
        b.copy_envs(rec["src"], rec["dst"])
    else:
        raise ValueError(kind)


def drive(tag, dev, model, walk, route=None, seen=None):
    """The walk on the batch and on the model; route = (family, forced route) of a single batch: every run of a fresh walk is checked
    to have gone that way.  seen: a dict the horizon queries count into.  -> the ops driven"""
    route = route if walk.fresh else None
    rwa = dev.first.ENV_TYPE == 2
    snaps, k, rec = [], 0, None
    compare(tag, -1, "construction", dev.readback(), model.readback())
    for what, it in walk.items:
        if what == "q":
            before, flags = dev.get_state(), dev.b.flags()
            check_query("%s: after op %d: query %s" % (tag, k - 1, it["q"]), k - 1, dev, model, it, rec, seen)
            assert same_state(dev.get_state(), before), "%s: after op %d: query %s changed the state" % (tag, k - 1, it["q"])
            assert np.array_equal(dev.b.flags(), flags), "%s: after op %d: query %s changed the flags" % (tag, k - 1, it["q"])
            if it["q"] == "get_state":
                snaps.append(before)
                model.snapshot()
            continue
        rec = model.apply(it)
        if it["kind"] == "set_state":
            dev.set_state(snaps[it["snapshot"]])
        else:
            apply_op(tag, k, dev, rec, route)
        got, want = dev.readback(), model.readback()
        got["flags"], want["flags"] = dev.b.flags(), np.where(model.reseeded() & (not rwa), ORL_FLAG_MT2, 0)
        compare(tag, k, it["kind"], got, want)
        k += 1
    dev.b.check()
    return k


def twins_agree(tag, dev, model, envs):
    """the pending releases of `envs` against one-env twin batches, constructed fresh and driven only by the envs' replayed lists"""
    chk = _exact_bits(tag + ": twin")
    for e in envs:
        lst = model.lists[e]
        twin = make(model.f, [lst[0][1]])
        for entry in lst[1:]:
            what = entry[0]
            if what == "reset":
                twin.reset(full=entry[1])
            elif what == "seed":
                twin.seed([entry[1]])
            elif what == "rates":
                twin.set_load(load=entry[1], mean_service_holding_time=entry[2])
            elif what == "step":
                twin.step(np.array([entry[1]], np.int32)[:, :len(model.bounds)], auto_reset=True)
            else:
                twin.run(entry[1], entry[2])
        twin.check()
        t_d, rec_d = _pending_sorted(dev.b, e)
        t_t, rec_t = _pending_sorted(twin, 0)
        chk(e, "pending release times", t_d, t_t)
        chk(e, "pending release records", rec_d, rec_t)
        chk(e, "active", len(t_d), model.envs[e].active()[0])
        twin.close()


def twin_envs(model, walk):
    """three envs: the first, the last, and a destination of the walk's last copy (a walk without one: an env in the middle)"""
    copies = [it for what, it in walk.items if what == "op" and it["kind"] == "copy_envs"]
    dst = [int(d) for d in (copies[-1]["dst"] if copies else ()) if 0 < int(d) < model.n - 1]
    return [0, dst[-1] if dst else model.n // 2, model.n - 1]


@pytest.mark.parametrize("name,walk,route", cases(), ids=["%s-%s-%s" % c for c in cases()])
def test_walk_equals_the_oracle(name, walk, route, monkeypatch):
    force_route(monkeypatch, route)
    f = ow.FAMILIES[name]
    w = ow.walk_of(name, walk)
    tag = "%s, walk %s, %s" % (name, walk, route)
    model = ow.Model(name)
    dev = Dev(make(f, ow.seeds_of(f)))
    if route in STEP_KERNEL:
        assert int(dev.b.lib.orl_batch_debug_step_kernel(dev.b._h)) == STEP_KERNEL[route], tag
    seen = {}
    assert drive(tag, dev, model, w, (f, route), seen) == len(w.kinds())
    if seen:  # (reported, not asserted: whether a route leaves holes in the release table is the route's business)
        print("%s: %r" % (tag, seen))
    twins_agree(tag, dev, model, twin_envs(model, w))
    dev.b.close()


def test_the_routes_are_the_ones_asked_for():
    assert set(routes_of("rmsa")) == {"wave64", "agent8", "split2", "persist", "persist_global", "persist_lds", "persist_rd", "persist_pair"}
    assert set(routes_of("rmcsa")) == {"wave64", "agent8", "split2", "persist", "persist_global", "persist_pair"}
    assert routes_of("rwa") == routes_of("rwa_s8") == routes_of("deeprmsa") == tuple(r for r in routes_of("rmsa") if r != "persist_pair")
    assert routes_of("qos") == QOS_ROUTES
    for name in ow.FAMILIES:
        assert all((name, w, r) in cases() for r in routes_of(name) for w in ow.WALK_NAMES)
        assert ow.view_walk_names(name) == (() if name == "qos" else ow.VIEW_WALK_NAMES)
        assert all((name, w, r) in cases() for r in routes_of(name) for w in ow.view_walk_names(name))


SHARD_CUT = 13


def test_sharded_walk_equals_the_oracle_and_the_unsharded_batch():
    """RMSA in two shards on one GPU, cut at 13 | 27: global indices and masks go through sharding.py, copies stay inside a shard.
    The sharded and the unsharded batch are driven by the same walk, each against a model of its own: equal to the oracle on every
    read-back after every op, they equal each other.  Then the same with the view walk views_fresh: the choosers, their hand-offs
    through the actions buffer of every shard, the tables and the release horizons of the sharded batch."""
    from optical_rl_gym_amd.sharding import MultiDeviceBatch

    name = "rmsa"
    f = ow.FAMILIES[name]
    seeds = ow.seeds_of(f)
    segments = ((0, SHARD_CUT), (SHARD_CUT, f.batch))
    for walk in ("fresh1", "views_fresh"):
        w = ow.walk_of(name, walk, segments)
        copies = [it for what, it in w.items if what == "op" and it["kind"] == "copy_envs"]
        assert copies and all((s < SHARD_CUT) == (d < SHARD_CUT) for it in copies for s, d in zip(it["src"], it["dst"]))
        if walk == "fresh1":
            assert any(s < SHARD_CUT for it in copies for s in it["src"]) and any(s >= SHARD_CUT for it in copies for s in it["src"])
        sharded = Dev(MultiDeviceBatch.from_shards([make(f, seeds[:SHARD_CUT]), make(f, seeds[SHARD_CUT:])]))
        whole = Dev(make(f, seeds))
        for tag, dev in (("rmsa in shards of 13 and 27, walk %s" % walk, sharded), ("rmsa unsharded, the sharded walk %s" % walk, whole)):
            model = ow.Model(name)
            assert drive(tag, dev, model, w) == len(w.kinds())
            twins_agree(tag, dev, model, twin_envs(model, w))
        compare("sharded against unsharded", len(w.kinds()), "end", sharded.readback(), whole.readback())
        if walk == "views_fresh":  # the five calls on the final state, one batch against the other
            tag = "sharded against unsharded, the five calls"
            a, b = sharded.b, whole.b
            paths = np.arange(f.batch, dtype=np.int32) % 6 - 1
            for rule, route in (("min_cuts", "best"), ("most_used", "least_loaded")):
                for x, y, what in zip(a.route_spectrum(rule, route, table=True), b.route_spectrum(rule, route, table=True), ("actions", "table")):
                    _same(tag, "route_spectrum %s %s: %s" % (rule, route, what), x, y)
            for rule in ("exact", "most_used"):
                _same(tag, "assign_spectrum " + rule, a.assign_spectrum(rule, paths=paths), b.assign_spectrum(rule, paths=paths))
            for x, y, what in zip(a.block_table(4), b.block_table(4), ("table", "mask")):
                _same(tag, "block_table: " + what, x, y)
            idx = np.arange(f.batch, dtype=np.int32) % 22 - 1
            _same(tag, "select_blocks", a.select_blocks(idx, 4, placement="last"), b.select_blocks(idx, 4, placement="last"))
            for layout, j in (("slots", 1), ("blocks", 3)):
                x, y = a.release_horizons(layout, j), b.release_horizons(layout, j)
                assert (x[:, :-1] > 0).any(), (tag, layout)
                _same(tag, "release_horizons " + layout, x, y)
        sharded.b.close()
        whole.b.close()
