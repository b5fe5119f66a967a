"""Shared helpers for the parity tests: golden-trace loading and trace replay, the step implementations a test can force, and the
exact comparison."""
import glob
import json
import os
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_names(prefix="g"):
    """g* = step traces (gen_golden.py), w* = wrappers / seed / full reset (gen_golden_wrappers.py), v* = seed() on a live env of
    the other families (gen_golden_seed.py).  A trace is <letter><number>_<what>.npz: the tables of host decisions beside them
    (view_plan.npz, run_plan.npz, ...) are no traces."""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, prefix + "[0-9]*.npz")))


VIEW_PLAN_FIELDS = ("dim", "rows", "width", "pitch", "elem_bytes", "ok", "waves", "block", "grid", "lds_bytes", "staged", "chunk", "counted")
VIEWS = ("action_mask", "rmcsa_mask", "complete", "assign", "path_features", "link_features", "matrix_paths_obs")


def view_plan_of(env, view, arg=0):
    """The shape and launch plan of a view of this batch (include/orl.h, orl_debug_view_plan) as a dict over VIEW_PLAN_FIELDS: what a
    GPU case asserts so that it keeps reaching the branch of the plan it is there for.  view: a name of VIEWS; arg: the mask
    layout id, the assignment rule id, the path features' j."""
    import ctypes

    cfg, d = env._cfg, env._desc
    out = (ctypes.c_int32 * len(VIEW_PLAN_FIELDS))()
    n = env.lib.orl_debug_view_plan(cfg.env_type, env.lib.orl_batch_row_words(env._h), env.num_envs, d.n_nodes, d.n_links, d.k_paths,
                                    cfg.num_spatial_resources, cfg.num_spectrum_resources, max(1, cfg.j), d.n_modulations, VIEWS.index(view), arg, out)
    assert n == len(VIEW_PLAN_FIELDS)
    return dict(zip(VIEW_PLAN_FIELDS, out))


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def crc_slots(slots_u8):
    """CRC32 of the dense 0/1 availability array, flattened [core][link][slot] (cores omitted when 1)."""
    return zlib.crc32(np.ascontiguousarray(slots_u8, np.uint8).tobytes())


def replay(env, g, check, n_steps=None):
    """Replay golden trace `g` on a 1-env batch object `env` (oracle or product; same method names).

    check(t, what, got, expected) is called for every compared quantity.
    """
    meta = g["meta"]
    T = meta["n_steps"] if n_steps is None else min(n_steps, meta["n_steps"])
    use_policy = meta["policy"] != "ACTIONS"
    for t in range(T):
        if g["reset_before"][t]:
            env.reset(full=False)
        check(t, "svc", env.services()[0], g["svc"][t])
        if "obs" in g:
            check(t, "obs", env.observation()[0], g["obs"][t])
        if use_policy:
            a = env.policy(meta["policy"])
            width = g["actions"].shape[1]
            check(t, "action", np.asarray(a[0, :width], np.int64), g["actions"][t])
        else:
            a = g["actions"][t][None, :]
        _, reward, done, info = env.step(a)
        check(t, "reward", reward[0], g["reward"][t])
        check(t, "done", int(done[0]), int(g["done"][t]))
        check(t, "info", info[0, : g["info"].shape[1]], g["info"][t])
        check(t, "counters", env.counters()[0], g["counters"][t])
        sl = env.slots(0)
        if sl.shape[0] == 1:
            sl = sl[0]
        check(t, "crc", crc_slots(sl), int(g["crc"][t]))
        check(t, "n_active", env.n_active(0), int(g["n_active"][t]))
        if (t + 1) in meta["snapshot_steps"]:
            s = t + 1
            packed = np.packbits(sl, axis=-1, bitorder="little")
            check(t, "snap_slots", packed, g["snap%d_slots" % s])
            check(t, "snap_link_stats", env.link_stats(0), g["snap%d_link_stats" % s])
            check(t, "snap_net_stats", env.net_stats(0), g["snap%d_net_stats" % s])
            if "snap%d_path_action_probability" % s in g:  # RWA vector infos ride behind the 2 scalars
                pa = g["snap%d_path_action_probability" % s]
                wa = g["snap%d_wavelength_action_probability" % s]
                check(t, "path_action_probability", info[0, 2 : 2 + len(pa)], pa)
                check(t, "wavelength_action_probability", info[0, 2 + len(pa) : 2 + len(pa) + len(wa)], wa)
    if T == meta["n_steps"]:
        check(T, "svc", env.services()[0], g["svc"][T])


def replay_w(env, g, check):
    """Replay a w* fixture (oracle/gen_golden_wrappers.py) on a 1-env batch object `env` (oracle or product):
    PathOnlyFirstFitAction through policy "PATH_FF", SimpleMatrixObservation through matrix_observation(), seed() and
    full resets at the recorded steps, the 2-D action histograms at the end."""
    meta = g["meta"]
    events = {int(k): v for k, v in meta.get("events", {}).items()}
    wrapper = meta.get("wrapper")
    done = True
    for t in range(meta["n_steps"]):
        for kind, arg in events.get(t, []):
            if kind == "seed":
                env.seed([arg])
            else:
                env.reset(full=True)
                done = False
        if done:
            env.reset(full=False)
        check(t, "svc", env.services()[0], g["svc"][t])
        if "obs_bits" in g:
            obs = np.asarray(env.matrix_observation()[0], np.uint8)
            check(t, "matrix_obs", np.packbits(obs, bitorder="little"), g["obs_bits"][t])
            assert obs.size == int(g["obs_dim"])
        if wrapper == "PathOnlyFirstFitAction":
            a = env.policy("PATH_FF", paths=[int(g["choice"][t][0])])
        else:
            a = env.policy(meta["policy"])
        width = g["actions"].shape[1]
        check(t, "action", np.asarray(a[0, :width], np.int64), g["actions"][t])
        _, reward, done_a, info = env.step(a)
        done = bool(done_a[0])
        check(t, "reward", reward[0], g["reward"][t])
        check(t, "done", int(done), int(g["done"][t]))
        check(t, "info", info[0, : g["info"].shape[1]], g["info"][t])
        check(t, "counters", env.counters()[0], g["counters"][t])
        sl = env.slots(0)
        if sl.shape[0] == 1:
            sl = sl[0]
        check(t, "crc", crc_slots(sl), int(g["crc"][t]))
        check(t, "n_active", env.n_active(0), int(g["n_active"][t]))
    T = meta["n_steps"]
    check(T, "svc", env.services()[0], g["svc"][T])
    sl = env.slots(0)
    if sl.shape[0] == 1:
        sl = sl[0]
    check(T, "final_slots", np.packbits(sl, axis=-1, bitorder="little"), g["final_slots"])
    check(T, "final_link_stats", env.link_stats(0), g["final_link_stats"])
    check(T, "final_net_stats", env.net_stats(0), g["final_net_stats"])
    if "actions_output" in g:
        out, taken = env.action_histograms_of(0)
        ro, rt = g["actions_output"], g["actions_taken"]
        check(T, "actions_output", out[: ro.shape[0], : ro.shape[1]], ro)
        check(T, "actions_taken", taken[: rt.shape[0], : rt.shape[1]], rt)
        assert out.sum() == ro.sum() and taken.sum() == rt.sum()


def replay_h(env, g, check):
    """Replay the h1 fixture (oracle/gen_golden_hist.py): RMCSA under a stored action stream with a full reset in the
    middle; the 4-D actions_output / actions_taken arrays (rmcsa_env.py:145-180) right before the reset and at the end,
    compared through their non-zero cells."""
    meta = g["meta"]

    def cells(a):
        flat = np.asarray(a, np.int64).ravel()
        idx = np.flatnonzero(flat)
        return np.stack([idx, flat[idx]], 1)

    done = True
    for t in range(meta["n_steps"]):
        if t == meta["reset_at"]:
            out, taken = env.action_histograms_of(0)
            assert list(out.shape) == meta["shape"]
            check(t, "actions_output before reset", cells(out), g["out_before"])
            check(t, "actions_taken before reset", cells(taken), g["taken_before"])
            env.reset(full=True)
            done = False
        if done:
            env.reset(full=False)
        _, reward, done_a, _ = env.step(g["actions"][t][None, :])
        done = bool(done_a[0])
        check(t, "reward", reward[0], g["reward"][t])
    out, taken = env.action_histograms_of(0)
    check(meta["n_steps"], "actions_output", cells(out), g["out_final"])
    check(meta["n_steps"], "actions_taken", cells(taken), g["taken_final"])
    check(meta["n_steps"], "counters", env.counters()[0], g["counters"])


def replay_q(env, g, check):
    """Replay a q* fixture (QoSConstrainedRA, oracle/gen_golden_qos.py) on a 1-env batch object `env`."""
    meta = g["meta"]
    use_policy = meta["policy"] != "ACTIONS"
    for t in range(meta["n_steps"]):
        if g["reset_before"][t]:
            env.reset(full=False)
        check(t, "svc", env.services()[0], g["svc"][t])
        if use_policy:
            a = env.policy(meta["policy"])
            check(t, "action", np.asarray(a[0, :1], np.int64), g["actions"][t])
        else:
            a = g["actions"][t][None, :]
        _, reward, done, info = env.step(a)
        check(t, "reward", reward[0], g["reward"][t])
        check(t, "done", int(done[0]), int(g["done"][t]))
        check(t, "info", info[0, :2], g["info"][t])
        check(t, "counters", env.counters()[0, :4], g["counters"][t][:4])
        check(t, "spectrum", env.spectrum(0), g["spectrum"][t])
        check(t, "n_active", env.n_active(0), int(g["n_active"][t]))
        if (t + 1) in meta["snapshot_steps"]:
            ls = env.link_stats(0)
            ref = g["snap%d_link_stats" % (t + 1)]
            check(t, "utilization", ls[0], ref[0])
            check(t, "last_update", ls[3], ref[3])
    check(meta["n_steps"], "svc", env.services()[0], g["svc"][meta["n_steps"]])


def replay_v(env, g, check, on_event=None):
    """Replay a v* fixture (seed() on a live env, oracle/gen_golden_seed.py) on a 1-env batch object `env` (oracle or
    product): seed() and full resets at the recorded steps as replay_w does, with the DeepRMSA observation of every step, the
    QoSConstrainedRA quantities of replay_q, link statistics at the recorded steps, and at the end the slot map, the network
    statistics and — discrete bit rates — the four bit-rate histograms through the info values that are made of them.
    on_event(t, kind) is called after every event."""
    meta = g["meta"]
    qos = meta["env"] == "QoSConstrainedRA"
    events = {int(k): v for k, v in meta["events"].items()}
    width = g["actions"].shape[1]
    done = True
    info = None
    for t in range(meta["n_steps"]):
        for kind, arg in events.get(t, []):
            if kind == "seed":
                env.seed([arg])
            else:
                env.reset(full=True)
                done = False
            if on_event is not None:
                on_event(t, kind)
        if done:
            env.reset(full=False)
        check(t, "svc", env.services()[0], g["svc"][t])
        if "obs" in g:
            check(t, "obs", env.observation()[0], g["obs"][t])
        a = env.policy(meta["policy"])
        check(t, "action", np.asarray(a[0, :width], np.int64), g["actions"][t])
        _, reward, done_a, info = env.step(a)
        done = bool(done_a[0])
        check(t, "reward", reward[0], g["reward"][t])
        check(t, "done", int(done), int(g["done"][t]))
        check(t, "info", info[0, : g["info"].shape[1]], g["info"][t])
        check(t, "n_active", env.n_active(0), int(g["n_active"][t]))
        if qos:
            check(t, "counters", env.counters()[0, :4], g["counters"][t][:4])
            check(t, "spectrum", env.spectrum(0), g["spectrum"][t])
        else:
            check(t, "counters", env.counters()[0], g["counters"][t])
            sl = env.slots(0)
            if sl.shape[0] == 1:
                sl = sl[0]
            check(t, "crc", crc_slots(sl), int(g["crc"][t]))
        if (t + 1) in meta["snapshot_steps"]:
            ls, ref = env.link_stats(0), g["snap%d_link_stats" % (t + 1)]
            if qos:
                check(t, "utilization", ls[0], ref[0])
                check(t, "last_update", ls[3], ref[3])
            else:
                check(t, "link_stats", ls, ref)
    T = meta["n_steps"]
    check(T, "svc", env.services()[0], g["svc"][T])
    if not qos:
        sl = env.slots(0)
        if sl.shape[0] == 1:
            sl = sl[0]
        check(T, "final_slots", np.packbits(sl, axis=-1, bitorder="little"), g["final_slots"])
        check(T, "final_net_stats", env.net_stats(0), g["final_net_stats"])
    if "bit_rate_histograms" in g:
        # rmsa_env.py:258-282: bit_rate_blocking_<rate> = (requested - provisioned) / requested of the rate's two histograms,
        # fairness = max - min of them.  The recorded requested histogram already counts the pending service (drawn after the
        # last step's info was made, rmsa_env.py:283 / 545-580): taken out here
        req, prov = g["bit_rate_histograms"][0].astype(np.float64), g["bit_rate_histograms"][1].astype(np.float64)
        req[list(g["bit_rates"]).index(int(g["svc"][T][4]))] -= 1
        blocking = np.where(req > 0, (req - prov) / np.where(req > 0, req, 1.0), 0.0)
        keys = meta["info_keys"]
        col = [keys.index("bit_rate_blocking_%d" % int(r)) for r in g["bit_rates"]]
        check(T, "blocking per bit rate from the recorded histograms", info[0, col], blocking)
        check(T, "fairness from the recorded histograms", info[0, keys.index("fairness")], blocking.max() - blocking.min())


# ---- step implementations -------------------------------------------------------------------------------------------------
# Device-resident runs go through the persistent kernel (k_persist) wherever it applies, host-driven step() through the
# one-wavefront-per-env kernel (k_step).  The small parity cases run against every implementation by forcing it
# (ORL_STEP_IMPL, ORL_PERSIST and ORL_AGENT_STEP are read when a batch is created; the form overrides — ORL_PERSIST_VARIANT,
# _INNER, _RW — at every launch of the persistent kernel): "wave64" = k_step for everything, "persist" = the default, "split2" = the
# phases of the persistent kernel as two separate launches (liborlgpu_alt.so, the -DORL_ALT_IMPLS build).
IMPLS = ["wave64", "split2", "persist", "persist_global", "persist_lds", "agent8", "persist_pair", "persist_rd"]
IMPL_ENV = {"wave64": dict(ORL_STEP_IMPL="64", ORL_PERSIST="0", ORL_LIB_VARIANT="default", ORL_PERSIST_VARIANT=None, ORL_PERSIST_INNER=None),
            "split2": dict(ORL_STEP_IMPL="2", ORL_PERSIST="0", ORL_LIB_VARIANT="alt", ORL_PERSIST_VARIANT=None, ORL_PERSIST_INNER=None),
            # the persistent kernel in the form the library picks, with all state in global memory, and with slot maps +
            # link statistics + per-core sums resident in LDS (a form only liborlgpu_alt.so carries; where it does not fit
            # the library's default form runs) and the per-row cache of inner free runs switched on (the library uses it only
            # where it costs no wavefront per CU)
            "persist": dict(ORL_STEP_IMPL="2", ORL_PERSIST="1", ORL_LIB_VARIANT="default", ORL_PERSIST_VARIANT=None, ORL_PERSIST_INNER=None),
            "persist_global": dict(ORL_STEP_IMPL="2", ORL_PERSIST="1", ORL_LIB_VARIANT="default", ORL_PERSIST_VARIANT="0", ORL_PERSIST_INNER=None),
            "persist_lds": dict(ORL_STEP_IMPL="2", ORL_PERSIST="1", ORL_LIB_VARIANT="alt", ORL_PERSIST_VARIANT="2", ORL_PERSIST_INNER="2"),
            # host- / agent-driven steps through k_agent (the phases of the persistent kernel for one step, with info) whatever
            # the batch size — the library takes it from 2 048 envs — for all four families (RMSA, DeepRMSA, RWA, RMCSA: every
            # g* / w* / h* fixture of theirs replays through it); device-resident runs as "persist"
            "agent8": dict(ORL_STEP_IMPL="2", ORL_PERSIST="1", ORL_LIB_VARIANT="default", ORL_PERSIST_VARIANT=None, ORL_PERSIST_INNER=None,
                           ORL_AGENT_STEP="1"),
            # the two-wavefront form of the persistent kernel (a control and a row wavefront per 8 envs; the library takes it for
            # batches of at most 12 288 envs of the single-core families) at every batch size: it exists in specialisation libraries
            # only, so one is built for every configuration (RMCSA: the one-wavefront kernel, specialised)
            "persist_pair": dict(ORL_STEP_IMPL="2", ORL_PERSIST="1", ORL_LIB_VARIANT="default", ORL_PERSIST_VARIANT="4", ORL_PERSIST_INNER=None,
                                 ORL_PERSIST_RW="1", ORL_JIT_SPEC="1"),
            # the rows-deferred form (round 6): the loop is slot scan + control phase, which changes the slot maps itself and logs an
            # event per provision / release; k_rowstats replays link statistics and compactness sums after every launch, one lane per
            # link row (single-core families with at most 64 links; elsewhere the library's own choice runs)
            "persist_rd": dict(ORL_STEP_IMPL="2", ORL_PERSIST="1", ORL_LIB_VARIANT="default", ORL_PERSIST_VARIANT="7", ORL_PERSIST_INNER=None,
                               ORL_PERSIST_RW="0")}
for _name, _env in IMPL_ENV.items():
    _env.setdefault("ORL_AGENT_STEP", None)
    _env.setdefault("ORL_PERSIST_RW", None)
    _env.setdefault("ORL_JIT_SPEC", None)


def force_impl(monkeypatch, name):
    for k, v in IMPL_ENV[name].items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _ran_pair_form(env):
    """The last device-resident run of `env` was launches of the two-wavefront kernel (debug query: 2)."""
    return int(env.lib.orl_batch_debug_persist_spec(env._h)) == 2


def _exact(name):
    def check(t, what, got, exp):
        got, exp = np.asarray(got), np.asarray(exp)
        if got.dtype.kind == "f" or exp.dtype.kind == "f":
            ok = np.array_equal(got.astype(np.float64), exp.astype(np.float64), equal_nan=True)
        else:
            ok = np.array_equal(got, exp)
        assert ok, "%s: step %d: %s differs\n got %r\n exp %r" % (name, t, what, got, exp)
    return check


def _exact_bits(name):
    """_exact with floats compared as their uint64 bit patterns: -0.0 differs from 0.0, a nan equals the nan of the same bits"""
    def check(t, what, got, exp):
        got, exp = np.asarray(got), np.asarray(exp)
        if got.dtype.kind == "f" or exp.dtype.kind == "f":
            got = np.ascontiguousarray(got, np.float64).view(np.uint64)
            exp = np.ascontiguousarray(exp, np.float64).view(np.uint64)
        ok = np.array_equal(got, exp)
        assert ok, "%s: step %d: %s differs (floats as bit patterns)\n got %r\n exp %r" % (name, t, what, got, exp)
    return check


# ---- the set_load fixtures (tests/golden/s1_*.npz): shared by tests/test_set_load_gpu.py (device) and tests/test_timescale.py (oracle)
S1 = {"RMSA": "s1_rmsa_set_load", "DeepRMSA": "s1_deeprmsa_set_load", "RWA": "s1_rwa_set_load", "RMCSA": "s1_rmcsa_set_load",
      "QoSConstrainedRA": "s1_qos_set_load"}


def _schedule(g):
    return {int(k): v for k, v in json.loads(str(g["schedule"])).items()}


def _replay_with_schedule(env, g, check, set_load=None):
    """tests.helpers.replay / replay_q with env.set_load(**schedule[t]) before the action of step t is decided (where the
    fixture's policy closure called the reference's set_load)."""
    meta, sched = g["meta"], _schedule(g)
    qos = meta["env"] == "QoSConstrainedRA"
    set_load = set_load or (lambda **ch: env.set_load(**ch))
    for t in range(meta["n_steps"]):
        if g["reset_before"][t]:
            env.reset(full=False)
        check(t, "svc", env.services()[0], g["svc"][t])
        if "obs" in g:
            check(t, "obs", env.observation()[0], g["obs"][t])
        if t in sched:
            set_load(**sched[t])
            check(t, "svc after set_load", env.services()[0], g["svc"][t])
        a = env.policy(meta["policy"])
        width = g["actions"].shape[1]
        check(t, "action", np.asarray(a[0, :width], np.int64), g["actions"][t])
        _, reward, done, info = env.step(a)
        check(t, "reward", reward[0], g["reward"][t])
        check(t, "done", int(done[0]), int(g["done"][t]))
        check(t, "info", info[0, : g["info"].shape[1]], g["info"][t])
        check(t, "n_active", env.n_active(0), int(g["n_active"][t]))
        if qos:
            check(t, "counters", env.counters()[0, :4], g["counters"][t][:4])
            check(t, "spectrum", env.spectrum(0), g["spectrum"][t])
        else:
            check(t, "counters", env.counters()[0], g["counters"][t])
            sl = env.slots(0)
            sl = sl[0] if sl.shape[0] == 1 else sl
            check(t, "crc", crc_slots(sl), int(g["crc"][t]))
        if (t + 1) in meta["snapshot_steps"]:
            ls = env.link_stats(0)
            ref = g["snap%d_link_stats" % (t + 1)]
            if qos:
                check(t, "utilization", ls[0], ref[0])
                check(t, "last_update", ls[3], ref[3])
            else:
                check(t, "snap_slots", np.packbits(sl, axis=-1, bitorder="little"), g["snap%d_slots" % (t + 1)])
                check(t, "snap_link_stats", ls, ref)
                check(t, "snap_net_stats", env.net_stats(0), g["snap%d_net_stats" % (t + 1)])
    check(meta["n_steps"], "svc", env.services()[0], g["svc"][meta["n_steps"]])


# ---- full, masked and soft resets between runs (tests/test_gpu_parity.py in the library's own form, tests/test_run_plans_gpu.py in
# every form of the persistent kernel with the batch in two halves)
def resets_between_runs(dev, ora, policy, masks, chk, sample, after_run=None):
    """reset(only_episode_counters=False) after stepping, for all envs and for a mask of envs, and masked soft resets
    (rmsa_env.py:284-359, rwa_env.py:164-208, rmcsa_env.py:386-483): full masked reset (masks[0]) after a run, run, host steps, full
    reset, run, soft masked reset (masks[1]), run — the batch keeps equal to the oracle.  Counters, pending service and pending
    releases of every env; slot maps and statistics of the envs in `sample`.  after_run() is called after every device-resident run."""
    n = dev.num_envs

    def compare(tag):
        chk(tag, "counters", dev.counters(), ora.counters())
        chk(tag, "services", dev.services(), ora.services())
        chk(tag, "active", dev.active(), np.array([ora.n_active(i) for i in range(n)]))
        for e in sample:
            chk(tag, "slots", dev.slots(e), ora.slots(e))
            chk(tag, "link_stats", dev.link_stats(e), ora.link_stats(e))
            chk(tag, "net_stats", dev.net_stats(e), ora.net_stats(e))
        if dev.obs_dim:
            chk(tag, "obs", dev.observation(), ora.observation())

    def run(steps):
        dev.run(policy, steps); ora.run(policy, steps)
        if after_run is not None:
            after_run(steps)

    run(130)
    dev.reset(full=True, mask=masks[0]); ora.reset(full=True, mask=masks[0])
    compare(1)
    run(90)
    compare(2)
    for t in range(40):  # host-driven steps after a masked full reset
        a_o, a_d = ora.policy(policy), dev.policy(policy)
        chk(t, "actions", a_d, a_o)
        _, r_o, d_o, i_o = ora.step(a_o, auto_reset=True)
        _, r_d, d_d, i_d = dev.step(a_d, auto_reset=True)
        chk(t, "reward", r_d, r_o); chk(t, "done", d_d, d_o); chk(t, "info", i_d, i_o)
    dev.reset(full=True); ora.reset(full=True)
    compare(3)
    run(70)
    dev.reset(full=False, mask=masks[1]); ora.reset(full=False, mask=masks[1])
    compare(4)
    run(60)
    compare(5)
    assert not dev.flags().any()
