"""The accepted configuration range, without a GPU (tests/envelope.py holds the table): the topology builder against tables
recorded from the reference's own builder at k = 9, k = 64, one path per pair and 30 hops; the oracle against reference traces
there (e* fixtures, oracle/gen_golden_envelope.py); the conditions that keep a GPU case from passing by doing nothing (C1:
provisioning AND blocking, episode boundaries, releases; C2: the branch the case exists for is taken), judged on the oracle's own
run; which side of the persistent kernel's limits each case is on, as the library itself answers without a device, with a
specialisation library cross-compiled for every served case; and the refusals of orl_topology_create."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from tests import envelope
from tests.helpers import GOLDEN, ROOT, golden_names, load_golden, replay

HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not HAVE_HIPCC, reason="needs hipcc")

TOPO_FIELDS = ("link_nodes", "link_length", "edge_iter_order", "n_paths", "path_hops", "path_links", "path_nodes", "path_length",
               "path_id", "path_best_mod")


@pytest.fixture(scope="module")
def topo_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("envelope_topologies")


def _exact(name):
    def check(t, what, got, exp):
        got, exp = np.asarray(got), np.asarray(exp)
        if got.dtype.kind == "f" or exp.dtype.kind == "f":
            ok = np.array_equal(got.astype(np.float64), exp.astype(np.float64), equal_nan=True)
        else:
            ok = np.array_equal(got, exp)
        assert ok, "%s: step %d: %s differs\n got %r\n exp %r" % (name, t, what, got, exp)
    return check


# ---- topologies ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", envelope.GOLDEN_TOPOLOGIES)
def test_build_topology_equals_the_reference_builder(name, k, topo_dir):
    """topology_io.build_topology on the raw file == the tables flattened from the reference's get_topology on the same file,
    field for field: k != 5, n_paths < k (star129: one path per pair), max_hops = 30 (ring31)."""
    built = envelope.topology_of(envelope.topology_npz(name, k, topo_dir))
    ref = envelope.topology_of(os.path.join(GOLDEN, "topo_%s_k%d.npz" % (name, k)))
    assert built.node_names == ref.node_names and built.k_paths == ref.k_paths == k and built.link_ids == ref.link_ids
    for f in TOPO_FIELDS:
        a, b = getattr(built, f), getattr(ref, f)
        assert a.shape == b.shape and np.array_equal(a, b), f
    assert [(m.name, m.maximum_length, m.spectral_efficiency) for m in built.modulations] == \
        [(m.name, m.maximum_length, m.spectral_efficiency) for m in ref.modulations]


def test_the_synthetic_topologies_sit_on_the_limits(topo_dir):
    shape = {}
    for name, k in (("ring10c8", 8), ("ring10c8", 9), ("ring10c8", 16), ("k6full", 64), ("star65", 5), ("star66", 5), ("star129", 5),
                    ("ring31", 2), ("ring32", 2)):
        t = envelope.topology_of(envelope.topology_npz(name, k, topo_dir))
        shape[(name, k)] = (t.n_nodes, t.n_links, t.max_hops, int(t.n_paths.max()))
    assert shape[("ring10c8", 16)][3] == 16 and shape[("k6full", 64)] == (6, 15, 5, 64)
    assert shape[("star65", 5)] == (65, 64, 2, 1) and shape[("star66", 5)] == (66, 65, 2, 1) and shape[("star129", 5)] == (129, 128, 2, 1)
    assert shape[("ring31", 2)] == (31, 31, 30, 2) and shape[("ring32", 2)] == (32, 32, 31, 2)
    hops = envelope.topology_of(envelope.topology_npz("ring31", 2, topo_dir)).path_hops
    assert (hops == 30).any() and (hops == 29).any()


def test_every_boundary_has_both_sides_in_the_table():
    sides = {}
    for c in envelope.CASES:
        sides.setdefault(c.boundary, set()).add(c.side)
    for boundary, have in sides.items():
        # "at": the accepted extreme itself, whose far side is a refusal
        assert have >= {"near", "far"} or have == {"at"}, (boundary, have)
    assert {c.served for c in envelope.CASES} == {True, False}


# ---- the oracle at the envelope -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("e"))
def test_oracle_reproduces_reference_trace_at_the_envelope(name):
    from oracle.oracle import OracleBatch

    g = load_golden(name)
    kw = dict(g["meta"]["kwargs"])
    seed = kw.pop("seed")
    env = OracleBatch(g["meta"]["env"], os.path.join(GOLDEN, g["meta"]["topology"]), [seed], **kw)
    replay(env, g, _exact(name))


def test_the_envelope_fixtures_take_the_branches_they_were_recorded_for():
    names = golden_names("e")
    assert len(names) == 10
    for name in names:
        g = load_golden(name)
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= os.path.getsize(os.path.join(GOLDEN, "g5_rwa_testcfg_sapff.npz"))
        acc = np.diff(np.concatenate([[0], g["counters"][:, 1]])) == 1
        assert 0.1 < acc.mean() < 0.95, name
        if "_k9_" in name or "_k64_" in name:  # (DeepRMSA: action = path * j + block)
            j = g["meta"]["kwargs"].get("j", 1)
            assert (g["actions"][acc, 0] // j >= 8).any(), name
        if "star129" in name:
            assert (g["svc"][:, 2] >= 64).any() and (g["svc"][:, 2] == 128).any() and (g["svc"][:, 3] == 128).any(), name
        if "ring31_sapff" in name:
            t = envelope.topology_of(os.path.join(GOLDEN, g["meta"]["topology"]))
            src, dst = g["svc"][:-1, 2].astype(int), g["svc"][:-1, 3].astype(int)
            p = np.minimum(g["actions"][:, 0], 1)
            assert (acc & (g["actions"][:, 0] < 2) & (t.path_hops[src, dst, p] == 30)).any(), name


@pytest.mark.parametrize("case,policy", envelope.policy_and_case_ids(), ids=lambda v: v if isinstance(v, str) else v.name)
def test_conditions_c1_c2_hold_on_the_oracle(case, policy, topo_dir):
    path = envelope.topology_npz(case.topo, case.k, topo_dir)
    w = envelope.oracle_walk(case, policy, path)
    envelope.check_c1(case, w)
    envelope.check_c2(case, w, envelope.topology_of(path))


def test_condition_c3_the_high_occupancy_run_fills_the_last_64_release_slots(topo_dir):
    """rmcsa_hiocc: over every step a GPU test runs it for, the oracle's pending releases peak above 1984 in at least one env and
    never above the 2048 the batch is created with in any — so the upper bits of the 8 + 3-bit release index are in use and no env
    overflows."""
    from oracle.oracle import OracleBatch

    case = envelope.CASE_BY_NAME["rmcsa_hiocc"]
    assert case.kw["event_capacity"] == 2048 and case.served
    ora = OracleBatch(case.fam, case.topo, envelope.seeds_of(case), **envelope.oracle_kwargs(case))
    peak = np.zeros(case.batch, np.int64)
    at_handover = None
    for t in range(case.warm + case.steps + envelope.EXTRA_STEPS):
        ora.run(case.policies[0], 1)
        peak = np.maximum(peak, ora.active())
        if t + 1 == case.warm:
            at_handover = ora.active().copy()
    print("rmcsa_hiocc: pending releases after the warm-up %s, peak %s" % (at_handover, peak))
    assert peak.max() > 1984 and peak.max() <= 2048, peak
    assert at_handover.max() > 1984, at_handover


# ---- dispatch, without a device ---------------------------------------------------------------------------------------------
def _derived(case, topo_dir):
    from optical_rl_gym_amd import envs

    topo = envelope.topology_npz(case.topo, case.k, topo_dir)
    return envs.ENV_CLASSES[case.fam]._derived(topology=topo, **case.kw)


@pytest.mark.parametrize("case", envelope.CASES, ids=lambda c: c.name)
def test_the_library_serves_exactly_the_near_side(case, topo_dir, monkeypatch):
    """orl_spec_flags_for_batch / orl_debug_persist_choice answer "served" for k <= 8, capacity <= 2048, widest service <= 63
    slots — and for nothing beyond.  star65 (64 links) may take the rows-deferred form 7, star66 (65 links) may not."""
    for v in ("ORL_PERSIST_VARIANT", "ORL_PERSIST_RW", "ORL_PERSIST_INNER", "ORL_PERSIST_EVL", "ORL_PERSIST_WGS_PER_CU", "ORL_PERSIST_SPEC"):
        monkeypatch.delenv(v, raising=False)
    cfg = _derived(case, topo_dir)
    buf = C.create_string_buffer(1024)
    for batch in (case.batch, 4096, 1 << 20):
        n = cfg.lib.orl_spec_flags_for_batch(C.byref(cfg._cfg), C.byref(cfg._desc), batch, buf, len(buf))
        choice = cfg.persist_choice(batch)
        assert (n > 0) == case.served and (choice is not None) == case.served, (case.name, batch, n, choice)
    if case.served and case.fam != "RMCSA" and case.topo in ("star65", "star66"):
        monkeypatch.setenv("ORL_PERSIST_VARIANT", "7")
        monkeypatch.setenv("ORL_PERSIST_RW", "0")
        form = cfg.persist_choice(case.batch)[0]
        assert (form == 7) == (case.topo == "star65"), (case.name, form)


# k_persist (the kernels tests/test_kernel_regs.py inspects) of an envelope specialisation that needs scratch memory: {case: (spilled VGPRs, private segment bytes)}, as
# tools/kernel_regs.py reports them at this commit.  Recorded, not targets (tests/test_kernel_regs.py demands 0 / 0 of the
# BASELINE specialisations); every case not listed here needs none.
MEASURED_SCRATCH = {}


@needs_hipcc
@pytest.mark.parametrize("case", [c for c in envelope.CASES if c.served], ids=lambda c: c.name)
def test_a_specialisation_builds_for_every_served_case(case, topo_dir):
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs
    from optical_rl_gym_amd import _build

    cfg = _derived(case, topo_dir)
    buf = C.create_string_buffer(1024)
    assert cfg.lib.orl_spec_flags_for_batch(C.byref(cfg._cfg), C.byref(cfg._desc), case.batch, buf, len(buf)) > 0
    lib = _build.build_spec(buf.value.decode())
    ks = [k for k in kernel_regs.kernels(lib) if "k_persist" in kernel_regs.demangle(k["name"])]
    assert ks, "%s: no k_persist in %s" % (case.name, lib)
    got = (max(int(k["vgpr_spill_count"]) for k in ks), max(int(k["private_segment_fixed_size"]) for k in ks))
    print("%s: %d k_persist kernel(s), %d spilled VGPRs, %d B of scratch" % (case.name, len(ks), got[0], got[1]))
    assert got == MEASURED_SCRATCH.get(case.name, (0, 0)), (case.name, got)


# ---- refusals of orl_topology_create (validation precedes the first HIP call) -------------------------------------------------
def _desc(t, **over):
    """(TopologyDesc, arrays kept alive) of topology `t` with fields or tables replaced."""
    from optical_rl_gym_amd import _lib

    keep = dict(n_paths=np.ascontiguousarray(t.n_paths, np.int32), path_hops=np.ascontiguousarray(t.path_hops, np.int32),
                path_links=np.ascontiguousarray(t.path_links, np.int32), path_length=np.ascontiguousarray(t.path_length, np.float64),
                path_mod=np.ascontiguousarray(t.path_best_mod, np.int32), edge_iter_order=np.ascontiguousarray(t.edge_iter_order, np.int32))
    scal = dict(n_nodes=t.n_nodes, n_links=t.n_links, k_paths=t.k_paths, max_hops=t.max_hops, n_modulations=len(t.modulations))
    for k, v in over.items():
        if k in scal:
            scal[k] = v
        else:
            keep[k] = v
    d = _lib.TopologyDesc(scal["n_nodes"], scal["n_links"], scal["k_paths"], scal["max_hops"], scal["n_modulations"],
                          *[keep[n].ctypes.data for n in ("n_paths", "path_hops", "path_links", "path_length", "path_mod", "edge_iter_order")])
    return d, keep


RANGE = b"topology out of supported range (N<=512, E<=128, k<=64, hops<=30)"


def test_topology_refusals(topo_dir):
    from optical_rl_gym_amd import _lib

    lib = _lib.lib()
    t = envelope.topology_of(envelope.topology_npz("ring10c8", 9, topo_dir))
    ring32 = envelope.topology_of(envelope.topology_npz("ring32", 2, topo_dir))
    assert ring32.max_hops == 31
    bad_link = np.ascontiguousarray(t.path_links, np.int32).copy()
    bad_link[0, 1, 0, 0] = t.n_links
    many = np.ascontiguousarray(t.n_paths, np.int32).copy()
    many[0, 1] = t.k_paths + 1
    twice = np.ascontiguousarray(t.edge_iter_order, np.int32).copy()
    twice[1] = twice[0]
    beyond = np.ascontiguousarray(t.edge_iter_order, np.int32).copy()
    beyond[2] = t.n_links
    refusals = [("N = 1", t, dict(n_nodes=1), RANGE), ("N = 513", t, dict(n_nodes=513), RANGE),
                ("E = 0", t, dict(n_links=0), RANGE), ("E = 129", t, dict(n_links=129), RANGE),
                ("k = 0", t, dict(k_paths=0), RANGE), ("k = 65", t, dict(k_paths=65), RANGE),
                ("H = 0", t, dict(max_hops=0), RANGE), ("H = 31", ring32, {}, RANGE),
                ("link index >= E", t, dict(path_links=bad_link), b"bad link index %d at hop 0" % t.n_links),
                ("n_paths > k", t, dict(n_paths=many), b"n_paths[1] out of range"),
                ("edge_iter_order with a link twice", t, dict(edge_iter_order=twice), b"edge_iter_order is not a permutation"),
                ("edge_iter_order beyond E", t, dict(edge_iter_order=beyond), b"edge_iter_order is not a permutation")]
    good, good_keep = _desc(t)
    for what, topo, over, message in refusals:
        d, keep = _desc(topo, **over)
        h = C.c_void_p()
        rc = lib.orl_topology_create(C.byref(d), 0, C.byref(h))
        assert rc == -1 and not h.value, what  # ORL_E_INVALID
        assert message in lib.orl_last_error(), (what, lib.orl_last_error())
        # ... and the next valid call is not affected: ORL_OK where a device exists, the HIP error without one — never "invalid"
        rc = lib.orl_topology_create(C.byref(good), 0, C.byref(h))
        assert rc in (0, -2), (what, rc, lib.orl_last_error())
        if rc == 0:
            lib.orl_topology_destroy(h)
    assert lib.orl_topology_create(None, 0, None) == -1
