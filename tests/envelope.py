"""The envelope table: configurations at the edges of what orl_topology_create / batch_create_impl accept (include/orl.h),
each naming the limit or dispatch boundary it sits on and the side — shared by tests/test_envelope.py (CPU: topology tables,
fixtures, the oracle's own conditions, the dispatch without a device) and tests/test_envelope_gpu.py (every case on every env
against the oracle).  Helper module, no tests.

Synthetic topologies are written in the raw `.txt` format of topology_io.read_txt (nodes, links, "a b length" per link) and
built with topology_io.build_topology into a directory the caller names (a session's temporary directory); builds are cached
by (raw text, k).  `served`: the persistent kernel serves the device-resident loop (k <= 8, event capacity <= 2048, widest
service <= 63 slots); the far side of those runs k_step / k_policy<.., 64>."""
import os
from collections import namedtuple

import numpy as np


# ---- raw topologies -----------------------------------------------------------------------------------------------------
def _raw(n_nodes, links, title):
    return "# %s\n%d\n%d\n%s\n" % (title, n_nodes, len(links), "\n".join("%d %d %d" % l for l in links))


def _ring(n, length):
    return [(i + 1, (i + 1) % n + 1, length(i)) for i in range(n)]


def _star(leaves):
    # hub = node 1; leaf lengths 40 .. ~1600 km: two-hop paths of 80 .. 3200 km, every modulation but the shortest-reach one
    return [(1, 2 + i, 40 + (i * 37) % 1571) for i in range(leaves)]


def raw_text(name):
    if name == "ring10c8":  # 10-node ring with 8 chords: 18 links, dozens of simple paths per pair
        links = _ring(10, lambda i: 120 + 70 * i) + [(1 + c, 1 + (c + 2 + c % 3) % 10, 260 + 90 * c) for c in range(8)]
        return _raw(10, links, name)
    if name == "k6full":  # complete graph on 6 nodes: 15 links, 65 simple paths per pair
        links = [(a, b, 150 + 110 * ((3 * a + 5 * b) % 7)) for a in range(1, 7) for b in range(a + 1, 7)]
        return _raw(6, links, name)
    if name.startswith("star"):  # a hub and N - 1 leaves: N - 1 links, one tree path per pair
        n = int(name[4:])
        return _raw(n, _star(n - 1), name)
    if name.startswith("ring"):  # plain ring: the two paths of a pair have h and N - h hops; k = 2 gives max_hops = N - 1
        n = int(name[4:])
        return _raw(n, _ring(n, lambda i: 60 + 45 * (i % 5)), name)
    raise KeyError(name)


SHIPPED = ("nsfnet_chen", "cost239", "germany50")
# (name, k) of the synthetic topologies whose tables are committed as tests/golden/topo_<name>_k<k>.npz, recorded from the
# reference's own topology builder (oracle/gen_golden_envelope.py)
GOLDEN_TOPOLOGIES = (("ring10c8", 9), ("k6full", 64), ("star129", 5), ("ring31", 2))

_BUILT = {}


def topology_npz(name, k, directory):
    """Path of the flattened tables of topology `name` at `k` paths: a shipped topology's name as it is, a synthetic one
    built (once per raw text and k) into `directory`."""
    if name in SHIPPED:
        assert k == 5
        return name
    text = raw_text(name)
    if (text, k) not in _BUILT:
        from optical_rl_gym_amd.topology_io import build_topology, save_topology

        raw = os.path.join(str(directory), "%s.txt" % name)
        with open(raw, "w") as f:
            f.write(text)
        out = os.path.join(str(directory), "%s_k%d.npz" % (name, k))
        save_topology(build_topology(raw, name=name.upper(), k_paths=k), out)
        _BUILT[(text, k)] = out
    return _BUILT[(text, k)]


def topology_of(path_or_name):
    from optical_rl_gym_amd.topology import Topology

    return Topology.load(path_or_name)


# ---- the table ----------------------------------------------------------------------------------------------------------
# name: the test id.  boundary / side: the limit the case exists for ("near" = the side the suite's other tests are on or the
# persistent kernel serves, "far" = the other, "at" = the accepted extreme itself).  policies: heuristics compared.  served: see above.
# c2: the branch conditions the oracle's run must show (tests/test_envelope.py, C2).  batch / warm / steps: sizes of the oracle
# comparison (envs, steps of run() in front, host-driven steps).
Case = namedtuple("Case", "name fam topo k kw policies boundary side served c2 batch warm steps")


def _c(name, fam, topo, k, kw, policies, boundary, side, served, c2=(), batch=64, warm=400, steps=75):
    """warm: steps of the device-resident loop (run()) in front of the host-driven ones — an env holds no more services than it
    has accepted, so a network only blocks after about as many steps as its load in Erlang."""
    kw = dict(kw)
    kw.setdefault("episode_length", 25)
    kw.setdefault("mean_service_holding_time", 10.0)
    return Case(name, fam, topo, k, kw, tuple(policies), boundary, side, served, tuple(c2), batch, warm, steps)


def _deep(load, S=64, j=8, **kw):
    return dict(kw, mean_service_holding_time=10.0, mean_service_inter_arrival_time=10.0 / load, j=j, num_spectrum_resources=S)


_RING10 = dict(load=160, num_spectrum_resources=70)
_QOS = dict(load=100, num_spectrum_resources=12, num_service_classes=2, classes_arrival_probabilities=[0.5, 0.5], classes_reward=[2.0, 1.0])
_WXT = dict(worst_xt=-84.7, allow_rejection=True)
# ring31: most requests between two neighbours, so that their direct link fills up and the 30-hop way round is taken
_RING31_PROBS = [0.3, 0.3] + [0.4 / 29] * 29
_W63 = dict(load=250, num_spectrum_resources=512, allow_rejection=True, bit_rate_selection="discrete", bit_rate_probabilities=(0.5, 0.5))

CASES = [
    # --- K <= 8: persistent kernel, k_agent, one-launch policy_step, k_obs8 | k_policy<ENV, W, 64>, k_obs, k_step --------
    _c("ring10c8_k8_rmsa", "RMSA", "ring10c8", 8, dict(_RING10, allow_rejection=True), ("SAP_FF", "LLP_FF"), "K <= 8", "near", True),
    _c("ring10c8_k9_rmsa", "RMSA", "ring10c8", 9, dict(_RING10, allow_rejection=True), ("SAP_FF", "LLP_FF"), "K <= 8", "far", False,
       ("path_ge_8",)),
    _c("ring10c8_k16_rmsa", "RMSA", "ring10c8", 16, _RING10, ("SAP_FF", "LLP_FF"), "K <= 8", "far", False, ("path_ge_8",)),
    _c("ring10c8_k9_rwa", "RWA", "ring10c8", 9, dict(load=170, num_spectrum_resources=16), ("SAP_LF", "LLP_FF"), "K <= 8", "far", False,
       ("path_ge_8",)),
    _c("ring10c8_k8_deep_j8", "DeepRMSA", "ring10c8", 8, _deep(140), ("SAP",), "K == 8 && J == 8 (k_obs8)", "near", True),
    _c("ring10c8_k8_deep_j8_rej", "DeepRMSA", "ring10c8", 8, _deep(140, allow_rejection=True), ("SAP",), "K == 8 && J == 8 (k_obs8)",
       "near", True),
    _c("ring10c8_k9_deep_j8", "DeepRMSA", "ring10c8", 9, _deep(140), ("SAP",), "K == 8 && J == 8 (k_obs8)", "far", False, ("path_ge_8",)),
    _c("ring10c8_k9_deep_j8_rej", "DeepRMSA", "ring10c8", 9, _deep(140, allow_rejection=True), ("SAP",), "K == 8 && J == 8 (k_obs8)",
       "far", False, ("path_ge_8",)),
    _c("ring10c8_k8_qos", "QoSConstrainedRA", "ring10c8", 8, _QOS, ("SAP_FF", "LLP_FF"), "K <= 8 (k_agent_qos)", "near", False),
    _c("ring10c8_k9_qos", "QoSConstrainedRA", "ring10c8", 9, _QOS, ("SAP_FF", "LLP_FF"), "K <= 8 (k_agent_qos)", "far", False,
       ("path_ge_8",)),
    # --- k = 64: the accepted maximum --------------------------------------------------------------------------------------
    _c("k6full_k64_rmsa", "RMSA", "k6full", 64, dict(load=200, num_spectrum_resources=24, allow_rejection=True), ("SAP_FF", "LLP_FF"),
       "k_paths <= 64", "at", False, ("path_ge_8",), warm=600),
    _c("k6full_k64_deep_j8", "DeepRMSA", "k6full", 64, _deep(200, S=24), ("SAP",), "k_paths <= 64", "at", False, ("path_ge_8",), warm=600),
    _c("k6full_k64_rwa", "RWA", "k6full", 64, dict(load=150, num_spectrum_resources=8), ("SAP_FF", "LLP_FF"), "k_paths <= 64", "at",
       False, ("path_ge_8",)),
    # --- N > 64 (rng_choice in rounds), E <= 64 (rows-deferred forms, one round of the link-row loops), n_paths < k --------
    _c("star65_rmsa", "RMSA", "star65", 5, dict(load=250, num_spectrum_resources=24, allow_rejection=True), ("SAP_FF", "LLP_FF"),
       "E <= 64 / N > 64", "near", True, ("missing_paths", "src_ge_64"), warm=600),
    _c("star65_rwa", "RWA", "star65", 5, dict(load=130, num_spectrum_resources=4), ("SAP_FF",), "E <= 64 / N > 64", "near", True,
       ("missing_paths", "src_ge_64")),
    _c("star66_rmsa", "RMSA", "star66", 5, dict(load=250, num_spectrum_resources=24, allow_rejection=True), ("SAP_FF", "LLP_FF"),
       "E <= 64 / N > 64", "far", True, ("missing_paths", "src_ge_64"), warm=600),
    _c("star66_rwa", "RWA", "star66", 5, dict(load=130, num_spectrum_resources=4), ("SAP_FF",), "E <= 64 / N > 64", "far", True,
       ("missing_paths", "src_ge_64")),
    _c("star129_rmsa", "RMSA", "star129", 5, dict(load=400, num_spectrum_resources=24, allow_rejection=True), ("SAP_FF", "LLP_FF"),
       "E <= 128", "at", True, ("missing_paths", "src_ge_64", "src_eq_128"), batch=32, warm=900),
    _c("star129_deep", "DeepRMSA", "star129", 5, _deep(400, S=24, j=2), ("SAP",), "E <= 128", "at", True,
       ("missing_paths", "src_ge_64", "src_eq_128"), warm=900),
    _c("star129_rwa", "RWA", "star129", 5, dict(load=260, num_spectrum_resources=4), ("SAP_LF",), "E <= 128", "at", True,
       ("missing_paths", "src_ge_64", "src_eq_128"), warm=600),
    # --- H = 30: the path record filled to its last byte -------------------------------------------------------------------
    _c("ring31_rmsa", "RMSA", "ring31", 2, dict(load=40, num_spectrum_resources=70, allow_rejection=True,
                                                node_request_probabilities=_RING31_PROBS),
       ("SAP_FF", "LLP_FF"), "max_hops <= 30", "at", True, ("hops_30", "hops_odd")),
    _c("ring31_deep", "DeepRMSA", "ring31", 2, _deep(40, j=3, node_request_probabilities=_RING31_PROBS), ("SAP",), "max_hops <= 30",
       "at", True, ("hops_30", "hops_odd")),
    _c("ring31_rwa", "RWA", "ring31", 2, dict(load=48, num_spectrum_resources=16, node_request_probabilities=_RING31_PROBS),
       ("SAP_FF", "LLP_FF"), "max_hops <= 30", "at", True, ("hops_30", "hops_odd")),
    # --- slots ---------------------------------------------------------------------------------------------------------------
    # (RMSA's first fit searches range(0, S - n): a service as wide as the spectrum never fits, so S = 2 is an RWA case)
    _c("s2_rwa", "RWA", "nsfnet_chen", 5, dict(load=8, num_spectrum_resources=2), ("SAP_FF", "SAP_LF"), "S >= 2", "at", True, warm=100),
    _c("s512_w63_rmsa", "RMSA", "nsfnet_chen", 5, dict(_W63, bit_rates=(100, 775)),  # 775 Gb/s on BPSK: 62 + 1 slots
       ("SAP_FF", "LLP_FF"), "S <= 512 / widest service <= 63", "near", True, ("width_63", "slot_ge_256"), batch=24, warm=800),
    _c("s512_w64_rmsa", "RMSA", "nsfnet_chen", 5, dict(_W63, bit_rates=(100, 780)),  # 780 Gb/s on BPSK: 63 + 1 slots
       ("SAP_FF",), "S <= 512 / widest service <= 63", "far", False, ("width_64", "slot_ge_256"), batch=24, warm=800),
    _c("one_rate_rmsa", "RMSA", "nsfnet_chen", 5, dict(load=200, num_spectrum_resources=64, allow_rejection=True,
                                                       bit_rate_selection="discrete", bit_rates=(40,)),
       ("SAP_FF", "LLP_FF"), "n_bit_rates >= 1", "at", True, ("single_rate",), warm=600),
    # --- cores: 4 C against the 16-word lines of cs_words --------------------------------------------------------------------
    _c("rmcsa_c1", "RMCSA", "nsfnet_chen", 5, dict(_WXT, load=60, num_spectrum_resources=64, num_spatial_resources=1),
       ("SAP_BM_FC_FF",), "C >= 1", "at", True, ("core_last",)),
    _c("rmcsa_c16", "RMCSA", "nsfnet_chen", 5, dict(_WXT, load=600, num_spectrum_resources=12, num_spatial_resources=16),
       ("SAP_BM_FC_FF",), "4 C <= 64 (cs_words)", "near", True, ("core_last",), warm=1500),
    _c("rmcsa_c17", "RMCSA", "nsfnet_chen", 5, dict(_WXT, load=600, num_spectrum_resources=12, num_spatial_resources=17),
       ("SAP_BM_FC_FF",), "4 C <= 64 (cs_words)", "far", True, ("core_last",), warm=1500),
    _c("rmcsa_c31", "RMCSA", "nsfnet_chen", 5, dict(_WXT, load=1100, num_spectrum_resources=12, num_spatial_resources=31),
       ("SAP_BM_FC_FF",), "C <= 31", "at", True, ("core_last",), warm=2500),
    # (31 cores x 512 slots on COST239's 26 links: a per-env window of 53 136 B, the largest RMCSA one under the 64 KiB limit that
    # a shipped topology gives; Germany50's 88 links give 174 KiB and are refused)
    _c("rmcsa_c31_s512", "RMCSA", "cost239", 5, dict(_WXT, load=100, num_spectrum_resources=512, num_spatial_resources=31),
       ("SAP_BM_FC_FF",), "per-env LDS window <= 64 KiB", "at", True, batch=16, warm=300),
    # --- event capacity: release slots indexed with 8 + 3 bits ---------------------------------------------------------------
    _c("evcap_2048_rmsa", "RMSA", "nsfnet_chen", 5, dict(load=250, num_spectrum_resources=100, allow_rejection=True, event_capacity=2048),
       ("SAP_FF",), "event_capacity <= 2048", "near", True, warm=700),
    _c("evcap_2112_rmsa", "RMSA", "nsfnet_chen", 5, dict(load=250, num_spectrum_resources=100, allow_rejection=True, event_capacity=2112),
       ("SAP_FF",), "event_capacity <= 2048", "far", False, warm=700),
    # (condition C3: the warm-up ends while the pending releases of the fullest env stand in the last 64 of 2048 — the steady state of
    # this load, 0.8 x 2600, would overflow; the oracle's peak over the whole run is checked step by step in tests/test_envelope.py)
    _c("rmcsa_hiocc", "RMCSA", "cost239", 5, dict(_WXT, load=2600, mean_service_holding_time=25.0, num_spectrum_resources=320,
                                                  num_spatial_resources=7, event_capacity=2048),
       ("SAP_BM_FC_FF",), "event_capacity <= 2048 (upper bits of the release index)", "at", True, ("c3_peak",), batch=8, warm=7350),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# steps a GPU test runs a case for at most: warm-up, 4 timed steps (loops other than the persistent kernel), host-driven steps, 41 + 23
EXTRA_STEPS = 4 + 64


def oracle_kwargs(case):
    """The case's kwargs as OracleBatch takes them (event_capacity is a property of the product's arrays only)."""
    kw = dict(case.kw)
    kw.pop("event_capacity", None)
    return kw


def seeds_of(case):
    return [1000 + 13 * i + len(case.name) for i in range(case.batch)]


def policy_and_case_ids():
    return [(c, p) for c in CASES for p in c.policies]


# ---- the oracle's own run of a case: what conditions C1 / C2 are judged on ------------------------------------------------
def oracle_walk(case, policy, topo_path):
    """Oracle run of the case (run() for the warm-up, then policy(), step(auto_reset=True) host-driven) -> dict of per-step arrays [steps][batch]:
    svc (pending service before the step), actions, accepted (the step provisioned), plus final counters and active."""
    from oracle.oracle import OracleBatch

    ora = OracleBatch(case.fam, topo_path, seeds_of(case), **oracle_kwargs(case))
    ora.run(policy, case.warm)
    svc, acts, acc, dones, rel = [], [], [], [], []
    for _ in range(case.steps):
        svc.append(ora.services().copy())
        before, held = ora.counters()[:, 1].copy(), ora.active().copy()
        a = ora.policy(policy).copy()
        _, _, d, _ = ora.step(a, auto_reset=True)
        acts.append(a)
        acc.append(ora.counters()[:, 1] - before == 1)
        rel.append(held + acc[-1] - ora.active())
        dones.append(d.copy())
    return dict(svc=np.array(svc), actions=np.array(acts), accepted=np.array(acc), done=np.array(dones), released=np.array(rel),
                counters=ora.counters().copy(), active=ora.active().copy())


def check_c1(case, w):
    """C1, judged on the host-driven steps alone (the warm-up, which starts from an empty network and accepts nearly everything, does
    not count — the stricter reading): acceptance between 10 % and 95 % over all envs, >= 2 episode boundaries in every env, and
    >= 1 release in every env, counted step by step as pending releases before + provisioned - pending releases after."""
    processed, accepted = int(w["accepted"].size), int(w["accepted"].sum())
    assert 0.10 * processed <= accepted <= 0.95 * processed, "%s: %d of %d services accepted" % (case.name, accepted, processed)
    assert (w["done"].sum(axis=0) >= 2).all(), "%s: an env passed fewer than two episode boundaries" % case.name
    assert (w["released"] >= 0).all() and (w["released"].sum(axis=0) >= 1).all(), "%s: an env released nothing" % case.name


def check_c2(case, w, topo):
    """C2: the branch the case exists for is taken in the oracle's run."""
    svc, a, ok = w["svc"], w["actions"], w["accepted"]
    src, dst = svc[..., 2].astype(int), svc[..., 3].astype(int)
    deep = case.fam == "DeepRMSA"
    j = case.kw.get("j", 1)
    path = a[..., 0] // j if deep else a[..., 0]
    chosen = ok & (path < case.k)
    p = np.minimum(path, case.k - 1)
    hops = topo.path_hops[src, dst, p]
    for what in case.c2:
        if what == "path_ge_8":
            assert (chosen & (path >= 8)).any(), "%s: no service provisioned on a path index >= 8" % case.name
        elif what == "missing_paths":
            np_ = topo.n_paths[src, dst]
            # one path per pair, k = 5: the heuristics scan indices 0 .. k - 1, of which 1 .. 4 do not exist.  What is observed: every
            # provisioned service is on path 0, and every service not provisioned got the reject action (path index k) — a policy
            # that took a missing index for a path would have answered 1 .. 4 for some of the services whose path 0 was full
            assert (np_ == 1).all() and case.k == 5
            assert chosen.any() and (path[chosen] == 0).all()
            assert (~ok).any() and (path[~ok] == case.k).all()
        elif what == "src_ge_64":
            assert (src >= 64).any() and (dst >= 64).any()
        elif what == "src_eq_128":
            assert (src == 128).any() and (dst == 128).any()
        elif what == "hops_30":
            assert (chosen & (hops == 30)).any(), "%s: no 30-hop path provisioned" % case.name
        elif what == "hops_odd":
            assert (chosen & (hops % 2 == 1)).any() and (chosen & (hops % 2 == 0)).any()
        elif what in ("width_63", "width_64"):
            width = int(what[-2:])
            se = np.array([m.spectral_efficiency for m in topo.modulations])[topo.path_best_mod[src, dst, p]]
            n = np.ceil(svc[..., 4] / (se * 12.5)).astype(int) + 1
            assert (chosen & (n == width)).any(), "%s: no %d-slot service provisioned" % (case.name, width)
            assert n[chosen].max() == width
        elif what == "slot_ge_256":
            assert (chosen & (a[..., 1] >= 256)).any(), "%s: no service provisioned at a first slot >= 256" % case.name
        elif what == "core_last":  # RMCSA actions: (path, modulation, core, first slot)
            assert (chosen & (a[..., 2] == case.kw["num_spatial_resources"] - 1)).any(), "%s: the last core was never used" % case.name
        elif what == "c3_peak":
            pass  # judged on every step of the run, not on the host-driven part: tests/test_envelope.py
        elif what == "single_rate":
            assert (svc[..., 4] == float(case.kw["bit_rates"][0])).all()
        else:
            raise KeyError(what)
