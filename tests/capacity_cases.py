"""The network capacity view at the edges of the accepted range and with the slot maps left in global memory: the table of shapes
shared by tests/test_network_capacity.py (CPU: each shape's launch plan pinned, and on the oracle the conditions that keep a GPU case
from passing on maps that block nothing) and tests/test_network_capacity_gpu.py (every shape on the device against the numpy
restatement).  Helper module, no tests.

Most shapes are cases of tests/envelope.py under their own names and keywords, warmed up under one of the case's own heuristics; what
is overridden where the case's own leaves the maps without a blocked cell stands in the table with the reason.  Env e is seeded
horizon_model.SEED0 + e; the warm-up is run(policy, warm)."""
from collections import namedtuple

import numpy as np

from tests import capacity_restate as cap
from tests import envelope
from tests import horizon_model as hm

# envs: of the GPU test (the restatement's path rows are what costs the time).  blocked: (min, max) over the envs of the blocked cells of
# pairs with paths after the warm-up, as the oracle showed them (tests/test_network_capacity.py asserts them); second_word: the envs with
# a cell that only a path of index >= 8 serves (k > 8)
Shape = namedtuple("Shape", "name fam topo k kw envs policy warm purpose blocked second_word")
AFTER_STEPS = 5  # policy_steps after the warm-up


def _env(name, envs, purpose, blocked, second_word=None, warm=None, policy=None, **over):
    c = envelope.CASE_BY_NAME[name]
    assert policy is None or policy in c.policies
    return Shape(name, c.fam, c.topo, c.k, dict(c.kw, **over), envs, policy or c.policies[0], c.warm if warm is None else warm, purpose, blocked, second_word)


# COST239's 412 672 and germany50's 450 560 link slots (31 x 512 x 26, 10 x 512 x 88) do not fill within a test's steps: on the oracle
# under uniform traffic germany50 blocks nothing at 8 000 Erlang after as many steps and COST239 nothing at 40 000, and at -84.7 dB every
# class is within reach of every path of both.  COST239 (an envelope case, uniform traffic): at -52 dB the reach rule puts 178 cells of
# pairs with paths beyond reach while the heuristic still provisions a third of the services (at -51 dB none; NSFNET has such cells at
# -84.7 dB).  germany50 (this file's own case): 98 % of the requests start or end in nodes 0 and 1, whose five paths fill at 3 000 Erlang
COST239_XT = -52.0
_GER_PROBS = [0.49, 0.49] + [0.02 / 48] * 48
_WXT = dict(worst_xt=-84.7, allow_rejection=True, mean_service_holding_time=10.0, episode_length=25)


def _rates(n, blocked):
    kw = dict(load=200, num_spectrum_resources=64, allow_rejection=True, mean_service_holding_time=10.0, episode_length=25,
              bit_rate_selection="discrete", bit_rates=tuple(range(25, 25 + n)))
    return Shape("nsf_s64_r%d" % n, "RMSA", "nsfnet_chen", 5, kw, 24, "SAP_FF", 400, "COUNTS ballot slices at n_cls = %d" % n, blocked, None)


SHAPES = [
    _env("ring10c8_k8_rmsa", 24, "k8 == k: no pad byte", (150, 1726)),
    _env("ring10c8_k9_rmsa", 24, "W8 = 2, one real byte in word 1", (150, 1552), 12),
    _env("ring10c8_k16_rmsa", 24, "W8 = 2, no pad", (50, 1828), 18),
    # (SAP_LF, the case's first heuristic, never takes wavelength 0: no pair is ever blocked under it)
    _env("ring10c8_k9_rwa", 24, "W8 = 2 with n_cls = 1 (64 pairs per round)", (0, 46), 4, policy="LLP_FF"),
    _env("k6full_k64_rmsa", 24, "W8 = 8, the accepted maximum", (400, 1606), 16),
    _env("k6full_k64_rwa", 24, "W8 = 8, the accepted maximum, n_cls = 1", (0, 22), 8),
    _env("k6full_k64_deep_j8", 8, "DeepRMSA through the same kernel at k = 64", (328, 1640), 5),
    _env("star65_rmsa", 8, "N > 64; n_paths in {0, 1} under k = 5; COUNTS row is the large LDS term", (117584, 173446)),
    _env("star66_rmsa", 8, "N > 64 on 65 links", (135810, 179314)),
    _env("star129_rmsa", 8, '"paths" alone, 83 205 rows; the refusal of the other two', (540842, 640992)),
    _env("ring31_rmsa", 24, "30 hops, k = 2", (0, 27906)),
    _env("s512_w64_rmsa", 24, "need = 64 at W = 8; n_cls = 2", (50, 126)),
    _env("s512_w63_rmsa", 24, "need = 63 at W = 8; n_cls = 2", (52, 122)),
    _env("one_rate_rmsa", 24, "n_cls = 1 under RMSA", (20, 94)),
    _env("rmcsa_c1", 8, "C = 1", (4412, 4412)),
    _env("rmcsa_c17", 8, "17 cores", (4482, 5034)),
    _env("rmcsa_c31_s512", 8, "the largest staged RMCSA window a shipped topology gives", (178, 178), worst_xt=COST239_XT, load=400, warm=600),
    Shape("ger_rmcsa_c10_s512", "RMCSA", "germany50", 5, dict(_WXT, load=3000, num_spectrum_resources=512, num_spatial_resources=10, node_request_probabilities=_GER_PROBS), 2,
          "SAP_BM_FC_FF", 3500, 'unstaged: "serviceable" on 2 wavefronts, "counts" on 1; "paths" staged at 63 360 B', (2370, 2852), None),
    _rates(63, (2034, 6342)), _rates(64, (2246, 5956)), _rates(65, (1172, 6466)),
]
SHAPE_BY_NAME = {s.name: s for s in SHAPES}
K_ABOVE_8 = tuple(s.name for s in SHAPES if s.k > 8)
UNSTAGED = "ger_rmcsa_c10_s512"


ENV_TYPE = {"RMSA": 0, "DeepRMSA": 1, "RWA": 2, "RMCSA": 3}
# (ok, staged, wavefronts per workgroup, LDS bytes of a workgroup) of "paths", "serviceable" and "counts", as orl_debug_capacity_plan
# answers and tests/test_network_capacity.py's expected_plan derives from the sizes.  What the numbers say: at k = 9 and 16 the longest
# runs take 16 bytes per pair (8 128 - 1 728 = 4 x 1 600), at k = 8 eight (4 x 800), at k = 64 sixty-four (4 x 36 x 64 = 9 216 beside
# 4 x 128 of maps); star65's 4 225 x 8 = 33 808 bytes (33 800 rounded to 16) leave room for one wavefront, and with the 4 304 int32 of
# its COUNTS row one wavefront above the default 48 KiB (51 536); star129's 133 136 are refused; COST239 at 31 cores of 512 slots is
# staged on one wavefront above 48 KiB in all three; germany50 at 10 cores of 512 slots stages 63 360 bytes of maps for "paths" and
# leaves them in global memory beside 20 000 bytes of longest runs (two wavefronts) and 10 304 more of counts (one)
PLANS = {
    "ring10c8_k8_rmsa": ((1, 1, 4, 1728), (1, 1, 4, 4928), (1, 1, 4, 7744)),
    "ring10c8_k9_rmsa": ((1, 1, 4, 1728), (1, 1, 4, 8128), (1, 1, 4, 10944)),
    "ring10c8_k16_rmsa": ((1, 1, 4, 1728), (1, 1, 4, 8128), (1, 1, 4, 10944)),
    "ring10c8_k9_rwa": ((1, 1, 4, 576), (1, 1, 4, 6976), (1, 1, 4, 8640)),
    "k6full_k64_rmsa": ((1, 1, 4, 512), (1, 1, 4, 9728), (1, 1, 4, 11520)),
    "k6full_k64_rwa": ((1, 1, 4, 512), (1, 1, 4, 9728), (1, 1, 4, 10368)),
    "k6full_k64_deep_j8": ((1, 1, 4, 512), (1, 1, 4, 9728), (1, 1, 4, 11520)),
    "star65_rmsa": ((1, 1, 4, 2048), (1, 1, 1, 34320), (1, 1, 1, 51536)),
    "star66_rmsa": ((1, 1, 4, 2112), (1, 1, 1, 35376), (1, 1, 1, 53104)),
    "star129_rmsa": ((1, 1, 4, 4096), (0, 0, 0, 0), (0, 0, 0, 0)),
    "ring31_rmsa": ((1, 1, 4, 3008), (1, 1, 4, 33792), (1, 1, 2, 25216)),
    "s512_w64_rmsa": ((1, 1, 4, 6336), (1, 1, 4, 12608), (1, 1, 4, 15808)),
    "s512_w63_rmsa": ((1, 1, 4, 6336), (1, 1, 4, 12608), (1, 1, 4, 15808)),
    "one_rate_rmsa": ((1, 1, 4, 704), (1, 1, 4, 6976), (1, 1, 4, 10176)),
    "rmcsa_c1": ((1, 1, 4, 704), (1, 1, 4, 6976), (1, 1, 4, 11328)),
    "rmcsa_c17": ((1, 1, 4, 11968), (1, 1, 4, 18240), (1, 1, 4, 22592)),
    "rmcsa_c31_s512": ((1, 1, 1, 58032), (1, 1, 1, 59008), (1, 1, 1, 59808)),
    "ger_rmcsa_c10_s512": ((1, 1, 1, 63360), (1, 0, 2, 40000), (1, 0, 1, 30304)),
    "nsf_s64_r63": ((1, 1, 4, 704), (1, 1, 4, 6976), (1, 1, 4, 11136)),
    "nsf_s64_r64": ((1, 1, 4, 704), (1, 1, 4, 6976), (1, 1, 4, 11136)),
    "nsf_s64_r65": ((1, 1, 4, 704), (1, 1, 4, 6976), (1, 1, 4, 11200)),
}
assert set(PLANS) == set(SHAPE_BY_NAME)


def row_words(S):
    """64-bit words of a slot row: the widths the library is built for"""
    return 1 if S <= 64 else 2 if S <= 128 else 5 if S <= 320 else 8


def plan_sizes(shape, topo):
    """(env_type, W, N, E, K, C, S, n_br) of a shape: orl_debug_capacity_plan's arguments but for the batch size, M and the layout"""
    S = spectrum_of(shape)
    n_br = len(cap.class_rates(need_family(shape), shape.kw))
    return ENV_TYPE[shape.fam], row_words(S), topo.n_nodes, topo.n_links, topo.k_paths, shape.kw.get("num_spatial_resources", 1), S, n_br


def window_bytes(spec_flags):
    """The per-env LDS window batch_create_impl checks against 64 KiB (csrc/orl_api.hip, derive_sizes), from the sizes the library
    itself derives for the configuration without a device: the -D flags of its specialisation"""
    v = {k: int(x) for k, x in (f[len("-DORL_SPEC_"):].split("=") for f in spec_flags.split() if "=" in f and f.startswith("-DORL_SPEC_"))}
    b = ((v["BMWORDS"] + 5 * v["E"] + v["OBSDIM"]) * 8 + v["CSWORDS"] * 4 + 15) // 16 * 16
    return max(b, 624 * 4)


def seeds_of(shape, n=None):
    return [hm.SEED0 + e for e in range(shape.envs if n is None else n)]


def need_family(shape):
    """DeepRMSA's needs are RMSA's over the uniform bit rates"""
    return "RMSA" if shape.fam == "DeepRMSA" else shape.fam


def cores_of(shape):
    return shape.kw.get("num_spatial_resources", 1) if shape.fam == "RMCSA" else 1


def spectrum_of(shape):
    return shape.kw["num_spectrum_resources"]


def rmcsa_tables(topology, kw):
    """slot_agent.rmcsa_tables for any topology: the tables the batch hands to the ABI, made without a device"""
    from optical_rl_gym_amd import envs

    keep = envs.ENV_CLASSES["RMCSA"]._derived(topology=topology, **kw)._keep
    return dict(n_slots=keep["n_slots"].astype(np.int64), lmax_snr=keep["lmax_snr"], lmax_xt=keep["lmax_xt"],
                rate_index={int(r): i for i, r in enumerate(keep["bit_rates"])}, path_length=keep["path_length"], path_best_mod=keep["path_mod"])


_NEED = {}


def need_of(shape, topo_path):
    """(need table, RMCSA tables or None) of a shape, computed once and left unchanged"""
    if shape.name not in _NEED:
        topo = envelope.topology_of(topo_path)
        tab = rmcsa_tables(topo_path, shape.kw) if shape.fam == "RMCSA" else None
        fam = need_family(shape)
        need = cap.need_table(fam, topo, cap.class_rates(fam, shape.kw), tab)
        need.setflags(write=False)
        _NEED[shape.name] = (need, tab)
    return _NEED[shape.name]


def restate_each(avail, topo, need):
    """cap.restate one env at a time (germany50 at 10 cores of 512 slots: 60 MB of path rows per env)"""
    parts = [cap.restate(avail[e:e + 1], topo, need) for e in range(len(avail))]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def blocked_of(counts, n_cls):
    return counts[:, :n_cls].sum(axis=1)


def only_through_second_word(paths, need, topo, n):
    """bool [n, N, N, n_cls]: the cell is serviceable and no path of index < 8 of the pair has L >= need >= 1 — a path of index >= 8
    decides it (paths: the "paths" layout [n, N N K 2] of a one-core family)"""
    N, K = topo.n_nodes, topo.k_paths
    L = paths.reshape(n, N, N, K, 2)[..., 0]
    fits = (L[..., None] >= need[None]) & (need[None] >= 1)  # [n, N, N, K, n_cls]; L = -1 where the path does not exist
    return ~fits[:, :, :, :8].any(axis=3) & fits[:, :, :, 8:].any(axis=3)
