"""The time-scale table: one base configuration per family and the powers of two both of its mean times are multiplied by, each
naming the constant of the soon list's rebuild scan (release_soon, csrc/orl_device_split.h) it sits on and the side — shared by
tests/test_timescale.py (CPU: the scaling claim on the oracle itself, and the condition every case exists for) and
tests/test_timescale_gpu.py (every step route against the oracle and against the base scale).  Helper module, no tests.

The scan selects on 32-bit keys built from (t - now) * 4096 + 2^19, clamped to [0, 2^23 - 1]: the quantum is 1/4096 time unit,
releases overdue by more than 128 units share key 0, releases more than ~1 920 units ahead saturate.  The reference has no time
unit: load = holding time / inter-arrival time fixes the dynamics, and multiplying both means by c = 2^k multiplies every time
by c exactly (rates, -log(1 - u) / rate, sums and products of times: all exact while nothing over- or underflows) and leaves
every integer and every quotient of two times as it was."""
from collections import namedtuple

import numpy as np

TOPO = "nsfnet_chen"
QUANTUM = 1.0 / 4096.0
AHEAD = 1920.0  # (2^23 - 1 - 2^19) / 4096 = 1 920 - 1/4096: where the key of a pending release saturates
OVERDUE = 128.0  # 2^19 / 4096: releases overdue by more share key 0

Base = namedtuple("Base", "fam kw h0 load policy")
_QOS = dict(num_spectrum_resources=40, num_service_classes=3, classes_arrival_probabilities=[0.2, 0.5, 0.3], classes_reward=[10.0, 2.0, 1.0],
            allow_rejection=True, episode_length=200)
BASES = {
    "RMSA": Base("RMSA", dict(num_spectrum_resources=100, allow_rejection=True, episode_length=100), 25.0, 100.0, "SAP_FF"),
    "DeepRMSA": Base("DeepRMSA", dict(j=2, episode_length=50), 7.5, 90.0, "SAP"),
    "RWA": Base("RWA", dict(allow_rejection=True, episode_length=200), 25.0, 120.0, "SAP_FF"),
    "RMCSA": Base("RMCSA", dict(num_spectrum_resources=64, num_spatial_resources=7, worst_xt=-84.7, allow_rejection=True, episode_length=100),
                  25.0, 180.0, "SAP_BM_FC_FF"),
    "QoSConstrainedRA": Base("QoSConstrainedRA", _QOS, 25.0, 300.0, "SAP_FF"),
}
FAMILIES = list(BASES)

# k: both mean times are the base's times 2^k.  constant / side: what the scale sits on.  cond: the condition the oracle's run must
# show (tests/test_timescale.py).
Scale = namedtuple("Scale", "k constant side cond")
SCALES = [
    Scale(0, "none", "control", None),
    Scale(6, "saturation 1 920 ahead", "the tail of the holding times crosses it", "ahead_both_sides"),
    Scale(7, "saturation 1 920 ahead", "most pushes beyond: the list is left with less than it must hold", "ahead_most"),
    Scale(9, "overdue clamp 128", "the mean inter-arrival gap of the RMSA base is the clamp: gaps straddle it", "gap_both_sides"),
    Scale(20, "saturation and overdue clamp", "all pushes saturated, nearly all gaps beyond the clamp, several overdue entries a lane", "gap_most_beyond"),
    Scale(30, "saturation and overdue clamp", "as 2^20, and every gap of the run beyond the clamp", "gap_all_beyond"),
    Scale(-7, "quantum 1/4096", "the inter-arrival gap is about 8 quanta", None),
    Scale(-12, "quantum 1/4096", "gaps below one quantum, holding times a few: times straddle quantum edges", "quantum_both_sides"),
    Scale(-30, "quantum 1/4096", "the whole pending set inside one quantum for the whole run", "one_quantum"),
]
KS = [s.k for s in SCALES]
# The scales above are the RMSA base's.  A family whose base misses a case's condition at that k (tests/test_timescale.py judges it
# on the oracle's stream) takes the case at the k where its own means meet the constant — the thresholds stay, the case moves:
#  - DeepRMSA's holding time of 7.5 reaches 1 920 at 2^8, not 2^6 (at 2^6 1.5 % of its pushes lie beyond, at 2^7 13 %);
#  - its gap of 7.5 / 90 and QoSConstrainedRA's of 25 / 300 reach 128 at 2^10.6 (at 2^9 5 % of the gaps are beyond);
#  - "every gap beyond 128" over 4 800 gaps needs a mean gap above ~10^7: 2^20 promises that to no base (the largest mean gap there,
#    RMSA's, is 2.6 * 10^5: one gap in 2 000 falls short), 2^30 to all of them.  So the case of the issue's k = +20 sits at 2^30 for
#    every family, and 2^20 is stepped too, under the condition every base meets there by its rates: at least 99 % of the gaps
#    beyond 128 (the smallest mean gap at 2^20, DeepRMSA's 8.7 * 10^4, leaves 0.15 % short) and two releases due at one step.
K_OF = {
    "DeepRMSA": {6: 8, 7: 9, 9: 11},
    "QoSConstrainedRA": {9: 11},
}


def ks_of(fam):
    """The family's scales, in the order of SCALES."""
    return [K_OF.get(fam, {}).get(k, k) for k in KS]


def scale_of(fam, k):
    """The row of SCALES that family `fam` takes at k."""
    return SCALES[ks_of(fam).index(k)]


# not powers of two times the base: the oracle is the only reference
PLAIN = ["defaults", "h10800_load100"]


def case_id(case):
    return case if isinstance(case, str) else "k%+d" % case


def kwargs_of(fam, case):
    """Constructor kwargs of family `fam` at `case`: an int k of SCALES, or a name of PLAIN."""
    b = BASES[fam]
    if case == "defaults":  # the reference's constructor defaults: holding time 10 800, load 10, the family's own S
        if fam == "DeepRMSA":  # (its own defaults are a holding time of 25 and a gap of 0.1: the two means are what it takes)
            return dict(mean_service_holding_time=10800.0, mean_service_inter_arrival_time=1080.0)
        return {}
    if case == "h10800_load100":
        ht, load = 10800.0, 100.0
    else:
        ht, load = b.h0 * 2.0 ** case, b.load
    kw = dict(b.kw, mean_service_holding_time=ht)
    if fam == "DeepRMSA":  # deeprmsa_env.py:22-32: load = holding time / inter-arrival time
        kw["mean_service_inter_arrival_time"] = (b.h0 / b.load) * 2.0 ** case if not isinstance(case, str) else ht / load
    else:
        kw["load"] = load
    return kw


def seeds_of(fam, n):
    return [3000 + 17 * i + len(fam) for i in range(n)]


# ---- what scales and how ------------------------------------------------------------------------------------------------
# services(): at, ht, src, dst, bit_rate, id.  link_stats(): utilization, fragmentation, compactness, last_update.
# net_stats(): throughput, compactness, last_update, clock.
def scaled(what, base, k):
    """The value the base scale's `what` must have at scale k, bit for bit: times multiplied by 2^k, everything else as it is."""
    base = np.asarray(base)
    c = 2.0 ** k
    if what == "services":
        out = base.copy()
        out[..., 0:2] *= c
        return out
    if what == "link statistics":  # [.., 4, E]
        out = base.copy()
        out[..., 3, :] *= c
        return out
    if what == "link statistics (qos)":  # [.., 2, E]: utilization, last_update
        out = base.copy()
        out[..., 1, :] *= c
        return out
    if what == "network statistics":
        out = base.copy()
        out[..., 2:4] *= c
        return out
    return base
