"""What the tests of the routing rules share (tests/test_route_spectrum.py on the oracle, tests/test_route_spectrum_gpu.py on the
device): the restated answers of one state for every rule x route, the kinds it holds, and crafted slot maps for the kinds a walk may
miss.  The shapes, walks and crowded maps are tests/assign_cases.py's.  Helper module, no tests."""
from tests import assign_cases as ac
from tests import assign_restate as ar
from tests import route_restate as rr


def prepared(fam, topo, k, S, avail, services):
    return ar.Prepared(ac.ENV_TYPE[fam], avail, services, topo, k, S), rr.Links(avail, services, topo)


def expected(fam, topo, k, S, avail, services, seen=None):
    """{rule: (table, {route: actions})} of one state; the kinds it holds are counted into `seen`"""
    prep, links = prepared(fam, topo, k, S, avail, services)
    out = {}
    for rule in rr.RULES:
        tab = rr.table(prep, links, rule)
        out[rule] = (tab, {route: rr.route(tab, route, k, S) for route in rr.ROUTES})
    if seen is not None:
        rr.count_kinds(prep, links, seen)
    return out


def craft(fam, topo, k, S, avail, services):
    """Slot maps for the kinds of min_cuts and of the routes, whatever the walk left: `avail` (bool [n, links, S]) rewritten by env
    index mod 4, n = the slots the service needs on the path named —
    0: every link free except one taken slot at n + 1 (path 0's n): a start at 0 cuts nothing, the starts behind the taken slot do;
    1: the last link of the pair's LAST path keeps only slots [3, 3 + n), every other link is free: the one fit of that path cuts
       every other hop (c* = hops - 1: 29 on a 30-hop path, every plane of the count but one);
    2: the top n + 2 slots (path 0's n) free everywhere: the winner is s = S - n (ends at the top, no cut), first fit is S - n - 2;
    3: path 0's first link keeps only the top n slots, the others are free: first fit on path 0 starts high (route best leaves path
       0) and path 0 has the fewest free slots (route least_loaded leaves it too)."""
    out = avail.copy()
    prep = ar.Prepared(ac.ENV_TYPE[fam], avail, services, topo, k, S)
    for i in range(len(services)):
        src, dst = int(services[i, 2]), int(services[i, 3])
        kind, n = i % 4, prep.need[i][0]
        if kind == 0:
            out[i] = True
            if n + 1 < S:
                out[i, :, n + 1] = False
        elif kind == 1:
            out[i] = True
            p = len(prep.need[i]) - 1
            last = int(topo.path_links[src, dst, p, int(topo.path_hops[src, dst, p]) - 1])
            out[i, last] = False
            out[i, last, 3:3 + prep.need[i][p]] = True
        elif kind == 2:
            out[i] = False
            out[i, :, max(S - n - 2, 0):] = True
        else:
            out[i] = True
            out[i, int(topo.path_links[src, dst, 0, 0]), :max(S - n, 0)] = False
    return out
