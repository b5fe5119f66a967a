#!/usr/bin/env python3
"""tests/golden/view_plan.npz: the host-side decisions of the per-step device views (action masks, RMCSA masks, action completion,
spectrum assignment, path features, link features, MatrixObservationWithPaths) — the shape of a view's rows and the geometry of
its launch (wavefronts per workgroup, grid, dynamic LDS, whether rows are staged, chunked or counted, or the launch refused) — over
a grid of env families, row widths, sizes, layouts, rules and batch sizes.  No device is needed (orl_debug_view_plan).

The fixture is a record of those decisions as they were BEFORE they became pure functions (csrc/orl_view_plan.h): it was written
by this script running on commit fa2c44e with tools/record_parent_view_plan.patch applied (nothing but the query, over statements
lifted verbatim out of that commit's launchers and shape functions, and its Python binding).  tests/test_view_plan.py recomputes
every row with the library under test and compares with ==.  The file is regenerated only when a decision is changed on purpose,
never to make that test pass; the zip members carry a fixed date, so the same library gives the same bytes.

Usage:  python3 tools/gen_golden_view_plan.py [out.npz]
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "view_plan.npz")

RMSA, DEEPRMSA, RWA, RMCSA, QOS = range(5)  # ORL_ENV_*
VIEWS = ("action_mask", "rmcsa_mask", "complete", "assign", "path_features", "link_features", "matrix_paths_obs")  # ViewKind
ACTION_MASK, RMCSA_MASK, COMPLETE, ASSIGN, PATH_FEATURES, LINK_FEATURES, MATRIX_PATHS_OBS = range(7)
JOINT, PATH, PATH_MOD, CORE_SLOT = range(4)  # ORL_MASK_*
RULES = range(6)  # ORL_ASSIGN_*
KEY_COLS = ("env", "W", "B", "N", "E", "K", "C", "S", "J", "M", "view", "arg")
FIELDS = ("dim", "rows", "width", "pitch", "elem_bytes", "ok", "waves", "block", "grid", "lds_bytes", "staged", "chunk", "counted")

# a row width with the slot counts at both of its ends (512 slots is the most a batch takes)
WS = ((1, 64), (2, 65), (2, 128), (5, 129), (5, 320), (8, 321), (8, 512))
KS = (1, 5, 8, 9, 23, 24, 38, 39, 64)
CS = (1, 2, 4, 5, 7, 10, 11, 13, 22, 23, 31)  # cores (RMCSA): 1 .. 31 are accepted
ES = (1, 22, 43, 88, 128)
MS = (1, 6, 32, 33)
BS = (1, 31, 32, 33, 65536)
N0, E0, K0, J0, M0, B0 = 14, 43, 5, 8, 6, 65536  # where a size does not bear on a slice


def grid():
    """(env, W, B, N, E, K, C, S, J, M, view, arg): slices of the product, each over the sizes its view's decision reads."""
    def row(env, view, arg, W=5, S=320, B=B0, N=N0, E=E0, K=K0, C=1, J=J0, M=M0):
        return (env, W, B, N, E, K, C, S, J, M, view, arg)

    for env in (RMSA, DEEPRMSA, RWA):  # action masks: k rows of a slot row (joint) or one word
        for layout in (JOINT, PATH, PATH_MOD, CORE_SLOT):
            for K in KS:
                for W, S in WS:
                    for J in ((1, 8) if env == DEEPRMSA else (8,)):
                        yield row(env, ACTION_MASK, layout, W=W, S=S, K=K, J=J)
    for K in KS:  # RMCSA masks.  path-modulation: k words + k C runs, whatever the row width
        for Cc in CS:
            yield row(RMCSA, RMCSA_MASK, PATH_MOD, K=K, C=Cc)
    for K in (5, 64):
        for Cc in (1, 7, 31):
            for M in MS:
                for layout in (PATH_MOD, CORE_SLOT):
                    yield row(RMCSA, RMCSA_MASK, layout, K=K, C=Cc, M=M)
    for W, S in WS:  # core-slot: C slot rows, whatever k
        for Cc in CS:
            yield row(RMCSA, RMCSA_MASK, CORE_SLOT, W=W, S=S, C=Cc)
        for Cc in (7, 31):
            yield row(RMCSA, RMCSA_MASK, PATH_MOD, W=W, S=S, K=64, C=Cc)
    for K in KS:
        yield row(RMCSA, RMCSA_MASK, CORE_SLOT, W=8, S=512, K=K, C=7)
    for layout in (JOINT, PATH):  # (layouts the family does not have: dim 0)
        yield row(RMCSA, RMCSA_MASK, layout, C=7)
    for W, S in WS:  # completion, assignment: the row width alone
        yield row(RMCSA, COMPLETE, 0, W=W, S=S, C=7)
        for env in (RMSA, RWA):
            for rule in RULES:
                yield row(env, ASSIGN, rule, W=W, S=S)
    for j in (1, 8):  # path features: 1 + 2 N + rows (2 j + 3) floats
        for K in KS:
            for env in (RMSA, DEEPRMSA, RWA):
                yield row(env, PATH_FEATURES, j, K=K)
            for Cc in CS:
                yield row(RMCSA, PATH_FEATURES, j, K=K, C=Cc)
        for N in (2, 50, 512):
            for K in (5, 64):
                yield row(RMSA, PATH_FEATURES, j, N=N, K=K)
                yield row(RMCSA, PATH_FEATURES, j, N=N, K=K, C=7)
    for K in KS:  # link features: 1 + 2 N + C E (10 + k) floats beside k link sets
        for E in ES:
            for env in (RMSA, DEEPRMSA, RWA):
                yield row(env, LINK_FEATURES, 0, K=K, E=E)
            for Cc in CS:
                yield row(RMCSA, LINK_FEATURES, 0, K=K, E=E, C=Cc)
    for N in (2, 50, 512):
        for K in (5, 64):
            yield row(RMSA, LINK_FEATURES, 0, N=N, K=K)
    for K in KS + (63,):  # MatrixObservationWithPaths: E (k + 1) run lengths (QoSConstrainedRA: row width 1)
        for E in ES:
            for S in (2, 64, 320, 512):
                yield row(QOS, MATRIX_PATHS_OBS, 0, W=1, S=S, K=K, E=E)
    for B in BS:  # the batch size: the grid, in every view and at every wavefront count
        yield row(RMSA, ACTION_MASK, JOINT, B=B)
        for Cc in (1, 7, 13, 31):
            yield row(RMCSA, RMCSA_MASK, PATH_MOD, B=B, K=64, C=Cc)
        yield row(RMCSA, COMPLETE, 0, B=B, C=7)
        for rule in (0, 4):
            yield row(RMSA, ASSIGN, rule, B=B)
        for Cc in (1, 7, 13, 31):
            yield row(RMCSA, PATH_FEATURES, 8, B=B, C=Cc)
            yield row(RMCSA, LINK_FEATURES, 0, B=B, K=39, C=Cc)
        yield row(QOS, MATRIX_PATHS_OBS, 0, B=B, W=1, S=64)


def query(lib, key):
    """The FIELDS of one key, None where the query refuses its arguments."""
    out = (C.c_int32 * len(FIELDS))()
    return tuple(out) if lib.orl_debug_view_plan(*(tuple(int(v) for v in key) + (out,))) == len(FIELDS) else None


def rows():
    """[n][len(KEY_COLS) + 1 + len(FIELDS)] int32: the key columns, `valid`, then FIELDS (zeros where the query refuses)."""
    from optical_rl_gym_amd import _lib

    lib = _lib.lib()
    out = []
    for key in sorted(set(grid())):
        p = query(lib, key)
        out.append(key + (int(p is not None),) + (p or (0,) * len(FIELDS)))
    return np.array(out, np.int32)


if __name__ == "__main__":
    from gen_golden_persist_choice import write

    r = rows()
    meta = dict(columns=list(KEY_COLS + ("valid",) + FIELDS), views=list(VIEWS))
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    # (stored column by column: a column repeats itself far more than a row does)
    write(path, dict(cols=np.ascontiguousarray(r.T), meta=np.array(json.dumps(meta, sort_keys=True))))
    print("%s: %d rows, %d bytes" % (path, len(r), os.path.getsize(path)))
