#!/usr/bin/env python3
"""Cost of copy_envs (include/orl.h, orl_batch_copy_envs; k_copy_envs in csrc/orl_copy.h) on the headline batch: cfg2, 65 536 envs,
after 300 steps of the heuristic on the device.

Cases, each timed per call with a pair of HIP events on the destination's stream (the upload of the index arrays, the copy kernel
and nothing else: RMSA has no observation to rebuild), median and best of --calls calls after 3 untimed ones:
  a  identity mapping into a second batch: env i -> env i, every env;
  b  a random permutation into a second batch;
  c  fan-out into a second batch: 8 192 sources x 8 destinations each;
  d  4 096 pairs in place (sources and destinations disjoint).  Its working set — 2 x 4 096 rows, ~70 MB — fits the 256 MB MALL
     (Infinity Cache) and the calls repeat the same rows: NOT an HBM figure;
  e  get_state() + set_state() of the same batch through the host, the only way before copy_envs: wall clock, both directions.
TB/s counts 2 x pairs x sum(state_layout()) bytes, read + written.  The yardstick for (a) is the library's own streaming copy
(k_calib_copy through orl_debug_stream_peak: what bench.py --full reports as roofline.peak_measured) over the same number of bytes,
measured in this process right before.  Writes JSON lines to --out.

    python tools/copy_rate.py [--envs 65536] [--warmup 300] [--calls 20] [--out profiles/copy_rate.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o copy -- python tools/copy_rate.py --calls 20
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import optical_rl_gym_amd as orl  # noqa: E402
from bench import WORKLOADS  # noqa: E402


def time_calls(fn, stream, calls):
    """us of every one of `calls` calls of fn (each queues work on `stream`) from its own pair of HIP events, after 3 untimed calls."""
    out = []
    for k in range(calls + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if k >= 3:
            out.append(1e3 * e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.envs
    fam, topo, kw, pol = WORKLOADS["cfg2"]
    A = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1, 1 + n)), **kw)
    D = orl.make(fam, topology=topo, num_envs=n, seeds=list(range(1 + n, 1 + 2 * n)), **kw)
    A.run(pol, args.warmup)
    D.run(pol, args.warmup)
    layout = A.state_layout()
    row = sum(layout)
    rng = np.random.default_rng(7)
    every = np.arange(n)
    perm = rng.permutation(n)
    fan_src = np.repeat(rng.choice(n, n // 8, replace=False), 8)
    k = min(4096, n // 2)
    place = rng.choice(n, 2 * k, replace=False)

    read, copy = C.c_double(), C.c_double()
    A._ck(A.lib.orl_debug_stream_peak(A.device_id, n * row, 5, C.byref(read), C.byref(copy)))
    peak_tbs = copy.value / 1e3

    cases = [("a_identity", lambda: D.copy_envs(every, every, source=A), n, "into a second batch"),
             ("b_permutation", lambda: D.copy_envs(perm, every, source=A), n, "into a second batch"),
             ("c_fan_out_8192x8", lambda: D.copy_envs(fan_src, every, source=A), n, "into a second batch; each source row is read 8 times"),
             ("d_in_place_4096", lambda: A.copy_envs(place[:k], place[k:]), k,
              "in place; the working set (2 x %d rows, %.0f MB) fits the 256 MB MALL and is reused by every call: not an HBM figure" % (k, 2 * k * row / 1e6))]
    lines = []
    device = torch.cuda.get_device_name(A.device_id)
    for name, fn, pairs, note in cases:
        stream = (A if name.startswith("d_") else D).torch_stream()
        us = time_calls(fn, stream, args.calls)
        med, best = float(np.median(us)), float(np.min(us))
        nbytes = 2 * pairs * row
        rec = dict(case=name, envs=n, pairs=pairs, bytes_per_env=row, sections=layout, bytes=nbytes, calls=args.calls,
                   us_per_call_median=round(med, 1), us_per_call_best=round(best, 1), tb_per_s_median=round(nbytes / med / 1e6, 3),
                   tb_per_s_best=round(nbytes / best / 1e6, 3), streaming_copy_tb_per_s=round(peak_tbs, 3),
                   share_of_streaming_copy_median=round(nbytes / med / 1e6 / peak_tbs, 3), note=note, device=device,
                   time=time.strftime("%Y-%m-%d %H:%M:%S"))
        print("%-18s %6d pairs: %8.1f us per call (best %8.1f), %.2f TB/s = %.2f of the streaming copy (%.2f TB/s); %s"
              % (name, pairs, med, best, rec["tb_per_s_median"], rec["share_of_streaming_copy_median"], peak_tbs, note), flush=True)
        lines.append(rec)
    A.check()
    D.check()
    # (e) through the host
    ts = []
    for _ in range(3):
        A.sync()
        t0 = time.perf_counter()
        buf = A.get_state()
        t1 = time.perf_counter()
        A.set_state(buf)
        A.sync()
        ts.append((t1 - t0, time.perf_counter() - t1))
    g, s = min(t[0] for t in ts), min(t[1] for t in ts)
    nbytes = 2 * n * row
    rec = dict(case="e_host_get_set_state", envs=n, pairs=n, bytes_per_env=row, bytes=nbytes, calls=3, us_get_state_best=round(g * 1e6, 1),
               us_set_state_best=round(s * 1e6, 1), us_per_call_best=round((g + s) * 1e6, 1), tb_per_s_best=round(nbytes / (g + s) / 1e12, 4),
               note="wall clock, pageable host buffer; the whole batch only", device=device, time=time.strftime("%Y-%m-%d %H:%M:%S"))
    print("%-18s %6d envs : get_state %.1f ms + set_state %.1f ms = %.4f TB/s" % (rec["case"], n, g * 1e3, s * 1e3, rec["tb_per_s_best"]), flush=True)
    lines.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    A.close()
    D.close()


if __name__ == "__main__":
    main()
