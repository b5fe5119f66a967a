#!/usr/bin/env python3
"""Golden vectors at the edges of the accepted configuration range, recorded by IMPORTING THE REFERENCE.

TEST INFRASTRUCTURE — runs only where the reference tree exists (ORL_REFERENCE, see gen_golden.py), never on a GPU box.
For the synthetic topologies of tests/envelope.py (GOLDEN_TOPOLOGIES: k = 9, k = 64, 129 nodes / 128 links with one path per
pair, 30 hops) the reference's OWN topology builder (get_topology of its examples/create_topology.py) reads the same raw file;
its graph is flattened with topology_io.topology_from_reference_graph and
  tests/golden/topo_<name>_k<k>.npz   the tables (data; tests/test_envelope.py compares topology_io.build_topology with them)
  tests/golden/e*.npz                 step traces in the layout of gen_golden.py (run_trace), meta["topology"] = the topo_*.npz
are written.  Zip members carry a fixed date: the same reference gives the same bytes.

Usage:  cd /tmp && PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python3 -W ignore <repo>/oracle/gen_golden_envelope.py
"""
import contextlib
import io
import os
import sys
import tempfile
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import gen_golden as gg  # noqa: E402  (imports the reference through the shim)
import numpy as np  # noqa: E402

sys.path.insert(0, os.path.join(gg.REF, "examples"))
import create_topology as ref_topology  # noqa: E402
from optical_rl_gym.envs import deeprmsa_env, rmsa_env, rwa_env  # noqa: E402

from optical_rl_gym_amd.topology_io import save_topology, topology_from_reference_graph  # noqa: E402
from tests import envelope  # noqa: E402


def _savez_fixed_date(path, **arrays):
    """np.savez_compressed with a fixed date on every member (tools/gen_golden_persist_choice.py does the same)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


np.savez_compressed = _savez_fixed_date  # what gg.run_trace and save_topology write through


def reference_graph(name, k, directory):
    raw = os.path.join(directory, name + ".txt")
    with open(raw, "w") as f:
        f.write(envelope.raw_text(name))
    with contextlib.redirect_stdout(io.StringIO()):  # (it prints every path)
        return ref_topology.get_topology(raw, name.upper(), ref_topology.modulations, k)


def topo_file(name, k):
    return "topo_%s_k%d.npz" % (name, k)


def trace(fixture, case_name, graphs, policy_name, policy_fn, n_steps, seed=10, actions=None, obs=False, **extra):
    c = envelope.CASE_BY_NAME[case_name]
    kw = dict(envelope.oracle_kwargs(c), seed=seed, **extra)
    ref_kw = dict(kw)
    if "node_request_probabilities" in ref_kw:
        ref_kw["node_request_probabilities"] = np.array(ref_kw["node_request_probabilities"])
    env = gg.gym.make({"RMSA": "RMSA-v0", "DeepRMSA": "DeepRMSA-v0", "RWA": "RWA-v0"}[c.fam], topology=graphs[(c.topo, c.k)], **ref_kw)
    gg.run_trace(fixture, env, policy=policy_fn, actions=actions, n_steps=n_steps,
                 info_keys=gg.RWA_INFO if c.fam == "RWA" else gg.RMSA_INFO, snapshot_every=250,
                 obs_fn=(lambda e: e.observation()) if obs else None,
                 vec_info_keys=("path_action_probability", "wavelength_action_probability") if c.fam == "RWA" else (),
                 meta=dict(env=c.fam, topology=topo_file(c.topo, c.k), kwargs=kw, policy=policy_name, case=case_name))


def main():
    graphs = {}
    with tempfile.TemporaryDirectory() as d:
        for name, k in envelope.GOLDEN_TOPOLOGIES:
            g = reference_graph(name, k, d)
            graphs[(name, k)] = g
            t = topology_from_reference_graph(g)
            save_topology(t, os.path.join(gg.GOLD, topo_file(name, k)))
            print("topology %s k %d: N %d E %d Hmax %d" % (name, k, t.n_nodes, t.n_links, t.max_hops))
    sapff, llpff = rmsa_env.shortest_available_path_first_fit, rmsa_env.least_loaded_path_first_fit
    # k = 9 and k = 64: policies that reach path indices >= 8, DeepRMSA's observation with j = 8
    trace("e1_rmsa_ring10c8_k9_sapff", "ring10c8_k9_rmsa", graphs, "SAP_FF", sapff, 700)
    trace("e1_rmsa_ring10c8_k9_llpff", "ring10c8_k9_rmsa", graphs, "LLP_FF", llpff, 500)
    trace("e1_deeprmsa_ring10c8_k9_j8_sap", "ring10c8_k9_deep_j8", graphs, "SAP", deeprmsa_env.shortest_available_path_first_fit, 800, obs=True)
    trace("e1_rwa_ring10c8_k9_saplf", "ring10c8_k9_rwa", graphs, "SAP_LF", rwa_env.shortest_available_path_last_fit, 700)
    trace("e2_rmsa_k6full_k64_sapff", "k6full_k64_rmsa", graphs, "SAP_FF", sapff, 600)
    trace("e2_deeprmsa_k6full_k64_j8_sap", "k6full_k64_deep_j8", graphs, "SAP", deeprmsa_env.shortest_available_path_first_fit, 400, obs=True)
    # 129 nodes, 128 links, one path per pair
    trace("e3_rmsa_star129_llpff", "star129_rmsa", graphs, "LLP_FF", llpff, 900)
    trace("e3_rwa_star129_saplf", "star129_rwa", graphs, "SAP_LF", rwa_env.shortest_available_path_last_fit, 700)
    # 30 hops; a stored action stream (valid / busy / out-of-range / reject)
    trace("e4_rmsa_ring31_sapff", "ring31_rmsa", graphs, "SAP_FF", sapff, 500)
    trace("e4_rmsa_ring31_random_actions", "ring31_rmsa", graphs, "ACTIONS", None, 800, seed=7,
          actions=gg.random_actions(4242, 800, 2, 70))
    for f in sorted(os.listdir(gg.GOLD)):
        if f.startswith(("e", "topo_")):
            print("%-44s %7d bytes" % (f, os.path.getsize(os.path.join(gg.GOLD, f))))


if __name__ == "__main__":
    main()
