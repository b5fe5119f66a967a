"""bench.py without and with --full: a plain run measures the timed steps only and leaves the figures that take runs of their
own null; --full measures them (HBM streaming peak, stand-alone slot scan, CPU baselines, host-driven rates)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "4096", "--steps", "20",
                        "--warmup", "5"] + list(flags), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_leaves_out_what_full_measures():
    plain = _bench()
    assert plain["full"] is False and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["roofline"]["achieved"] > 0 and plain["roofline"]["kernel"] == "k_persist"
    assert plain["roofline"]["peak_measured"] is None and plain["slot_scan_standalone"] is None
    assert plain["cpu_baseline"] is None and plain["host_driven"] is None

    full = _bench("--full")
    assert full["full"] is True and full["value"] > 0
    assert full["timing"]["state_preparation_steps"] == plain["timing"]["state_preparation_steps"]
    rf = full["roofline"]
    assert rf["peak_measured"] > 0 and rf["peak_measured"] == max(rf["peak_measured_read"], rf["peak_measured_copy"])
    assert full["slot_scan_standalone"]["kernel"] == "k_policy" and full["slot_scan_standalone"]["achieved"] > 0
    cpu = full["cpu_baseline"]
    assert cpu["value"] > 0 and cpu["kind"] == "port" and cpu["reference_python"]["value"] > 0
    host = full["host_driven"]
    assert host["value"] > 0 and host["agent_loop_zero_copy"]["value"] > 0
