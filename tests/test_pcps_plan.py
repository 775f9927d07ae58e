"""The planner of an acquisition search (sydr_amd/csrc/pcps_plan.h) through tests/csrc/pcps_plan_check.hip, host only: the plan
of every request of that program -- route, PRNs per sweep, streams, shared spectra, chirp-z length, record counts, every buffer
size -- equals what tests/golden/pcps_plans.txt holds, which was recorded from the planner while it was still part of pcps.hip
(the file's first line names the commit); the program's own assertions on the route thresholds hold as well (`make
check-sanitize` runs the same program under the address and undefined-behaviour sanitizers)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_plans_equal_the_recorded_ones(tmp_path):
    exe = str(tmp_path / "pcps_plan_check")
    subprocess.run([HIPCC, "-O1", "-std=c++17", "--cuda-host-only", "-ffp-contract=off", "-o", exe,
                    os.path.join(REPO, "tests", "csrc", "pcps_plan_check.hip")], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    golden = open(os.path.join(REPO, "tests", "golden", "pcps_plans.txt")).read().splitlines()
    assert golden[0].startswith("#") and "4842865" in golden[0]
    lines = out.stdout.splitlines()
    assert len(lines) == len(golden) - 1 >= 300
    for got, want in zip(lines, golden[1:]):
        assert got == want
