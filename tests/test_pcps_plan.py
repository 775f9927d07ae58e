"""The planner of an acquisition search (sydr_amd/csrc/pcps_plan.h) through tests/csrc/pcps_plan_check.hip, host only: the plan
of every request of that program -- route, PRNs per sweep, streams, shared spectra, chirp-z length, record counts, every buffer
size -- equals what tests/golden/pcps_plans.txt holds, which was recorded from the planner while it was still part of pcps.hip
(the file's first line names the commit); the program's own assertions on the route thresholds hold as well (`make
check-sanitize` runs the same program under the address and undefined-behaviour sanitizers)."""
import os
import subprocess

import host_check

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@host_check.requires_hipcc
def test_plans_equal_the_recorded_ones():
    exe = host_check.build("pcps_plan_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    golden = open(os.path.join(REPO, "tests", "golden", "pcps_plans.txt")).read().splitlines()
    assert golden[0].startswith("#") and "4842865" in golden[0]
    lines = out.stdout.splitlines()
    assert len(lines) == len(golden) - 1 >= 300
    for got, want in zip(lines, golden[1:]):
        assert got == want
