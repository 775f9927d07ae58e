"""The decisions of an E/P/L plan's creation (sydr_amd/csrc/epl_plan.h) through tests/csrc/epl_plan_check.hip, host only: the
route of a list by its length, its memory, its buffers, the half-chip view and its setups; the several-chips-per-lane shape and
the rule on strays; group_stride; the half-chip view's choice; and the fold of a list's statistics, item by item and merged
from scrambled parts, against the walk sdr_epl_plan_create did before the fold existed.  The expected values stand in the
program (`make check-sanitize` runs it under the address and undefined-behaviour sanitizers)."""
import subprocess

import host_check


@host_check.requires_hipcc
def test_every_decision_of_a_plans_creation():
    exe = host_check.build("epl_plan_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    words = out.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 70, out.stdout
