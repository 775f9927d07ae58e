"""The work list of the fused PCPS sweep and the key it is re-used by (sydr_amd/csrc/pcps_fused_work.h) through
tests/csrc/fused_work_check.hip, host only: the check passes with the key as it is, and its part (a) -- equal keys, equal
lists -- fails with the three ints the key used to be, on the pair a 25 MHz search over 82 bins and a 50 MHz search over 41
bins make (the proof that the check would have caught the stale list; `make check-sanitize` runs the same program under
the address and undefined-behaviour sanitizers)."""
import subprocess

import pytest

import host_check


@pytest.fixture(scope="module")
def check():
    return host_check.build("fused_work_check")


@host_check.requires_hipcc
def test_work_lists_and_their_key(check):
    out = subprocess.run([check], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) >= 40 * 90 * 2 * 3


@host_check.requires_hipcc
def test_the_three_int_key_confuses_25_and_50_mhz(check):
    out = subprocess.run([check, "three-int"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1, out.stdout[-2000:]
    assert "n_prn 4 block 4: (terms 2, 41 bins: 118 units per PRN) and (terms 1, 82 bins: 154 units per PRN)" in out.stdout
    assert "82 bins) / (n_prn 4, terms 2, 41 bins) among them" in out.stdout
