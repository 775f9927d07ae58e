"""What an acquisition request means (sydr_amd/csrc/acq_request.h) through tests/csrc/acq_request_check.hip, host only: the
half-even samples per code, the status of every request that is wrong in one way -- per flavour of the check: the FFT
searches and SerialSearch differ above 65535 bins or PRNs and on the code lengths -- and the grid length against NumPy's own
len(np.arange(-R, R + 1, S)) for the pairs of test_doppler_grid_length_host_helper and a few thousand random ones (`make
check-sanitize` runs the same program under the address and undefined-behaviour sanitizers)."""
import subprocess

import numpy as np
import pytest

import host_check


@pytest.fixture(scope="module")
def check():
    return host_check.build("acq_request_check")


@host_check.requires_hipcc
def test_single_faults_and_rounding(check):
    out = subprocess.run([check], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) >= 3 * 25 + 11      # (+ SerialSearch's short-code rule at 1.0, 1.023, 4 and 16.368 MHz)


@host_check.requires_hipcc
def test_grid_length_is_numpys(check):
    pairs = [(5000.0, 250.0), (5000.0, 100.0), (5000.0, 300.0), (7000.0, 125.0), (10.0, 3.0)]
    rng = np.random.default_rng(20261020)
    pairs += [(float(r), float(s)) for r, s in zip(rng.uniform(0.0, 20000.0, 3000), rng.uniform(0.5, 2000.0, 3000))]
    # whole steps that divide 2 R + 1 or miss it by one: the ceil's own edge
    pairs += [(float(r), float(s)) for r in range(0, 60) for s in (1.0, 2.0, 3.0, 7.0, 0.25)]
    text = "".join("%s %s\n" % (r.hex(), s.hex()) for r, s in pairs)
    out = subprocess.run([check, "grid"], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    got = [int(x) for x in out.stdout.split()]
    assert got == [len(np.arange(-r, r + 1, s)) for r, s in pairs]
