"""What sdr_pcps_signal's request means (sydr_amd/csrc/acq_request.h acq_signal_check) through tests/csrc/acq_signal_check.hip,
host only: every refusal in the header's order, N / T / the exclusion width for awkward rates, the C/A descriptor against the
old check and the old request's unchanged answers -- and the samples per code against NumPy's rint(fs * L / chip_rate) for
the rates of the tests and a few thousand random ones (`make check-sanitize` runs the same program under the address and
undefined-behaviour sanitizers)."""
import subprocess

import numpy as np
import pytest

import host_check
from sydr_amd.dsp import signalsearch as ss


@pytest.fixture(scope="module")
def check():
    return host_check.build("acq_signal_check")


@host_check.requires_hipcc
def test_refusals_lengths_and_the_old_request(check):
    out = subprocess.run([check], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) >= 120


@host_check.requires_hipcc
def test_samples_per_code_is_numpys(check):
    triples = [(4.092e6, 4092, 1.023e6), (4.0e6, 8184, 2.046e6), (2.038e6, 1023, 1.023e6), (50e6, 4092, 1.023e6),
               (50e6, 10230, 10.23e6), (4000500.0, 1023, 1.023e6), (4001500.0, 1023, 1.023e6), (2500.0, 1, 1000.0), (3500.0, 1, 1000.0)]
    rng = np.random.default_rng(20261020)
    triples += [(float(f), int(c), float(r)) for f, c, r in zip(rng.uniform(1e6, 60e6, 3000), rng.integers(1, 20000, 3000),
                                                                rng.uniform(0.5e6, 12e6, 3000))]
    # exact halves: fs = (2 k + 1) / 2 * rate / chips with power-of-two friendly numbers
    triples += [((2 * k + 1) * 512.0, 1024, 1048576.0) for k in range(1, 200)]
    text = "".join("%s %d %s\n" % (f.hex(), c, r.hex()) for f, c, r in triples)
    out = subprocess.run([check, "lengths"], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0
    got = [int(x) for x in out.stdout.split()]
    assert got == [ss.samples_per_code(f, c, r) for f, c, r in triples]
    assert ss.samples_per_code(3 * 512.0, 1024, 1048576.0) == 2 and ss.samples_per_code(5 * 512.0, 1024, 1048576.0) == 2   # 1.5, 2.5
