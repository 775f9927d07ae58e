"""Scenes of the signal-search tests (tests/test_signal_search_statement.py on the CPU, tests/test_gpu_signal_search.py on the
GPU): seeded +-1 codes whose data sign changes at code periods, a code start in the middle of the search window, and the three
geometries of the tests.  Host arithmetic only."""
import numpy as np

from sydr_amd.dsp import signalsearch as ss

# name -> (fs, chips, chip rate, N, BOC: the searched code is the half-chip code of a `chips / 2`-chip code, excl_samples)
GEOMETRIES = {
    "a_16368": (4.092e6, 4092, 1.023e6, 16368, False, 0),       # T = 32736 = 2^5 3 11 31: radices 11 and 31
    "b_16000": (4.0e6, 8184, 2.046e6, 16000, True, 4),          # a doubled BOC code, side peaks excluded
    "c_2038": (2.038e6, 1023, 1.023e6, 2038, False, 0),         # N = 2 x 1019, T = 4 x 1019: chirp-z
}
RANGE, STEP = 1000.0, 250.0                                     # nine bins
DOPPLER = -500.0                                                # of the signal: the peak is the bin of +500 Hz
TRUE_BIN = int(np.flatnonzero(np.arange(-RANGE, RANGE + 1, STEP) == -DOPPLER)[0])
AMP, SIGMA = 6.0, 20.0
SEED = 20261020


def codes_for(name, n_prn, seed=SEED):
    """(searched codes [n_prn][chips] int8): seeded stand-ins, no real signal's memory codes."""
    fs, chips, rate, n_code, boc, excl = GEOMETRIES[name]
    rng = np.random.default_rng([seed, chips])
    base = np.where(rng.random((n_prn, chips // 2 if boc else chips)) < 0.5, -1, 1).astype(np.int8)
    return np.stack([ss.boc_doubled(c) for c in base]) if boc else base


def code_start(name, prn=0):
    n_code = GEOMETRIES[name][3]
    return n_code // 2 + 37 + 11 * prn


def scene(name, n_prn, periods, seed=SEED, signs=None, amp=AMP, sigma=SIGMA):
    """(raw int8 I/Q interleaved of periods * N samples, codes): every PRN at DOPPLER, its code period starting at
    code_start(name, prn), its sign changing from period to period (`signs`: the sequence, default +,-: a flip at every period)."""
    fs, chips, rate, n_code, boc, excl = GEOMETRIES[name]
    codes = codes_for(name, n_prn, seed)
    total = periods * n_code
    n = np.arange(total)
    if signs is None:
        signs = np.array([1, -1])
    x = np.zeros(total, dtype=np.complex128)
    for p in range(n_prn):
        rep = ss.replica(codes[p].astype(np.float64), fs, rate, n_code)
        k = n - code_start(name, p)
        sign = np.asarray(signs)[(k // n_code) % len(signs)]
        x += amp * sign * rep[k % n_code] * np.exp(2j * np.pi * (DOPPLER / fs * n + 0.1 * (p + 1)))
    rng = np.random.default_rng([seed, 1, n_code])
    x += sigma * (rng.standard_normal(total) + 1j * rng.standard_normal(total))
    raw = np.empty(2 * total, dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return raw, codes


def to_complex(raw):
    return raw[0::2] + 1j * raw[1::2]


def statement(name, raw, codes, pad, noncoh=1, coh=1, start=0, excl=None):
    fs, chips, rate, n_code, boc, excl0 = GEOMETRIES[name]
    return ss.pcps_signal_statement(to_complex(raw), codes, fs, 0.0, RANGE, STEP, rate, pad=pad,
                                    excl_samples=excl0 if excl is None else excl, coh=coh, noncoh=noncoh, start_sample=start)
