"""Crafted acquisition streams whose peaks and second peaks sit where a kernel's bin bookkeeping and the two-peak
exclusion window can go wrong -- NumPy and the oracle only, seeded, cached per case (tests/test_pcps_edge_cases.py checks
the streams on the CPU, tests/test_gpu_pcps_edges.py runs them through every route of the library).

One stream carries twelve PRNs, one per placement: the PRN's code circularly shifted to column c on the carrier that row b
of the Doppler grid wipes off, at amplitude A, and where d != 0 a second copy at amplitude B, d columns away -- inside the
exclusion window, so that its flank makes the largest ALLOWED value sit on the window's boundary column.  Near the row's
ends the main triangle's own wrapped flank does the same.  `ratio_under` states the reference's window rule
(acquisition.py:78-115: `lo < 1` drops the left part, `hi >= N` drops the right part, the last column is never allowed --
none of it circular) and its six neighbours; a stream is useful because every neighbour changes some placement's ratio."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import sydr_oracle as orc

A_MAIN, B_COPY, NOISE_SIGMA = 7.0, 4.0, 2.0
PRNS = (1, 3, 6, 8, 11, 14, 17, 19, 22, 25, 28, 31)

RULES = ("reference", "left_lower", "left_higher", "right_lower", "right_higher", "last_allowed", "circular")
NEIGHBOURS = RULES[1:]

# fs, Doppler grid, intermediate frequency, non-coherent blocks, which rotation of the winning bins
Case = namedtuple("Case", "fs drange dstep if_hz noncoh rotation")
Case.__new__.__defaults__ = (5000.0, 250.0, 0.0, 1, 0)



def rotations(case, count=None):
    """the case in each of its first `count` rotations (default: as many as make every bin win)"""
    return [case._replace(rotation=r) for r in range(n_rotations(case) if count is None else count)]


# The streams of the GPU tests, by the route they are meant for (the CPU test checks every one of them).
FUSED_25 = Case(25e6, if_hz=1250.0)                        # 41 bins, classes of 4: four rotations
FUSED_25_ODD_IF = Case(25e6, if_hz=-1234.5)                # an intermediate frequency that is no multiple of the step
FUSED_50 = Case(50e6, if_hz=-2000.0)                       # two operand terms, columns as 2 m + parity
FUSED_10K = Case(10e6, dstep=300.0)                        # 34 bins, ten classes: three rotations
FUSED_10K_NONCOH = Case(10e6, dstep=300.0, if_hz=1250.0, noncoh=3)
SWEEPS_4 = Case(4e6)                                       # pcps_fastn.h
SWEEPS_12 = Case(12e6)                                     # general four-step kernels
NO_CLASSES = Case(25e6, drange=4950.0, dstep=330.0)        # 31 bins, P would be 100: every bin its own transform

Stream = namedtuple("Stream", "raw rf names cols offsets bins clipped")
Expect = namedtuple("Expect", "peak ratio row")


def geometry(fs):
    """(N samples per code, S samples per chip as the search rounds it, k: how far inside the window's right edge a second
    copy lies)"""
    n = orc.samples_per_code(fs)
    s = round(fs / orc.CODE_RATE)
    # (S = 4: a copy two columns inside the window leaves "right edge one higher" unseen; one column inside shows it)
    k = 1 if s < 6 else max(2, s // 6)
    return n, s, k


def _left_shift(s):
    """Extra columns by which the copies on the LEFT lie further out at S < 6.  The last allowed column on the left is
    c - S - 1, one further from a copy at c - (S - k) than the first allowed column c + S is from one at c + (S - k); with
    a flank of four columns and a cross-correlation floor near 2 N that one column hides the copy (4 MHz: `left edge one
    lower` moved no ratio at all)."""
    return 1 if s < 6 else 0


def placements(fs):
    """[(name, column c of the peak, offset d of the second copy or 0)] -- one PRN each, in the order of PRNS"""
    n, s, k = geometry(fs)
    e = _left_shift(s)
    return [("interior, second copy right", n // 5, s - k),
            ("interior, second copy left", n // 5, -(s - k + e)),
            ("row start", 0, 0),
            ("one past the row start", 1, 0),
            ("left branch boundary, inside", s, -(s - 2 + e)),
            ("left branch boundary, outside", s + 1, -(s - 1 + e)),
            ("right branch boundary, at it", n - s, s - k),
            ("right branch boundary, one before", n - s - 1, s - k),
            ("right branch boundary, two before", n - s - 2, s - k),
            ("row end", n - 1, 0),
            ("right branch boundary, second copy left", n - s, -(s - k + e)),
            ("plain control", n // 2, 0)]


def n_bins(case):
    return len(orc.doppler_bins(case.drange, case.dstep))


def n_rotations(case):
    """rotations after which every bin of the grid has been a winning row"""
    return -(-n_bins(case) // len(PRNS))


def winning_bins(nbins, rotation):
    """Winning row of each of the twelve placements.  The bins are dealt from the ends inwards (0, last, 1, last - 1, ...),
    so rotation 0 holds both end bins and their neighbours and rotations 0 .. ceil(nbins / 12) - 1 hold every bin."""
    order = [j // 2 if j % 2 == 0 else nbins - 1 - j // 2 for j in range(nbins)]
    return [order[(rotation * len(PRNS) + i) % nbins] for i in range(len(PRNS))]


@lru_cache(maxsize=None)
def stream(case):
    """The case's samples: interleaved int8 I, Q (`raw`), the same as complex128 (`rf`), and where its peaks were put."""
    n, s, k = geometry(case.fs)
    bins = orc.doppler_bins(case.drange, case.dstep)
    total = n * case.noncoh
    t = np.arange(total) * 2 * np.pi / case.fs
    rows = winning_bins(len(bins), case.rotation)
    x = np.zeros(total, dtype=np.complex128)
    names, cols, offsets = [], [], []
    for prn, (name, c, d), b in zip(PRNS, placements(case.fs), rows):
        code = orc.upsample_code(orc.gold_code(prn), case.fs).astype(np.float64)
        shape = A_MAIN * np.roll(code, c)
        if d:
            shape = shape + B_COPY * np.roll(code, c + d)
        x += np.tile(shape, case.noncoh) * np.exp(1j * (case.if_hz - bins[b]) * t)   # (row b mixes with if_hz - bins[b])
        names.append(name), cols.append(c), offsets.append(d)
    rng = np.random.default_rng([20261018, int(case.fs), int(case.dstep), case.noncoh, case.rotation])
    x += rng.normal(0.0, NOISE_SIGMA, total) + 1j * rng.normal(0.0, NOISE_SIGMA, total)
    iq = np.empty(2 * total)
    iq[0::2], iq[1::2] = np.rint(x.real), np.rint(x.imag)
    clipped = int(np.count_nonzero(np.abs(iq) > 127))
    raw = np.clip(iq, -127, 127).astype(np.int8)
    raw.setflags(write=False)
    rf = orc.iq_to_complex(raw)
    rf.setflags(write=False)
    return Stream(raw, rf, tuple(names), tuple(cols), tuple(offsets), tuple(rows), clipped)


@lru_cache(maxsize=None)
def expected(case):
    """Per PRN, from the oracle's map of the case's stream: ([bin, column], ratio, the winning row).  (The maps themselves
    are let go: twelve of them are 100 MB at 25 MHz.)"""
    n, s, _ = geometry(case.fs)
    x = stream(case).rf.reshape(1, -1)
    out = []
    for prn in PRNS:
        m = orc.pcps_map(x, case.if_hz, case.fs, orc.code_spectrum(orc.gold_code(prn), case.fs), case.drange, case.dstep, n,
                         1, case.noncoh)
        peak, ratio = orc.two_peak_compare(m, n, s)
        row = m[peak[0]].copy()
        row.setflags(write=False)
        out.append(Expect(peak, float(ratio), row))
    return tuple(out)


def allowed_columns(top, n, s, rule="reference"):
    """Columns of the winning row in which the second peak is looked for, top = the first peak's column."""
    lo, hi, end = top - s, top + s, n - 1
    if rule == "circular":        # the same window about the peak, continued round the row's ends
        off = (np.arange(n) - top) % n
        cols = np.nonzero((off >= s) & (off < n - s))[0]
        return cols[cols < end]
    lo += {"left_lower": -1, "left_higher": 1}.get(rule, 0)
    hi += {"right_lower": -1, "right_higher": 1}.get(rule, 0)
    if rule == "last_allowed":
        end = n
    if rule not in RULES:
        raise ValueError(rule)
    if lo < 1:
        return np.arange(hi, end)
    if hi >= n:
        return np.arange(0, lo)
    return np.r_[np.arange(0, lo), np.arange(hi, end)]


def second_column(row, top, n, s, rule="reference"):
    cols = allowed_columns(top, n, s, rule)
    return int(cols[np.argmax(row[cols])])


def ratio_under(row, top, n, s, rule="reference"):
    """first peak / second peak of the winning row under the reference's window rule or one of its neighbours"""
    return float(row[top] / np.max(row[allowed_columns(top, n, s, rule)]))
