"""SerialSearch (sdr_serial_search, sdr_two_peak_compare_ss) and the code upsampler where their bookkeeping can go wrong --
NumPy and the oracle only, seeded, reference maps cached (tests/test_serial_cases.py checks the catalogue on the CPU,
tests/test_gpu_serial_edges.py runs it through the library; docs/notes/serial.md has the tables).

The chip index of sample n is u(n) = trunc((ts*n)/tc) with ts = fl(1/fs), tc = fl(1/1.023e6) (gnsssignal.py:46-53).  At the
rates of RATES that are whole multiples of the chip rate the floating-point quotient falls below a whole number for a few
samples of a code period (`sensitive`): any other arithmetic (n*(ts/tc), n*1.023e6/fs, exact rationals) puts those samples
on the neighbouring chip and moves the map by 1e-4 .. 1e-2 of its maximum.  Below and at the chip rate some chips get no
sample at all, others two.  `chipsum_map` states the search as the kernels compute it (per-chip sums, then a circular
correlation) with the index as a parameter, so that the CPU half can show what a different index would do."""
from collections import namedtuple
from fractions import Fraction
from functools import cache

import numpy as np

from oracle import sydr_oracle as orc

SAT = dict(prn=7, doppler=230.0, code_phase=300.25, phase=0.1, amp=8.0)
NOISE_SIGMA, SEED = 20.0, 11
GRID = (500.0, 250.0)            # doppler_range, doppler_step: 5 bins
ONE_BIN = (0.0, 250.0)           # np.arange(0, 1, 250): the bin 0 Hz alone
PEAK = [1, 723]                  # of PRN 7 in the signal above, at every rate of RATES
ABSENT_PRN = 5

# fs; N = samples per code; chips of 0..1022 without a sample; fewest and most samples on a chip that has one; samples whose
# index differs from the exact quotient's; the highest index.  (tests/test_serial_cases.py asserts every figure.)
Rate = namedtuple("Rate", "fs n empty fewest most sensitive top")
RATES = (Rate(1.0e6, 1000, 23, 1, 1, 0, 1021),          # below the chip rate
         Rate(1.023e6, 1023, 9, 1, 2, 9, 1021),         # the chip rate: the float quotient is no longer the identity
         Rate(1.5e6, 1500, 0, 1, 2, 0, 1022),
         Rate(2.046e6, 2046, 0, 1, 3, 9, 1022),
         Rate(4.0005e6, 4000, 0, 3, 4, 0, 1022),        # N from 4000.5, rounded half to even
         Rate(4.092e6, 4092, 0, 3, 5, 9, 1022),
         Rate(16.368e6, 16368, 0, 15, 17, 9, 1022),
         Rate(38.192e6, 38192, 0, 37, 38, 3, 1022))     # the longest N
RATE_IDS = [f"{r.fs / 1e6:g}MHz" for r in RATES]

LENGTHS = (1023, 1024, 1025, 2046, 4096)   # random +-1 codes at 4 MHz: no Gold code, the workgroup's multiple, the LDS limit
SHORT = 1022                               # refused at 4 MHz (highest index 1022), searched at 1.0 MHz (highest index 1021)
NONCOH = (1, 2, 3, 5)
SEAM = dict(capacity=12008, noncoh=3, start=12008 - 5003)
MANY = dict(prns=(7, 5, 1, 12, 19, 23, 28, 31), noncoh=2, entries=40, repeated=0, oracle_entries=(0, 1, 38))

# satellite Doppler -> winning row of GRID (the search mixes with the opposite sign), code phase -> winning column
CORNER_DOPPLERS = {500.0: 0, 0.0: 2, -500.0: 4}
CORNER_PHASES = {0.1: 0, 1.1: 1022, 1022.1: 1, 511.6: 511}
INTERIOR_RATIO = (2.6, 3.3)

SMALL_SHAPES = ((1, 16), (2, 17), (3, 16), (4, 19))
TOP, SECOND = 9.0, 5.0
RULES = ("wrap_negative", "clip_negative", "cross_only", "clamp_late")


def _frozen(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------- the chip index
def exact_index(fs, n=None):
    """int(n * 1023000 / fs) in exact rationals"""
    n = orc.samples_per_code(fs) if n is None else n
    return np.array([int(Fraction(k) * 1023000 / Fraction(fs)) for k in range(n)])


def rate_facts(fs):
    """What RATES states of a rate, from orc.upsample_index."""
    n = orc.samples_per_code(fs)
    u = orc.upsample_index(fs)
    per_chip = np.bincount(u, minlength=orc.CODE_CHIPS)
    hit = per_chip[per_chip > 0]
    return Rate(fs, n, int(np.count_nonzero(per_chip[:orc.CODE_CHIPS] == 0)), int(hit.min()), int(hit.max()),
                int(np.count_nonzero(u != exact_index(fs))), int(u.max()))


# ---------------------------------------------------------------------------------------------- signals and codes
@cache
def samples(fs, blocks=1, doppler=SAT["doppler"], code_phase=SAT["code_phase"]):
    """interleaved int8 I, Q of `blocks` code periods of the catalogue's signal"""
    sat = dict(SAT, doppler=doppler, code_phase=code_phase)
    return _frozen(orc.synth_iq(fs, blocks * orc.samples_per_code(fs), [sat], NOISE_SIGMA, SEED))


def block(raw, fs, k):
    """code period k of `raw` as the [1][N] complex row the oracle takes"""
    n = orc.samples_per_code(fs)
    return orc.iq_to_complex(raw)[k * n:(k + 1) * n].reshape(1, -1)


@cache
def random_code(length):
    """+-1 chips, int8"""
    return _frozen((np.random.default_rng([20261020, length]).integers(0, 2, length) * 2 - 1).astype(np.int8))


def chips_of(code):
    """a code of the catalogue: a PRN number (Gold code) or ("random", L)"""
    return orc.gold_code(code) if isinstance(code, int) else random_code(code[1]).astype(np.float64)


# ---------------------------------------------------------------------------------------------- reference maps
@cache
def ref_block_map(fs, code, grid=GRID, k=0, blocks=1, doppler=SAT["doppler"], code_phase=SAT["code_phase"]):
    """orc.serial_search of code period k of samples(fs, blocks, ...) -> map [bins][L] (1-D for one bin)"""
    raw = samples(fs, blocks, doppler, code_phase)
    return _frozen(orc.serial_search(block(raw, fs, k), chips_of(code), grid[0], grid[1], fs, orc.samples_per_code(fs)))


@cache
def ref_map(fs, code, grid=GRID, noncoh=1, blocks=None, doppler=SAT["doppler"], code_phase=SAT["code_phase"]):
    """the per-period maps of the first `noncoh` periods added in block order (channel_l1ca_kaplan_ss.py:14-21), as 2-D"""
    blocks = noncoh if blocks is None else blocks
    total = None
    for k in range(noncoh):
        part = np.atleast_2d(ref_block_map(fs, code, grid, k, blocks, doppler, code_phase))
        total = part.copy() if total is None else total + part
    return _frozen(total)


def map_atol(ref, noncoh=1):
    return noncoh * 1e-9 * float(np.max(ref))


def chipsum_map(rf, chips, grid, fs, index):
    """The search as serial_search.hip states it: A[b][m] = the Doppler-mixed samples of chip m added up (np.add.at over
    `index`), map[b][k] = |sum_m A[b][m] * chip[(m - k) mod L]|^2 as one circulant product."""
    rf = np.squeeze(rf)
    length = len(chips)
    bins = orc.doppler_bins(*grid)
    phase_points = np.array(range(len(rf))) * 2 * np.pi / fs
    m = np.arange(length)
    circ = np.asarray(chips, dtype=np.float64)[(m[None, :] - m[:, None]) % length]       # [k][m]
    out = np.zeros((len(bins), length))
    for row, freq in enumerate(bins):
        mixed = rf * np.exp(-1j * -freq * phase_points)
        sums = np.zeros(length, dtype=np.complex128)
        np.add.at(sums, index, mixed)
        out[row] = (circ @ sums.real) ** 2 + (circ @ sums.imag) ** 2
    return out


def many_entries():
    """MANY's 40 slot numbers: slot `repeated` five times in scattered places, the other seven slots dealt over the rest"""
    rng = np.random.default_rng(20261021)
    n_slots = len(MANY["prns"])
    others = [s for s in range(n_slots) if s != MANY["repeated"]]
    entries = np.array([others[i % len(others)] for i in range(MANY["entries"])])
    rng.shuffle(entries)
    entries[[0, 7, 19, 20, 39]] = MANY["repeated"]
    return entries.astype(np.int32)


# ---------------------------------------------------------------------------------------------- the second-peak rule
def small_maps(shape):
    """For every top cell (TOP) of a map of `shape`, SECOND planted on every other cell in turn, on a seeded random base."""
    rows, cols = shape
    base = np.random.default_rng([20261022, rows, cols]).random(shape)
    for top in range(rows * cols):
        for second in range(rows * cols):
            if second == top:
                continue
            m = base.copy()
            m.flat[top], m.flat[second] = TOP, SECOND
            yield m


def tie_maps():
    """(name, map) where the maximum is not unique"""
    rng = np.random.default_rng(20261023)
    out = []
    m = rng.random((4, 19))
    m[3, 4] = m[1, 11] = TOP                          # the first in C order wins; the other lies outside its block
    out.append(("two equal maxima, apart", m))
    m = rng.random((4, 19))
    m[2, 7] = m[2, 8] = TOP                           # the other lies inside the block
    out.append(("two equal maxima, neighbours", m))
    m = rng.random((3, 16))
    m[1, 5] = m[2, 15] = TOP
    out.append(("second peak equal to the first, outside the block", m))
    m = rng.random((4, 19))
    m[0, 3] = m[0, 4] = TOP                           # row 0: nothing is excluded, the neighbour counts
    out.append(("two equal maxima in row 0", m))
    out.append(("all equal", np.full((3, 16), 2.5)))
    out.append(("all equal, one row", np.full((1, 16), 2.5)))
    out.append(("all zero", np.zeros((4, 19))))
    return out


def _excluded(top, shape, rule):
    """Boolean mask of the cells TwoCorrelationPeakComparison_SS sets to zero around `top`, stated without slices: the block
    spans [i - 1, min(i + 2, n)) per axis, and a lower end of -1 counts from the END (n - 1), which leaves the span empty
    unless n <= 2.  `rule` names a neighbouring rule:
      wrap_negative  the -1 taken circularly: index n - 1 joins 0 and 1
      clip_negative  the span clipped at 0 instead of emptied
      cross_only     the four neighbours of the peak, not the 3x3 block
      clamp_late     the upper clamp at n + 1 on cells addressed by their flat index r * ncols + c, as the kernel walks the
                     map: a block at the last column takes column 0 of the next row with it"""
    def span(i, n):
        lo, hi = i - 1, min(i + 2, n + (1 if rule == "clamp_late" else 0))
        if lo < 0:
            if rule == "wrap_negative":
                return [n - 1] + list(range(0, hi))
            lo = 0 if rule == "clip_negative" else lo + n
        return list(range(lo, hi))
    rows, cols = span(top[0], shape[0]), span(top[1], shape[1])
    mask = np.zeros(shape, dtype=bool)
    for r in rows:
        for c in cols:
            if rule == "cross_only" and r != top[0] and c != top[1]:
                continue
            flat = r * shape[1] + c
            if flat < mask.size:
                mask.flat[flat] = True
    return mask


def ratio_under(cmap, rule=None):
    """first peak / second peak under the reference's rule (None) or one of RULES"""
    if rule is not None and rule not in RULES:
        raise ValueError(rule)
    top = np.unravel_index(int(np.argmax(cmap)), cmap.shape)
    work = np.where(_excluded(top, cmap.shape, rule), 0.0, cmap)
    return cmap[top] / np.max(work)
