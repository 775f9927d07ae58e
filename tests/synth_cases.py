"""Shared by tests/test_synth.py (the NumPy statement alone, no GPU) and tests/test_gpu_synth.py (sdr_iq_synth on the device):
the statement of the on-device IQ synthesiser -- synth_kernel and the host half of sdr_iq_synth in sydr_amd/csrc/codes.hip,
restated line by line --, the quantisation into the ring's formats, the satellites and the case lists, and the bounds the
device is held to (docs/notes/synth.md)."""
import functools

import numpy as np

from oracle import sydr_oracle as orc

CAP = 1 << 18                                   # ring samples of the GPU tests unless said otherwise
NP_OF_FMT = {0: np.int8, 1: np.int16, 2: np.float32, 3: np.float64}
FMT_NAMES = {0: "ci8", 1: "ci16", 2: "cf32", 3: "cf64"}
RAIL = {0: 127, 1: 32767}
SEED = 20261023                                 # (data bits -1 and 0 differ for PRN 3 and for slot 0 + 1000: tests/test_synth.py)
SIGMA = 12.0
FIRST, COUNT = 12345, CAP - 12345 - 3           # the main window: an odd start, a count that is no multiple of 256
RATES = (4e6, 25e6)

BOC_SLOT = 0                                    # code slot of the staged 4092-chip code in the GPU tests
_U1_SCALE = np.float32(1.0) / np.float32(16777217.0)    # the kernel's float constants (2^-24 - 2^-48, and 2^-24)
_U2_SCALE = np.float32(1.0) / np.float32(16777216.0)


def mix64(z):
    """mix64 of the device generator (splitmix64's finaliser), vectorised over uint64 arrays; the arithmetic wraps."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def data_sign(seed, ident, bit_index):
    """+-1 of data bit `bit_index` (int64, may be negative: it wraps as the device's cast does) of the stream keyed by `ident`."""
    with np.errstate(over="ignore"):
        key = np.uint64(ident) * np.uint64(0x100000001B3) + np.asarray(bit_index, dtype=np.int64).astype(np.uint64)
        h = mix64(np.uint64(seed) ^ mix64(key))
    return np.where(h & np.uint64(1), 1.0, -1.0)


def staged_code():
    """The random 4092-chip code of the staged satellite."""
    return np.where(np.random.default_rng(4092).random(4092) < 0.5, -1, 1).astype(np.int8)


def satellites():
    """The three satellites of the prototype and one whose code phase is negative (bit index -1 at sample 0)."""
    return [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=8.0),
            dict(prn=19, doppler=-4321.5, code_phase=1022.9, phase=0.7, amp=5.0),
            dict(slot=BOC_SLOT, boc=True, doppler=2500.0, code_phase=4091.5, phase=0.3, amp=6.0),
            dict(prn=3, doppler=-250.0, code_phase=-3.5, phase=0.55, amp=4.0)]


def chips_of(sat, staged=None):
    """The +-1 chips the device uses for this satellite: the Gold code of its PRN, or the code staged in its slot."""
    if "slot" in sat:
        return np.asarray((staged or {BOC_SLOT: staged_code()})[sat["slot"]], dtype=np.int8)
    return orc.gold_code(int(sat["prn"])).astype(np.int8)


def sat_geometry(fs, n, sat, code_len):
    """(chip index, fraction of the chip, code period, bit index, carrier cycles in [-0.5, 0.5]) at sample numbers n (int64):
    the double-precision part of synth_kernel."""
    nd = n.astype(np.float64)
    L = float(code_len)
    cstep = 1.023e6 * (1.0 + sat["doppler"] / 1575.42e6) / fs
    chips = sat["code_phase"] + nd * cstep
    period = np.floor(chips / L)
    in_period = chips - period * L
    chip = np.clip(np.floor(in_period).astype(np.int64), 0, code_len - 1)
    frac = in_period - np.floor(in_period)
    bit_periods = 20 if code_len == 1023 else 1
    bit_index = np.floor(period / float(bit_periods)).astype(np.int64)
    cyc = sat.get("phase", 0.0) + nd * (sat["doppler"] / fs)
    cyc = cyc - np.rint(cyc)
    return chip, frac, period, bit_index, cyc


def _sincospi2(x, ft):
    """(sin, cos)(2 pi x) of a value already rounded to ft, the result rounded to ft: a correctly rounded sincospi(2x)."""
    a = 2.0 * np.pi * x.astype(np.float64)
    return np.sin(a).astype(ft), np.cos(a).astype(ft)


def statement(fs, first, count, sats, sigma, seed, ft=np.float64, staged=None):
    """(re, im) of samples first .. first + count - 1 before quantisation.  ft = np.float64: the definition; ft = np.float32:
    every value the kernel holds in a float is rounded to float32 after every operation (the elementary functions correctly
    rounded), which is what an ideal float32 implementation computes -- the yardstick of the float tolerance."""
    n = int(first) + np.arange(int(count), dtype=np.int64)
    re, im = np.zeros(n.size, dtype=ft), np.zeros(n.size, dtype=ft)
    for sat in sats:
        code = chips_of(sat, staged)
        ident = sat["slot"] + 1000 if "slot" in sat else sat["prn"]
        chip, frac, _, bit_index, cyc = sat_geometry(fs, n, sat, len(code))
        sgn = code[chip].astype(np.float64) * data_sign(seed, ident, bit_index)
        if sat.get("boc"):
            sgn = np.where(frac >= 0.5, -sgn, sgn)
        sn, cs = _sincospi2(cyc.astype(ft), ft)
        a = (ft(np.float32(sat["amp"])) * sgn).astype(ft)               # amp * sgn is exact
        re = (re + (a * cs).astype(ft)).astype(ft)
        im = (im + (a * sn).astype(ft)).astype(ft)
    sigma = ft(np.float32(sigma))
    if sigma > 0:
        with np.errstate(over="ignore"):
            h = mix64(np.array([seed], dtype=np.uint64) * np.uint64(0xD6E8FEB86659FD93) + n.astype(np.uint64))
        u1 = (((h >> np.uint64(40)) + np.uint64(1)).astype(ft) * ft(_U1_SCALE)).astype(ft)     # (0, 1)
        u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(ft) * ft(_U2_SCALE)            # [0, 1), exact
        lg = np.log(u1.astype(np.float64)).astype(ft)
        r = (sigma * np.sqrt((ft(-2.0) * lg).astype(ft)).astype(ft)).astype(ft)
        sn, cs = _sincospi2(u2.astype(ft), ft)
        re = (re + (r * cs).astype(ft)).astype(ft)
        im = (im + (r * sn).astype(ft)).astype(ft)
    return re, im


def quantise(re, im, fmt):
    """Interleaved I,Q as the ring of format `fmt` holds (re, im): integers rounded to even and clipped to +-127 / +-32767,
    float rings the float32 value (widened in a cf64 ring)."""
    raw = np.empty(2 * len(re), dtype=np.result_type(re, im))
    raw[0::2], raw[1::2] = re, im
    if fmt in RAIL:
        return np.clip(np.rint(raw), -RAIL[fmt], RAIL[fmt]).astype(NP_OF_FMT[fmt])
    return raw.astype(np.float32).astype(NP_OF_FMT[fmt])


def scale_of(sats, sigma):
    """S of the float tolerance: the largest signal plus 6 sigma of noise."""
    return sum(float(s["amp"]) for s in sats) + 6.0 * float(sigma)


# ---------------------------------------------------------------------------------------------------------------- case lists
def float_cases():
    """(name, fs, first, count, sats, sigma) of every window the GPU tests compare in a float ring."""
    sats = satellites()
    out = [(f"main_{int(fs)}", fs, FIRST, COUNT, sats, SIGMA) for fs in RATES]
    out.append(("ring_end", 4e6, CAP - 1000, 5000, sats, SIGMA))
    out.append(("beyond", 4e6, 5 * CAP + 77, 3001, sats, SIGMA))
    out.append(("noise_only", 4e6, FIRST, 70001, [], SIGMA))
    # (the BOC code at -0.5 chips: sample 0 lies exactly on the half-chip edge, where the flip is ">= 0.5")
    out.append(("negative_phase", 4e6, 0, 4099, [sats[3], dict(sats[2], code_phase=-0.5)], SIGMA))
    return out


def case(name):
    return next(c for c in float_cases() if c[0] == name)


@functools.lru_cache(maxsize=None)
def reference(name, seed=SEED):
    """(re, im) of a case in float64: computed once, shared, read-only."""
    _, fs, first, count, sats, sigma = case(name)
    re, im = statement(fs, first, count, sats, sigma, seed)
    re.flags.writeable = im.flags.writeable = False
    return re, im


@functools.lru_cache(maxsize=None)
def eps_ref():
    """max |statement(float64) - statement(float32)| / S over float_cases(): what float32 arithmetic alone costs."""
    worst = 0.0
    for name, fs, first, count, sats, sigma in float_cases():
        re, im = reference(name)
        re32, im32 = statement(fs, first, count, sats, sigma, SEED, ft=np.float32)
        worst = max(worst, float(max(np.max(np.abs(re - re32)), np.max(np.abs(im - im32)))) / scale_of(sats, sigma))
    return worst


FLOAT_MARGIN = 8.0                              # the device may be this many times eps_ref() off the float64 statement
INT_MAX_LSB = 1                                 # no integer sample differs by more than this from quantise(statement) ...
INT_MAX_SHARE = 1e-4                            # ... and at most this share differs at all


def float_error(raw, re, im, sats, sigma):
    """max |ring - statement| / S of a downloaded float ring window (interleaved)."""
    raw = np.asarray(raw, dtype=np.float64)
    return float(max(np.max(np.abs(raw[0::2] - re)), np.max(np.abs(raw[1::2] - im)))) / scale_of(sats, sigma)


def integer_difference(raw, re, im, fmt):
    """(largest |difference| in LSB, share of values that differ) of a downloaded integer window against the statement."""
    d = np.abs(np.asarray(raw, dtype=np.int64) - quantise(re, im, fmt).astype(np.int64))
    return int(d.max()), float(np.count_nonzero(d)) / d.size


def pattern(fmt, cap=CAP):
    """What the ring holds before a call (interleaved): every value distinct from anything the synthesiser would write there
    by accident, inside the rails of the integer formats."""
    k = np.arange(2 * cap, dtype=np.int64)
    if fmt in RAIL:
        return ((k * 37 + 11) % (2 * 101 + 1) - 101).astype(NP_OF_FMT[fmt])
    return ((k % 1013) * 0.25 - 1000.0).astype(NP_OF_FMT[fmt])


def rail_cases():
    """fmt -> (fs, first, count, sats, sigma): ci8 under noise of sigma = 40 (about 0.2 % of the values clip), ci16 under one
    satellite of amplitude 40000 (over a third of them do)."""
    return {0: (4e6, FIRST, 100003, satellites(), 40.0),
            1: (4e6, FIRST, 100003, [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=40000.0)], SIGMA)}


def all_gold_codes():
    """chips[prn - 1] of every GPS PRN 1 .. 210, from the reference's generator (tests/golden/g1_codes_all.npz)."""
    from conftest import load_golden
    return np.unpackbits(load_golden("g1_codes_all.npz")["packed"], axis=1)[:, :1023].astype(np.int8) * 2 - 1
