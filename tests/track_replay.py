"""Per-epoch replay of closed-loop trajectories against the oracle's correlator (test helper, no kernel code).

Every `sdr_track_epoch` record holds the exact inputs its epoch used (start sample, length, carrier, the two NCO
remainders, code step).  `replay()` recomputes each epoch's taps with `orc.epl` from a host copy of the ring, read at
(start + i) mod capacity, with the spacing that was in effect for the epoch, and `check_nco()` checks the bookkeeping
between consecutive records with the oracle loops' own update statements.  The bar for the taps is a rounding-error
scale, |d(I + jQ)| <= BAR * sum_i |x_i| over the epoch's samples: it holds for noise-only taps and for tracked prompts
alike, and a one-sample error in any tap of any core is orders of magnitude above it.

`expected_core()` restates the kernel's per-epoch choice of correlator (track_kernel.h) so that a test can prove which
cores its epochs actually reached; the thresholds are read from the kernel's headers.  It predicts no results."""
import math
import os
import re

import numpy as np

from oracle import sydr_oracle as orc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sydr_amd", "csrc")
BAR = 1e-11          # |d(I + jQ)| / sum |x| per epoch and tap
NCO_RTOL = 1e-12     # NCO hand-over between records, each against its own scale

# ring formats by name, as the engine numbers them
FORMATS = ("ci8", "ci16", "cf32", "cf64")
FORM_PARTS = {"W512": 1, "C2": 2, "C4": 4, "C8": 8, "D": 1}
CORES = ("PS", "B8", "B16", "SG", "CH")
_GROUP, _WIDE, _CLUSTER_THREADS = 8, 16, 256   # kGroup, kWide (correlator.h); threads of a cluster workgroup


def _read_thresholds():
    names = ("kFastMinCodeStep", "kFastMaxCodeStep", "kFastMaxCodeStep8", "kChipMinCodeStep", "kChipMaxCodeStep")
    num = r"[0-9]+(?:\.[0-9]*)?(?:[eE][-+]?[0-9]+)?"
    found = {}
    for header in ("correlator.h", "correlator_chip.h"):
        with open(os.path.join(CSRC, header)) as f:
            text = f.read()
        for name, a, b in re.findall(rf"constexpr\s+double\s+(k\w+)\s*=\s*({num})\s*(?:/\s*({num}))?\s*;", text):
            if name in names:
                found[name] = float(a) / float(b) if b else float(a)    # (one correctly rounded division, as in C++)
    missing = set(names) - set(found)
    if missing:
        raise RuntimeError(f"core thresholds not found in the kernel headers: {sorted(missing)}")
    return found


THRESHOLDS = _read_thresholds()


def _read_chip_block():
    """The block length the closed-loop kernel compiles into its chip-aligned core (chip_geometry<3, KM, 0, 0>): any other
    block length sets G.bad, and the epoch falls back to the boundary variants."""
    with open(os.path.join(CSRC, "track_kernel.h")) as f:
        found = re.findall(r"chip_geometry<3,\s*(\d+),\s*0,\s*0>", f.read())
    if len(set(found)) != 1:
        raise RuntimeError(f"closed-loop chip-aligned block length not found in track_kernel.h: {found}")
    return int(found[0])


CHIP_BLOCK = _read_chip_block()


def epoch_wraps(start, n, capacity):
    """correlator.h epoch_wraps(): the epoch (start rounded down to a multiple of 8, plus one 16-sample group of
    slack) crosses the end of the ring.  `start` is the absolute sample index."""
    aligned = start & ~(_GROUP - 1)
    return aligned % capacity + (start - aligned) + n + _WIDE > capacity


def expected_core(form, fmt, n_taps, s, n, pos, capacity, parts=None, prefix=True):
    """The correlator the closed-loop kernel picks for one epoch (track_kernel.h, the epoch loop):

    form      "W512" (512 threads, one workgroup per channel), "C2" / "C4" / "C8" (clusters of 256-thread workgroups) or
              "D" (256 threads, one workgroup per channel, more channels than compute units)
    fmt       ring format name ("ci8", "ci16", "cf32", "cf64")
    s, n      code step (chips per sample) and length of the epoch
    pos       absolute start sample of the epoch (the kernel keeps pos % capacity as its ring position)
    parts     workgroups per channel (default: from the form's name)
    prefix    the launcher found LDS for the boundary variants' prefix strips (true for single-period codes)

    Returns "PS", "B8", "B16", "SG" or "CH".  The closed loop tries the chip-aligned core for 1/25.9 <= s <= 1/15.5, but
    compiles its block length in (CHIP_BLOCK): with M = floor(2^32 / s) >> 32 samples per block (rounded as
    chip_geometry() does) any other M sets G.bad, and the epoch takes B16 / B8 -- this rule is applied here.  "CH" still
    means the chip-aligned core OR its fallback: the tap-geometry part of G.bad and the core's own per-epoch fallback
    are not visible from outside."""
    t = THRESHOLDS
    parts = FORM_PARTS[form] if parts is None else parts
    ring_pos = pos % capacity
    cluster = form.startswith("C")
    if cluster:
        groups = -(-n // _WIDE)
        fits = ring_pos + groups * _WIDE <= capacity
        if prefix and t["kFastMinCodeStep"] <= s <= t["kFastMaxCodeStep"] and fits and groups <= parts * _CLUSTER_THREADS:
            return "SG"
    boundary_ok = prefix and s >= t["kFastMinCodeStep"] and not epoch_wraps(pos, n, capacity)
    if (form == "D" and fmt == "ci8" and n_taps == 3 and boundary_ok and t["kChipMinCodeStep"] <= s <= t["kChipMaxCodeStep"]
            and ring_pos + n + 32 <= capacity and int(np.rint((1.0 / s) * 4294967296.0)) >> 32 == CHIP_BLOCK):
        return "CH"
    if boundary_ok and s <= t["kFastMaxCodeStep"]:
        return "B16"
    if boundary_ok and s <= t["kFastMaxCodeStep8"]:
        return "B8"
    return "PS"


# ------------------------------------------------------------------------------------------------ records
def columns(records):
    """Records as a dict of arrays: a trajectory row of the device (TRACK_EPOCH_DTYPE) or the oracle loops' dicts."""
    if isinstance(records, np.ndarray) and records.dtype.names:
        r = records
        out = dict(start=r["start_sample"].astype(np.int64), n=r["n_samples"].astype(np.int64),
                   carrier_hz_in=r["carrier_hz_in"], rem_carrier_in=r["rem_carrier_in"], rem_code_in=r["rem_code_in"],
                   code_step_in=r["code_step_in"], corr=r["corr"], carrier_hz=r["carrier_hz"], code_hz=r["code_hz"],
                   lock_state=r["lock_state"].astype(np.int64))
        return out
    key = {"start": "start", "n": "n"}
    out = {k: np.array([rec[key.get(k, k)] for rec in records]) for k in
           ("start", "n", "carrier_hz_in", "rem_carrier_in", "rem_code_in", "code_step_in", "carrier_hz", "code_hz")}
    out["start"], out["n"] = out["start"].astype(np.int64), out["n"].astype(np.int64)
    out["corr"] = np.array([rec["corr"] for rec in records], dtype=np.float64)
    out["lock_state"] = np.array([rec.get("lock_state", 0) for rec in records], dtype=np.int64)
    return out


def ring_complex(raw):
    """Interleaved I,Q of any ring format -> complex128 (float32 widened first: no complex64 on the way)."""
    raw = np.asarray(raw).astype(np.float64)
    return raw[0::2] + 1j * raw[1::2]


def spacings(cols, kind, wide, narrow, initial_narrow=False):
    """Taps in effect per epoch.  Borre (kind 0): fixed.  Kaplan (kind 1): narrow exactly when the previous record ends
    in LOCK_NARROW (KaplanLoop.step switches the taps with the lock state); epoch 0 takes the initial state's."""
    wide, narrow = [float(v) for v in wide], [float(v) for v in narrow]
    if kind == 0:
        return [wide] * len(cols["n"])
    sel = np.empty(len(cols["n"]), dtype=bool)
    sel[0] = bool(initial_narrow)
    sel[1:] = cols["lock_state"][:-1] == orc.LOCK_NARROW
    return [narrow if s else wide for s in sel]


def replay(cols, ring, fs, code, taps, epochs=None):
    """Expected taps of the epochs `epochs` (default: all) of one channel.

    ring: complex128 host copy of the whole ring (len = capacity); code: the +-1 code (unpadded); taps: per-epoch spacing
    lists (`spacings`).  Returns (expected [k][2 * n_taps], sum_i |x_i| [k]) for the selected epochs."""
    capacity = len(ring)
    padded = orc.pad_code(np.asarray(code, dtype=np.float64))
    ks = range(len(cols["n"])) if epochs is None else epochs
    exp, scale = [], []
    for k in ks:
        start, n = int(cols["start"][k]), int(cols["n"][k])
        if start % capacity + n <= capacity:
            x = ring[start % capacity:start % capacity + n]
        else:
            x = ring[(start + np.arange(n)) % capacity]
        exp.append(orc.epl(x, padded, fs, cols["carrier_hz_in"][k], cols["rem_carrier_in"][k], cols["rem_code_in"][k],
                           cols["code_step_in"][k], taps[k]))
        scale.append(np.abs(x).sum())
    return np.array(exp, dtype=np.float64), np.array(scale)


def tap_ratios(got, expected, scale):
    """|d(I + jQ)| / sum |x| per epoch and tap."""
    got, expected = np.asarray(got)[:, :expected.shape[1]], np.asarray(expected)
    err = np.hypot(got[:, 0::2] - expected[:, 0::2], got[:, 1::2] - expected[:, 1::2])
    return err / np.maximum(scale, 1e-300)[:, None]


def check_nco(cols, fs, kind, n0=None, epoch_chips=float(orc.CODE_CHIPS)):
    """The NCO hand-over between records k and k+1, by the oracle loops' own update statements (KaplanLoop.step /
    BorreLoop.step).  Integers exact; carrier and code step relative, the code remainder against 1 chip and the carrier
    remainder against 2 pi (circularly).  n0: the initial state's epoch length.  Returns a list of failures."""
    c = cols
    two_pi = orc.GPS_TWO_PI if kind == 1 else 2 * np.pi
    bad = []
    m = len(c["n"])
    if n0 is not None and m and int(c["n"][0]) != int(n0):
        bad.append(("n", 0, int(c["n"][0]), int(n0)))
    for k in range(1, m):
        want = int(math.ceil((epoch_chips - c["rem_code_in"][k]) / c["code_step_in"][k]))
        if int(c["n"][k]) != want:
            bad.append(("n", k, int(c["n"][k]), want))
    for k in range(m - 1):
        n = int(c["n"][k])
        if int(c["start"][k + 1]) != int(c["start"][k]) + n:
            bad.append(("start", k + 1, int(c["start"][k + 1]), int(c["start"][k]) + n))
        if abs(c["carrier_hz_in"][k + 1] - c["carrier_hz"][k]) > NCO_RTOL * abs(c["carrier_hz"][k]):
            bad.append(("carrier_hz_in", k + 1, c["carrier_hz_in"][k + 1], c["carrier_hz"][k]))
        step = c["code_hz"][k] / fs
        if abs(c["code_step_in"][k + 1] - step) > NCO_RTOL * abs(step):
            bad.append(("code_step_in", k + 1, c["code_step_in"][k + 1], step))
        rem_code = c["rem_code_in"][k] + n * c["code_step_in"][k] - epoch_chips
        if abs(c["rem_code_in"][k + 1] - rem_code) > NCO_RTOL:
            bad.append(("rem_code_in", k + 1, c["rem_code_in"][k + 1], rem_code))
        rem_carrier = c["rem_carrier_in"][k] - c["carrier_hz_in"][k] * two_pi * n / fs
        rem_carrier %= two_pi
        d = (c["rem_carrier_in"][k + 1] - rem_carrier + two_pi / 2) % two_pi - two_pi / 2
        if abs(d) > NCO_RTOL * two_pi:
            bad.append(("rem_carrier_in", k + 1, c["rem_carrier_in"][k + 1], rem_carrier))
    return bad


def classify(cols, form, fmt, n_taps, capacity, parts=None, epochs=None):
    """expected_core() of every (selected) epoch of one channel's records."""
    ks = range(len(cols["n"])) if epochs is None else epochs
    return [expected_core(form, fmt, n_taps, float(cols["code_step_in"][k]), int(cols["n"][k]), int(cols["start"][k]),
                          capacity, parts) for k in ks]
