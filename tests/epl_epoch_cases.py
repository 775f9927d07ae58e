"""The item lists of tests/test_gpu_epl_epoch_moves.py, shared with tools/make_epl_epoch_golden.py, which records what a
build computes for them (tests/golden/epl_epoch_moves.npz).  Not a test file.

Every ring is filled from a seeded NumPy generator through iq_upload (uniform int8, rails included): nothing but the E/P/L
path takes part.  A case returns the rows the plan computed and what the oracle needs to recompute any of them."""
from collections import namedtuple

import numpy as np

import bench
from oracle import sydr_oracle as orc
from sydr_amd.engine import FMT_CI8, make_items

FS = 25e6
HALF = (-0.5, 0.0, 0.5)
FIVE = (-1.0, -0.5, 0.0, 0.5, 1.0)
TOTAL = int(0.132 * FS)                  # 132 ms: 130 whole epochs of 32 channels
STRAIGHT_25 = 26 + 24 + 256 * 12
SEEDS = {"ring25": 20270101, "ring20": 20270102, "ring50": 20270103, "codes50": 20270104, "short": 20270105}

# got: the plan's rows; which: the rows held against the oracle; codes: padded replica per code slot; capacity: of the ring
Case = namedtuple("Case", "got variant kernel items spacing fs rf codes which prompt_tap capacity")

_cache = {}


def _noise(name, total):
    if name not in _cache:
        _cache[name] = np.random.default_rng(SEEDS[name]).integers(-128, 128, 2 * total, dtype=np.int8)
    return _cache[name]


def _gps_ring(engine, name, fs, total):
    """A fresh ring of `total` seeded samples and the 32 C/A codes of the headline's satellites; (sats, items, rf, codes)."""
    sats = bench.satellites()
    engine.iq_alloc(total, FMT_CI8)
    engine.code_slots(len(sats))
    for s, sat in enumerate(sats):
        engine.load_gps_code(s, sat["prn"])
    raw = _noise(name, total)
    engine.iq_upload(raw, 0)
    key = ("items", name)
    if key not in _cache:
        items, _ = bench.truth_items(sats, fs, total)
        _cache[key] = (items, orc.iq_to_complex(raw), [orc.pad_code(orc.gold_code(s["prn"])) for s in sats])
    items, rf, codes = _cache[key]
    return sats, items, rf, codes


def _run(engine, items, spacing, fs, ranges=None):
    plan = engine.epl_plan(items, spacing, fs)
    try:
        if ranges is None:
            plan.run()
        else:
            for first, count in ranges:
                plan.run(first, count)
        return plan.fetch(), plan.variant
    finally:
        plan.close()


def _case(engine, items, spacing, fs, rf, codes, which, prompt_tap, capacity, waves=1, ranges=None):
    got, variant = _run(engine, items, spacing, fs, ranges)
    return Case(got, variant, bench.kernel_of_variant(variant & 65535, len(spacing), waves), items, spacing, fs, rf, codes,
                np.asarray(which), prompt_tap, capacity)


def host_setups_64(engine):
    """25 MHz, 3 taps, 32 channels x 2 epochs: a list short enough for the host to make its setups."""
    _, items, rf, codes = _gps_ring(engine, "ring25", FS, TOTAL)
    return _case(engine, items[:64].copy(), HALF, FS, rf, codes, np.arange(64), 1, TOTAL)


def device_setups_4160(engine):
    """25 MHz, 3 taps, 32 x 130: setups made by chip_setup_kernel.  Every row is held against the recorded bytes; every
    seventh (7 and 32 are coprime: every channel, 595 rows) against the oracle, which keeps the case within a few seconds
    -- tools/make_epl_epoch_golden.py holds ALL rows against the oracle before it writes the file."""
    _, items, rf, codes = _gps_ring(engine, "ring25", FS, TOTAL)
    assert len(items) == 4160
    return _case(engine, items, HALF, FS, rf, codes, np.arange(0, 4160, 7), 1, TOTAL)


def short_epochs(engine, whole_chips):
    """A partial first chip, `whole_chips` whole ones, a partial last chip (1, 63, 64, 65, 130: rounds = 1, 1, 1, 2, 3)."""
    _, items, rf, codes = _gps_ring(engine, "ring25", FS, TOTAL)
    items = items[:64].copy()
    rng = np.random.default_rng(SEEDS["short"] + whole_chips)
    step = items["code_step"]
    rem = rng.uniform(0.2, 0.8, len(items))
    rem[:4] = [0.5, 0.25, 0.75, 0.5]
    n = np.ceil((whole_chips + 1.5 - (rem - np.floor(rem))) / step).astype(np.int64)
    items["rem_code"] = rem
    items["n_samples"] = n
    items["start_sample"] = items["start_sample"] + rng.integers(0, 20000, len(items))
    assert np.all(np.ceil((n - 1) * step + rem) - np.ceil(rem) - 1 == whole_chips)
    return _case(engine, items, HALF, FS, rf, codes, np.arange(64), 1, TOTAL)


def exact_path(engine):
    """Items whose block boundaries fall on or within 2^-16 sample of a sample (tests/test_gpu_epl_fold.py builds them)."""
    from test_gpu_epl_fold import _exact_path_items
    _, items, rf, codes = _gps_ring(engine, "ring25", FS, TOTAL)
    items, n_crafted = _exact_path_items(items[:64])
    assert n_crafted == 16
    return _case(engine, items, HALF, FS, rf, codes, np.arange(64), 1, TOTAL)


def ring_wrap(engine):
    """Item 0 wraps the ring's end, item 1 ends within the 32 samples of slack behind which the chip-aligned routine does
    not apply (base < 0 in both setups: the per-sample fallback, with `spacing`, `fs` and its own constants), item 2
    starts a whole ring later (base = start_sample % capacity)."""
    _, items, rf, codes = _gps_ring(engine, "ring25", FS, TOTAL)
    items = items[:64].copy()
    items["start_sample"][0] = TOTAL - 10000
    items["start_sample"][1] = TOTAL - int(items["n_samples"][1]) - 16
    items["start_sample"][2] = TOTAL + 777
    return _case(engine, items, HALF, FS, rf, codes, np.arange(64), 1, TOTAL)


def block_19_at_20_mhz(engine):
    """20 MHz: blocks of 19 samples, direct sums, four waves per SIMD."""
    fs, total = 20e6, int(0.012 * 20e6)
    _, items, rf, codes = _gps_ring(engine, "ring20", fs, total)
    assert len(items) == 320
    return _case(engine, items, HALF, fs, rf, codes, np.arange(320), 1, total)


def five_taps_at_50_mhz(engine):
    """50 MHz, five taps a half chip apart on 8184 half-chip codes (seeded 4092-chip codes, BOC(1,1)): replicas long
    enough for four waves -- four epochs of a channel -- per workgroup.  8 channels x 3 epochs, run as the ranges
    [0, 5) and [5, 24): the first is shorter than the group stride of 8, the second no multiple of it, so both launch waves
    that hold no item."""
    fs, n_ch, chips = 50e6, 8, 4092
    total = int(0.0165 * fs)
    rng = np.random.default_rng(SEEDS["codes50"])
    engine.iq_alloc(total, FMT_CI8)
    engine.code_slots(n_ch, 2 * chips)
    codes = []
    for s in range(n_ch):
        code = np.where(rng.random(chips) < 0.5, -1, 1).astype(np.int8)
        half = np.empty(2 * chips, dtype=np.int8)
        half[0::2], half[1::2] = code, -code
        engine.set_code(s, half)
        codes.append(orc.pad_code(half.astype(np.float64)))
    raw = _noise("ring50", total)
    engine.iq_upload(raw, 0)
    dop = rng.uniform(-4500, 4500, n_ch)
    cstep = bench.CODE_RATE * (1.0 + dop / bench.L1) / fs
    cp0 = rng.uniform(0, chips, n_ch)
    start = np.ceil((chips - cp0) / cstep).astype(np.int64)
    rem = cp0 + start * cstep - chips
    rows = []
    for _ in range(3):
        n = np.ceil((chips - rem) / cstep).astype(np.int64)
        rows.append((n.copy(), start.copy(), rem.copy()))
        rem = rem + n * cstep - chips
        start = start + n
    assert np.all(start <= total)
    items = make_items(np.tile(np.arange(n_ch), 3), np.stack([r[0] for r in rows]).reshape(-1),
                       np.stack([r[1] for r in rows]).reshape(-1), np.tile(dop, 3), np.tile(rng.uniform(0, 6.0, n_ch), 3),
                       2 * np.stack([r[2] for r in rows]).reshape(-1), np.tile(2 * cstep, 3))
    return _case(engine, items, tuple(2 * t for t in FIVE), fs, orc.iq_to_complex(raw), codes, np.arange(24), 2, total,
                 waves=4, ranges=[(0, 5), (5, 19)])


# name -> (builder, the instantiation it must run on)
CASES = {
    "host_setups_64": (host_setups_64, "epl_kernel<0,3,26,24,1,12,0,0>"),
    "device_setups_4160": (device_setups_4160, "epl_kernel<0,3,26,24,1,12,0,0>"),
    "short_1": (lambda e: short_epochs(e, 1), "epl_kernel<0,3,26,24,1,12,0,0>"),
    "short_63": (lambda e: short_epochs(e, 63), "epl_kernel<0,3,26,24,1,12,0,0>"),
    "short_64": (lambda e: short_epochs(e, 64), "epl_kernel<0,3,26,24,1,12,0,0>"),
    "short_65": (lambda e: short_epochs(e, 65), "epl_kernel<0,3,26,24,1,12,0,0>"),
    "short_130": (lambda e: short_epochs(e, 130), "epl_kernel<0,3,26,24,1,12,0,0>"),
    "exact_path": (exact_path, "epl_kernel<0,3,26,24,1,12,0,0>"),
    "ring_wrap": (ring_wrap, "epl_kernel<0,3,26,24,1,12,0,0>"),
    "block_19_at_20_mhz": (block_19_at_20_mhz, "epl_kernel<0,3,26,19,1,9,0,0>"),
    "five_taps_at_50_mhz": (five_taps_at_50_mhz, "epl_kernel<0,5,26,24,4,0,1,0>"),
}
RTOL = 1e-9


def oracle_rows(case, which=None):
    """orc.epl of the case's rows `which` (default: case.which); a ring index is taken modulo the ring's length."""
    which = case.which if which is None else which
    ref = np.empty((len(which), 2 * len(case.spacing)))
    for row, k in enumerate(which):
        it = case.items[k]
        a, n = int(it["start_sample"]), int(it["n_samples"])
        a %= case.capacity
        x = case.rf[a:a + n] if a + n <= case.capacity else np.take(case.rf, (a + np.arange(n)) % case.capacity)
        ref[row] = orc.epl(x, case.codes[int(it["code_slot"])], case.fs, float(it["carrier_hz"]), float(it["rem_carrier"]),
                           float(it["rem_code"]), float(it["code_step"]), case.spacing)
    return ref


def worst_error(case, which=None):
    """Largest |got - oracle| over max(|prompt|, 1), as tests/test_gpu_epl_mask.py measures it."""
    which = case.which if which is None else which
    ref = oracle_rows(case, which)
    p = case.prompt_tap
    scale = np.maximum(np.hypot(ref[:, 2 * p], ref[:, 2 * p + 1]), 1.0)
    return float(np.max(np.abs(case.got[which] - ref) / scale[:, None]))
