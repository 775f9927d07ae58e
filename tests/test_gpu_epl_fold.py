"""The straight-line E/P/L kernels with their half blocks summed as folded sample pairs (correlator_chip.h: ChipFold) on
the GPU: 32 channels at 25 MHz, taps half a chip either side, as the headline workload runs them.  Two lists of the same
stream -- 4160 items (130 epochs: per-item setups made on the device) and its first 2048 (setups made on the host) -- both
on the straight-line variant, on
  (a) the synthetic stream,
  (b) a ring of rail values only (every byte -128 or 127: sums and differences of a pair at their extremes),
  (c) carriers of +-4 MHz (in-block rotations of about a radian per sample),
  (d) items that take the exact re-evaluation: the first item with rem_code = 0, and items whose block boundaries fall on
      or within 2^-16 of a sample (24.5 samples per chip, exactly and detuned by 1e-9: every other boundary),
against the oracle at 1e-9 of max(|prompt|, 1) and against the run-time-position kernel (epl_no_split_variant) of the same
library; (a) also at 20 MHz (block length 19) and with five taps on the half-chip view at 50 MHz.

Every item of the 4160-item list is held against the oracle (computed once per case); the 2048-item list must equal the
long list's first 2048 rows bit for bit -- the device and the host make the same setups.  The block length 19 at 20 MHz
runs four waves per SIMD and keeps the direct sum (chip_folds()): its case holds the forms that do not fold to the same
bar."""
import numpy as np
import pytest

import bench
from oracle import sydr_oracle as orc
from sydr_amd.engine import FMT_CI8, make_items

pytestmark = pytest.mark.gpu

FS = 25e6
HALF = (-0.5, 0.0, 0.5)
N_LONG, N_SHORT = 4160, 2048
TOTAL = int(0.132 * FS)                  # 132 ms: 130 whole epochs of every channel
STRAIGHT_25 = 26 + 24 + 256 * 12
RTOL = 1e-9

_cache = {}


def _codes(engine, sats):
    engine.code_slots(len(sats))
    for s, sat in enumerate(sats):
        engine.load_gps_code(s, sat["prn"])


def _stream(engine, fs=FS, total=TOTAL):
    """The headline stream's first `total` samples in a fresh ring; returns (satellites, items, ring as complex)."""
    sats = bench.satellites()
    engine.iq_alloc(total, FMT_CI8)
    _codes(engine, sats)
    engine.iq_synth(sats, fs, 12.0, 20260003, 0, total)
    key = ("stream", fs, total)
    if key not in _cache:
        items, n_epochs = bench.truth_items(sats, fs, total)
        _cache[key] = (items, orc.iq_to_complex(engine.iq_download(total, 0)))
    items, rf = _cache[key]
    return sats, items, rf


def _oracle(key, rf, sats, items, which, spacing, fs):
    """orc.epl of items[which], computed once per key."""
    if key not in _cache:
        codes = [orc.pad_code(orc.gold_code(s["prn"])) for s in sats]
        ref = np.empty((len(which), 2 * len(spacing)))
        for row, k in enumerate(which):
            it = items[k]
            a, n = int(it["start_sample"]), int(it["n_samples"])
            ref[row] = orc.epl(rf[a:a + n], codes[int(it["code_slot"])], fs, float(it["carrier_hz"]), float(it["rem_carrier"]),
                               float(it["rem_code"]), float(it["code_step"]), spacing)
        _cache[key] = ref
    return _cache[key]


def _worst(got, ref, prompt_tap):
    scale = np.maximum(np.hypot(ref[:, 2 * prompt_tap], ref[:, 2 * prompt_tap + 1]), 1.0)
    return float(np.max(np.abs(got - ref) / scale[:, None]))


def _run(engine, items, spacing, fs, want_variant, no_split=False):
    engine.set_option("epl_no_split_variant", int(no_split))
    try:
        plan = engine.epl_plan(items, spacing, fs)
        try:
            assert plan.variant == want_variant, plan.variant
            plan.run()
            return plan.fetch()
        finally:
            plan.close()
    finally:
        engine.set_option("epl_no_split_variant", 0)


def _check_both_lists(engine, name, rf, sats, items, which_extra=None):
    """The two lists of `items` on the straight-line kernel against the oracle and the run-time-position kernel."""
    assert len(items) == N_LONG
    long_got = _run(engine, items, HALF, FS, STRAIGHT_25)
    short_got = _run(engine, items[:N_SHORT], HALF, FS, STRAIGHT_25)
    assert long_got[:N_SHORT].tobytes() == short_got.tobytes()
    which = np.arange(N_LONG) if which_extra is None else which_extra
    ref = _oracle(name, rf, sats, items, which, HALF, FS)
    err = _worst(long_got[which], ref, 1)
    dyn = _run(engine, items, HALF, FS, 26 + 24, no_split=True)
    err_dyn = _worst(long_got, dyn, 1)
    print(f"{name}: worst error against the oracle {err:.3g} ({len(which)} items), against the run-time-position kernel {err_dyn:.3g}")
    assert err <= RTOL
    assert err_dyn <= RTOL
    return long_got


def test_synthetic_stream(engine):
    sats, items, rf = _stream(engine)
    _check_both_lists(engine, "a", rf, sats, items)


def test_rail_values_only(engine):
    sats, items, _ = _stream(engine)
    rng = np.random.default_rng(20261101)
    raw = np.where(rng.integers(0, 2, 2 * TOTAL) == 1, 127, -128).astype(np.int8)
    raw[:50000] = -128                               # a stretch of all-low and one of all-high samples
    raw[50000:100000] = 127
    engine.iq_upload(raw, 0)
    _check_both_lists(engine, "b", orc.iq_to_complex(raw), sats, items)


def test_carriers_of_4_mhz(engine):
    sats, items, rf = _stream(engine)
    items = items.copy()
    items["carrier_hz"] = np.where(np.arange(N_LONG) % 2 == 0, 4e6, -4e6) + items["carrier_hz"]
    _check_both_lists(engine, "c", rf, sats, items)


def _exact_path_items(items):
    """Epoch 0 of the list replaced: rem_code = 0 in the first item, then 24.5 samples per chip -- exactly (every other block
    boundary ON a sample, the taps' switches a quarter sample off) and detuned by +-1e-9 (every other boundary of the first
    620 chips within 620 * 24.5e-9 < 2^-16 of a sample) -- with code phases that put the first boundary on, just before and
    just behind a sample."""
    items = items.copy()
    items["rem_code"][0] = 0.0
    items["n_samples"][0] = int(np.ceil(1023.0 / items["code_step"][0]))
    crafted = []
    for step in (2.0 / 49.0, 2.0 / 49.0 * (1.0 + 1e-9), 2.0 / 49.0 * (1.0 - 1e-9)):
        for rem in (0.0, 0.5, 1e-9, step * (1.0 - 1e-9), 0.25 * step):
            crafted.append((step, rem))
    for k, (step, rem) in enumerate(crafted, start=1):
        items["code_step"][k] = step
        items["rem_code"][k] = rem
        items["n_samples"][k] = int(np.ceil((1023.0 - rem) / step))
    return items, 1 + len(crafted)


def _epl_long_double(x, code_padded, fs, it, spacing):
    """The oracle's expression with the carrier in long double and the chip indices of orc.epl_indices."""
    n = len(x)
    t = np.arange(n).astype(np.longdouble) / np.longdouble(fs)
    ph = -(np.longdouble(float(it["carrier_hz"])) * 2 * np.longdouble(np.pi) * t) + np.longdouble(float(it["rem_carrier"]))
    mixed = (np.cos(ph) + 1j * np.sin(ph)) * x
    out = []
    for sp in spacing:
        chips = code_padded[orc.epl_indices(n, float(it["rem_code"]), float(it["code_step"]), sp)]
        z = np.sum(chips * mixed)
        out += [float(z.real), float(z.imag)]
    return np.array(out)


def test_items_that_take_the_exact_path(engine):
    sats, items, rf = _stream(engine)
    items, n_crafted = _exact_path_items(items)
    which = np.arange(32)
    ref = _oracle("d", rf, sats, items, which, HALF, FS)
    # on the CPU: the oracle alone is within the bar for the crafted items (its own roundings against long double)
    codes = [orc.pad_code(orc.gold_code(s["prn"])) for s in sats]
    for k in range(n_crafted):
        it = items[k]
        a, n = int(it["start_sample"]), int(it["n_samples"])
        exact = _epl_long_double(rf[a:a + n], codes[int(it["code_slot"])], FS, it, HALF)
        assert _worst(ref[k:k + 1], exact[None, :], 1) <= 0.1 * RTOL, k
    _check_both_lists(engine, "d", rf, sats, items, which_extra=which)


def test_block_length_19_at_20_mhz(engine):
    fs, total = 20e6, int(0.012 * 20e6)
    sats, items, rf = _stream(engine, fs, total)
    assert len(items) == 320
    got = _run(engine, items, HALF, fs, 26 + 19 + 256 * 9)
    ref = _oracle("20", rf, sats, items, np.arange(len(items)), HALF, fs)
    dyn = _run(engine, items, HALF, fs, 26, no_split=True)
    err, err_dyn = _worst(got, ref, 1), _worst(got, dyn, 1)
    print(f"20 MHz: worst error against the oracle {err:.3g}, against the run-time-position kernel {err_dyn:.3g}")
    assert err <= RTOL and err_dyn <= RTOL


def test_five_taps_on_the_half_chip_view_at_50_mhz(engine):
    fs, total = 50e6, int(0.008 * 50e6)
    five = (-1.0, -0.5, 0.0, 0.5, 1.0)
    sats = bench.satellites()
    engine.iq_alloc(total, FMT_CI8)
    engine.code_slots(len(sats), 1023, 2)
    for s, sat in enumerate(sats):
        engine.load_gps_code(s, sat["prn"])
    engine.iq_synth(sats, fs, 12.0, 20260003, 0, total)
    items, _ = bench.truth_items(sats, fs, total)
    assert len(items) == 192
    rf = orc.iq_to_complex(engine.iq_download(total, 0))
    got = _run(engine, items, five, fs, 65536 + 26 + 24 + 4096)
    ref = _oracle("50", rf, sats, items, np.arange(len(items)), five, fs)
    dyn = _run(engine, items, five, fs, 65536 + 26 + 24, no_split=True)
    err, err_dyn = _worst(got, ref, 2), _worst(got, dyn, 2)
    print(f"50 MHz, five taps: worst error against the oracle {err:.3g}, against the run-time-position kernel {err_dyn:.3g}")
    assert err <= RTOL and err_dyn <= RTOL
