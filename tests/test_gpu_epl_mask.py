"""The straight-line E/P/L kernels with a block's optional samples masked instead of selected (correlator_chip.h:
chip_mask_shares; tests/test_chip_mask.py holds one block's arithmetic on the CPU) on the GPU: 32 channels, taps half a chip
either side, lists of 4160 items and their first 2048 at 25 MHz, against the oracle at 1e-9 of max(|prompt|, 1) and against
the run-time-position kernel (epl_no_split_variant) of the same library, on
  (a) the synthetic stream,
  (b) a ring of rail values only,
  (c) carriers of +-4 MHz,
  (d) items on the exact path (rem_code = 0; 24.5 samples per chip, exactly and detuned by 1e-9): there a block's flags come
      from the integers the exact re-evaluation leaves, not from the carries of the block's fraction;
one list per kind of form -- 20 MHz (block length 19: taps switching inside the block, direct sum, four waves per SIMD),
32 MHz on the half-chip view (three whole-chip taps, folded), 40 MHz on the half-chip view (three whole-chip taps, direct),
five taps at 50 MHz -- and short epochs of 1, 63, 64, 65 and 130 whole chips (one round with one lane, with all but one and
with every lane at work; the clamped pair of rounds alone; an odd round count), where the last round's clamp meets the edge
samples.  Every case asserts the plan's variant.

The streams, items and oracle results of (a) .. (d), 20 MHz and 50 MHz are those of tests/test_gpu_epl_fold.py, computed once
for both files."""
import numpy as np
import pytest

import bench
from oracle import sydr_oracle as orc
from sydr_amd.engine import FMT_CI8
from test_gpu_epl_fold import (FS, HALF, N_LONG, RTOL, STRAIGHT_25, TOTAL, _check_both_lists, _exact_path_items, _oracle, _run, _stream,
                               _worst)

pytestmark = pytest.mark.gpu

DOUBLED, WHOLE_CHIP_TAPS = 65536, 4096


def test_synthetic_stream(engine):
    sats, items, rf = _stream(engine)
    _check_both_lists(engine, "a", rf, sats, items)


def test_rail_values_only(engine):
    sats, items, _ = _stream(engine)
    rng = np.random.default_rng(20261101)
    raw = np.where(rng.integers(0, 2, 2 * TOTAL) == 1, 127, -128).astype(np.int8)
    raw[:50000] = -128
    raw[50000:100000] = 127
    engine.iq_upload(raw, 0)
    _check_both_lists(engine, "b", orc.iq_to_complex(raw), sats, items)


def test_carriers_of_4_mhz(engine):
    sats, items, rf = _stream(engine)
    items = items.copy()
    items["carrier_hz"] = np.where(np.arange(N_LONG) % 2 == 0, 4e6, -4e6) + items["carrier_hz"]
    _check_both_lists(engine, "c", rf, sats, items)


def test_items_on_the_exact_path(engine):
    sats, items, rf = _stream(engine)
    items, n_crafted = _exact_path_items(items)
    assert n_crafted == 16
    _check_both_lists(engine, "d", rf, sats, items, which_extra=np.arange(32))


def _one_list(engine, name, fs, total, spacing, want, want_dyn, half_chip_view, prompt_tap):
    sats = bench.satellites()
    engine.iq_alloc(total, FMT_CI8)
    if half_chip_view:
        engine.code_slots(len(sats), 1023, 2)
    else:
        engine.code_slots(len(sats))
    for s, sat in enumerate(sats):
        engine.load_gps_code(s, sat["prn"])
    engine.iq_synth(sats, fs, 12.0, 20260003, 0, total)
    items, _ = bench.truth_items(sats, fs, total)
    rf = orc.iq_to_complex(engine.iq_download(total, 0))
    got = _run(engine, items, spacing, fs, want)
    ref = _oracle(name, rf, sats, items, np.arange(len(items)), spacing, fs)
    engine.set_option("epl_no_split_variant", 1)
    try:
        plan = engine.epl_plan(items, spacing, fs)
        try:
            assert plan.variant in want_dyn, plan.variant
            plan.run()
            dyn = plan.fetch()
        finally:
            plan.close()
    finally:
        engine.set_option("epl_no_split_variant", 0)
    err, err_dyn = _worst(got, ref, prompt_tap), _worst(got, dyn, prompt_tap)
    print(f"{name}: {len(items)} items, worst error against the oracle {err:.3g}, against the run-time-position kernel {err_dyn:.3g}")
    assert err <= RTOL and err_dyn <= RTOL
    return len(items)


def test_block_length_19_at_20_mhz(engine):
    assert _one_list(engine, "20", 20e6, int(0.012 * 20e6), HALF, 26 + 19 + 256 * 9, (26,), False, 1) == 320


def test_whole_chip_taps_folded_at_32_mhz(engine):
    # (15.6 samples per half chip: the no-split arm takes the 16-sample boundary groups, of the plain list or of the view)
    assert _one_list(engine, "32", 32e6, int(0.008 * 32e6), HALF, DOUBLED + 26 + 15 + WHOLE_CHIP_TAPS, (16, DOUBLED + 16), True, 1) == 192


def test_whole_chip_taps_direct_at_40_mhz(engine):
    assert _one_list(engine, "40", 40e6, int(0.008 * 40e6), HALF, DOUBLED + 26 + 19 + WHOLE_CHIP_TAPS, (DOUBLED + 26, DOUBLED + 26 + 19), True, 1) == 192


def test_five_taps_at_50_mhz(engine):
    five = (-1.0, -0.5, 0.0, 0.5, 1.0)
    assert _one_list(engine, "50", 50e6, int(0.008 * 50e6), five, DOUBLED + 26 + 24 + WHOLE_CHIP_TAPS, (DOUBLED + 26 + 24,), True, 2) == 192


@pytest.mark.parametrize("whole_chips", [1, 63, 64, 65, 130])
def test_short_epochs(engine, whole_chips):
    """Epochs of a partial first chip, `whole_chips` whole ones and a partial last chip: a wave's 64 lanes take a chip each per
    round."""
    sats, items, rf = _stream(engine)
    items = items[:64].copy()
    rng = np.random.default_rng(4100 + whole_chips)
    step = items["code_step"]
    rem = rng.uniform(0.2, 0.8, len(items))
    rem[:4] = [0.5, 0.25, 0.75, 0.5]
    n = np.ceil((whole_chips + 1.5 - (rem - np.floor(rem))) / step).astype(np.int64)
    items["rem_code"] = rem
    items["n_samples"] = n
    items["start_sample"] = items["start_sample"] + rng.integers(0, 20000, len(items))
    # the number of whole chips of the prompt tap, as the kernels count them: the chips strictly between the first and the last
    y_last = (n - 1) * step + rem
    assert np.all(np.ceil(y_last) - np.ceil(rem) - 1 == whole_chips)
    got = _run(engine, items, HALF, FS, STRAIGHT_25)
    ref = _oracle(("short", whole_chips), rf, sats, items, np.arange(len(items)), HALF, FS)
    dyn = _run(engine, items, HALF, FS, 26 + 24, no_split=True)
    err, err_dyn = _worst(got, ref, 1), _worst(got, dyn, 1)
    print(f"{whole_chips} whole chips: worst error against the oracle {err:.3g}, against the run-time-position kernel {err_dyn:.3g}")
    assert err <= RTOL and err_dyn <= RTOL
