"""The order in which the workgroups of an E/P/L launch take its items ("epl_xcd_run": runs of R consecutive items per XCD,
sydr_amd/csrc/xcd_order.h; tests/test_xcd_order_map.py holds the map itself on the CPU) on the GPU: it permutes which
workgroup computes which item and nothing else, so every case runs one plan with the library's default run length and with
epl_xcd_run = 0 (the linear order) and asks for the same BYTES, and for the plan's variant -- the kernel that took the map.

Headline form (25 MHz, 32 channels, taps half a chip either side, the straight-line kernel): lists of 8R - 1, 8R, 8R + 1,
3 * 8R - 1 and 4160 items -- under a tile, one tile, a tile and a partial one, two tiles and a partial one, eight tiles
and a partial one; ranges of one plan (first = 37, count = 8R + 5; then the rest of the list; the 37 items in front) against
the whole list in one launch; the first 64 items of the 4160-item list against the oracle at 1e-9 of max(|prompt|, 1).
One list each for the other kernels that take the map: 10 MHz (two chips per lane: epl2_kernel), 20 MHz (block length 19),
a ci16 ring at 25 MHz (16-sample groups), five taps at 50 MHz with four waves per workgroup (item counts that are no multiple
of 4 * 32: 192 -- a launch shorter than a tile -- and 2080).

A destroyed plan's output buffer serves the next plan of its size, results and all: every list here is one no other plan
has run (its carriers are moved by an offset of its own) and runs in the new order FIRST, so no row of that fetch can be
a left-over of the right answer.  Streams, items and helpers are those of tests/test_gpu_epl_fold.py."""
import numpy as np
import pytest

import bench
from sydr_amd.engine import FMT_CI8, FMT_CI16
from test_gpu_epl_fold import FS, HALF, N_LONG, RTOL, STRAIGHT_25, TOTAL, _oracle, _stream, _worst

pytestmark = pytest.mark.gpu

R = 64                      # the library's default run length (engine_internal.h: kEplXcdRunDefault)
TILE = 8 * R
DOUBLED, WHOLE_CHIP_TAPS, TWO_CHIPS = 65536, 4096, 8192


def _fetch(engine, items, spacing, fs, want_variant, xcd_run, ranges=None):
    engine.set_option("epl_xcd_run", xcd_run)
    try:
        plan = engine.epl_plan(items, spacing, fs)
        try:
            assert plan.variant == want_variant, plan.variant
            if ranges is None:
                plan.run()
            else:
                for first, count in ranges:
                    plan.run(first, count)
            return plan.fetch()
        finally:
            plan.close()
    finally:
        engine.set_option("epl_xcd_run", -1)        # the default


def _moved(items, hz):
    """`items` with every carrier moved by `hz`: a list no other plan has run."""
    items = items.copy()
    items["carrier_hz"] = items["carrier_hz"] + hz
    return items


def _both_orders(engine, items, spacing, fs, want_variant):
    new = _fetch(engine, items, spacing, fs, want_variant, -1)
    linear = _fetch(engine, items, spacing, fs, want_variant, 0)
    assert new.shape == (len(items), 2 * len(spacing))
    assert new.tobytes() == linear.tobytes()
    return new


@pytest.mark.parametrize("n_items", [TILE - 1, TILE, TILE + 1, 3 * TILE - 1])
def test_headline_lists_around_a_tile(engine, n_items):
    _, items, _ = _stream(engine)
    _both_orders(engine, _moved(items[:n_items], 10.0 + n_items), HALF, FS, STRAIGHT_25)


def test_headline_list_of_4160_items_and_the_oracle(engine):
    sats, items, rf = _stream(engine)
    assert len(items) == N_LONG
    items = _moved(items, 7.0)
    got = _both_orders(engine, items, HALF, FS, STRAIGHT_25)
    which = np.arange(64)
    ref = _oracle("xcd order, 4160", rf, sats, items, which, HALF, FS)
    err = _worst(got[which], ref, 1)
    print(f"first 64 of 4160 items in the new order: worst error against the oracle {err:.3g}")
    assert err <= RTOL


def test_ranges_of_a_plan_equal_one_launch(engine):
    """The map works on a range's own ids: [37, 37 + 8R + 5) is one tile and a partial one, the range behind it seven
    tiles and a partial one, the 37 items in front less than a tile."""
    _, items, _ = _stream(engine)
    items = _moved(items, -13.0)
    cut = 37 + TILE + 5
    parts = _fetch(engine, items, HALF, FS, STRAIGHT_25, -1, ranges=[(37, TILE + 5), (cut, N_LONG - cut), (0, 37)])
    whole = _fetch(engine, items, HALF, FS, STRAIGHT_25, 0)
    assert parts[37:].tobytes() == whole[37:].tobytes()        # the two ranges from item 37 on
    assert parts.tobytes() == whole.tobytes()


def test_two_chips_per_lane_at_10_mhz(engine):
    fs = 10e6
    _, items, _ = _stream(engine, fs, int(0.022 * fs))
    assert len(items) == 640 and TILE < 640 < 2 * TILE          # a tile and a partial one
    _both_orders(engine, _moved(items, 3.0), HALF, fs, 8 + TWO_CHIPS)


def test_block_length_19_at_20_mhz(engine):
    fs = 20e6
    _, items, _ = _stream(engine, fs, int(0.020 * fs))
    assert len(items) == 576 and TILE < 576 < 2 * TILE          # a tile and a partial one
    _both_orders(engine, _moved(items, 3.0), HALF, fs, 26 + 19 + 256 * 9)


def test_ci16_ring_at_25_mhz(engine):
    _, items, _ = _stream(engine)
    engine.iq_alloc(TOTAL, FMT_CI16)
    try:
        engine.iq_upload(np.random.default_rng(20261201).integers(-2000, 2000, 2 * TOTAL).astype(np.int16), 0)
        _both_orders(engine, _moved(items[:3 * TILE + 77], 3.0), HALF, FS, 16)
    finally:
        engine.iq_alloc(TOTAL, FMT_CI8)


@pytest.mark.parametrize("n_epochs", [6, 65])
def test_five_taps_at_50_mhz_four_waves_per_workgroup(engine, n_epochs):
    """Epochs of two code periods: their replica on the half-chip view is 4108 words, long enough (4096) for the workgroups
    of four waves -- four epochs of a channel around one staged table, 32 columns per group.  192 items launch 64 workgroups
    -- less than a tile, the linear order --, 2080 items 544 -- a tile and a partial one; neither count is a multiple of
    4 * 32."""
    fs, total = 50e6, int((2 * n_epochs + 2) * 1e-3 * 50e6)
    five = (-1.0, -0.5, 0.0, 0.5, 1.0)
    sats = bench.satellites()
    engine.iq_alloc(total, FMT_CI8)
    engine.code_slots(len(sats), 1023, 3)
    for s, sat in enumerate(sats):
        engine.load_gps_code(s, sat["prn"])
    engine.iq_synth(sats, fs, 12.0, 20260003, 0, total)
    every, _ = bench.truth_items(sats, fs, total)
    every = every.reshape(2 * n_epochs, len(sats))
    items = every[0::2].copy()
    items["n_samples"] += every[1::2]["n_samples"]            # every other epoch, as long as it and the one behind it
    items = items.reshape(-1)
    assert len(items) == 32 * n_epochs and len(items) % 128 != 0
    assert np.all(np.ceil(items["code_step"] * items["n_samples"] + items["rem_code"] + 1.0) == 2048)   # 2 * (2048 + 6) words
    _both_orders(engine, _moved(items, 3.0), five, fs, DOUBLED + 26 + 24 + WHOLE_CHIP_TAPS)
