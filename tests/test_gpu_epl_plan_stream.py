"""A long list's plan is checked and set up on the device (validate_items_kernel, chip_setup_kernel), in a segmented pass
beside the launch of the segment before.  validate_items_kernel serves one rule set per workgroup so that it fits there; that
may change neither which variant a plan gets, nor a bit of what it computes, nor how a bad list is refused.

25 MHz ci8, three taps half a chip apart, 32 channels: the headline's epl_kernel<0,3,26,24,1,12,0,0> row.  The lists are those
of tests/epl_epoch_cases.py (4160 items on a ring of seeded noise; tests/test_gpu_epl_epoch_moves.py holds the 4160 against the
parent's recorded bytes) and its prefixes of 4095 items -- the longest list the host still checks and sets up -- and 4096, the
shortest that goes to the device.  Every test makes its own engine."""
import numpy as np
import pytest

import bench
import epl_epoch_cases as cases
from conftest import load_golden
from sydr_amd._lib import SdrError
from sydr_amd.engine import FMT_CI8, Engine

pytestmark = pytest.mark.gpu

HEADLINE = "epl_kernel<0,3,26,24,1,12,0,0>"


@pytest.fixture
def eng():
    e = Engine(0)
    yield e
    e.close()


def _ring(eng):
    """The 132 ms ring of seeded noise, the 32 codes and the 4160 items of tests/epl_epoch_cases.py."""
    _, items, rf, codes = cases._gps_ring(eng, "ring25", cases.FS, cases.TOTAL)
    assert len(items) == 4160
    return items, rf, codes


def _make_run_fetch(eng, items):
    plan = eng.epl_plan(items, cases.HALF, cases.FS)
    try:
        plan.run()
        return plan.variant, plan.fetch()
    finally:
        plan.close()


def _error(items, got, rf, codes, which):
    case = cases.Case(got, 0, "", items, cases.HALF, cases.FS, rf, codes, np.asarray(which), 1, cases.TOTAL)
    return cases.worst_error(case)


@pytest.mark.parametrize("n_items", [4095, 4096, 4160])
def test_both_sides_of_the_long_list_threshold(eng, n_items):
    """The same variant on both sides, the first 64 rows against the oracle; the lists that go to the device (4096, 4160)
    are byte for byte the rows of the recorded 4160."""
    items, rf, codes = _ring(eng)
    items = items[:n_items].copy()
    variant, got = _make_run_fetch(eng, items)
    assert bench.kernel_of_variant(variant & 65535, 3) == HEADLINE, variant
    golden = load_golden("epl_epoch_moves.npz")
    assert variant == int(golden["device_setups_4160_variant"])
    err = _error(items, got, rf, codes, np.arange(64))
    print(f"{n_items} items: variant {variant}, worst error against the oracle over the first 64 rows {err:.3g}")
    assert err <= 1e-9
    if n_items >= 4096:
        assert got.tobytes() == golden["device_setups_4160"][:n_items].tobytes()


def test_created_beside_a_running_launch(eng):
    fs = cases.FS
    total = int(2.1 * fs) // 8 * 8                          # 2100 ms: 2098 whole epochs of 32 channels, 105 MB of ci8
    sats = bench.satellites()
    eng.iq_alloc(total, FMT_CI8)
    eng.code_slots(len(sats))
    for s, sat in enumerate(sats):
        eng.load_gps_code(s, sat["prn"])
    eng.iq_synth(sats, fs, 12.0, 20270201, 0, total)
    items, n_epochs = bench.truth_items(sats, fs, total)
    assert n_epochs >= 2048
    small = items[:4160].copy()
    idle_variant, idle = _make_run_fetch(eng, small)
    assert bench.kernel_of_variant(idle_variant & 65535, 3) == HEADLINE
    resident = eng.epl_plan(items[:65536].copy(), cases.HALF, fs)
    batch = eng.stream_create()
    try:
        for _ in range(8):
            resident.run(stream=batch)
        variant, got = _make_run_fetch(eng, small)          # while those are in flight
        eng.stream_sync(batch)
        assert variant == idle_variant
        assert got.tobytes() == idle.tobytes()
    finally:
        eng.stream_sync(batch)
        resident.close()


def test_the_statistics_of_both_rule_sets_reach_the_host(eng):
    """One item of 23.5 samples per chip among 4159 of 24.4 takes the whole list off the headline's row (the lowest and the
    highest block length are statistics of the list), and the rows still equal the oracle."""
    items, rf, codes = _ring(eng)
    items = items.copy()
    odd = 2000
    items["code_step"][odd] = 1.0 / 23.5
    items["n_samples"][odd] = 20000                         # (851 chips: inside the staged replica)
    variant, got = _make_run_fetch(eng, items)
    assert bench.kernel_of_variant(variant & 65535, 3) != HEADLINE, variant
    assert _error(items, got, rf, codes, np.concatenate([np.arange(64), [odd]])) <= 1e-9


def test_a_rejected_item_is_named_and_the_next_plan_works(eng):
    items, _, _ = _ring(eng)
    want = _make_run_fetch(eng, items)
    bad = items.copy()
    bad["start_sample"][3000] = -1
    bad["start_sample"][3500] = -1                          # (the lowest index is the one reported)
    with pytest.raises(SdrError) as info:
        eng.epl_plan(bad, cases.HALF, cases.FS)
    assert "item 3000: negative start_sample" in str(info.value)
    short = bad[2990:3010].copy()                           # the host's walk of a short list words it the same way
    with pytest.raises(SdrError) as info_short:
        eng.epl_plan(short, cases.HALF, cases.FS)
    assert info_short.value.status == info.value.status
    assert "item 10: negative start_sample" in str(info_short.value)
    variant, got = _make_run_fetch(eng, items)              # a correct plan right behind the failed ones
    assert variant == want[0] and got.tobytes() == want[1].tobytes()
