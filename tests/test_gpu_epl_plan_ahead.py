"""A long list's setups (chip_setup_kernel) are made on a stream of their own and sdr_epl_plan_create returns once the list
has been checked: launches and fetches are ordered behind the setups by the plan's `ready` event, destroy waits for that plan
alone, and the engine-wide waits cover the setup stream.  None of that may change a bit of what a plan computes, how a bad
list is refused, or when the caller gets its memory back.

The lists are those of tests/test_gpu_epl_plan_stream.py: the 132 ms ring of seeded noise and the 4160 items of
tests/epl_epoch_cases.py, whose rows tests/golden/epl_epoch_moves.npz holds as the parent computed them
(`device_setups_4160`).  An item's row does not depend on its place in a list, so a slice of the list gives that slice of the
rows.  4096 items is the shortest list that takes the device path.  Every test makes its own engine."""
import ctypes

import numpy as np
import pytest

import bench
import epl_epoch_cases as cases
from conftest import load_golden
from sydr_amd._lib import EPL_ITEM_DTYPE, SdrError
from sydr_amd.engine import FMT_CI8, Engine

pytestmark = pytest.mark.gpu

SLICES = [slice(0, 4096), slice(0, 4128), slice(32, 4160), slice(0, 4160), slice(64, 4160)]


@pytest.fixture
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    g = load_golden("epl_epoch_moves.npz")
    return g["device_setups_4160"], int(g["device_setups_4160_variant"])


def _ring(eng):
    _, items, _, _ = cases._gps_ring(eng, "ring25", cases.FS, cases.TOTAL)
    assert len(items) == 4160
    return items


def _plan(eng, items):
    return eng.epl_plan(items, cases.HALF, cases.FS)


@pytest.mark.parametrize("n_items", [4096, 4160])
@pytest.mark.parametrize("on_created_stream", [True, False])
def test_run_right_behind_creation(eng, golden, n_items, on_created_stream):
    rows, variant = golden
    items = _ring(eng)[:n_items].copy()
    stream = eng.stream_create() if on_created_stream else 0
    plan = _plan(eng, items)
    try:
        plan.run(stream=stream)                             # at once: the setups may not have begun
        got = plan.fetch()
        assert plan.variant == variant
        assert got.tobytes() == rows[:n_items].tobytes()
    finally:
        eng.stream_sync(stream)
        plan.close()


@pytest.mark.parametrize("n_items", [4095, 4096, 4160])
def test_same_bits_with_epl_plan_wait(eng, golden, n_items):
    """4095 items: the host makes the setups, with and without the option."""
    rows, _ = golden
    items = _ring(eng)[:n_items].copy()
    got = {}
    for wait in (0, 1):
        eng.set_option("epl_plan_wait", wait)
        plan = _plan(eng, items)
        try:
            plan.run()
            got[wait] = (plan.variant, plan.fetch().tobytes())
        finally:
            plan.close()
    assert got[0] == got[1]
    if n_items >= 4096:
        assert got[0][1] == rows[:n_items].tobytes()


@pytest.mark.parametrize("memory", ["page-locked", "pageable"])
def test_callers_memory_is_free_on_return(eng, golden, memory):
    rows, _ = golden
    items = _ring(eng)
    if memory == "page-locked":
        mine = eng.host_alloc(len(items) * EPL_ITEM_DTYPE.itemsize, np.uint8).view(EPL_ITEM_DTYPE)
    else:
        mine = np.empty(len(items), dtype=EPL_ITEM_DTYPE)
    mine[:] = items
    plan = _plan(eng, mine)
    mine["start_sample"] = -1                               # the whole array: items the check would reject
    try:
        plan.run()
        assert plan.fetch().tobytes() == rows.tobytes()
    finally:
        plan.close()


def test_the_pipeline_the_headline_runs(eng, golden):
    """bench.py's pipelined_passes over five lists of four lengths, two passes: run(k) on the batch stream, the plan of k + 1,
    close(k - 1).  The lengths differ, so the pool hands a plan buffers that a plan of another size left."""
    rows, _ = golden
    items = _ring(eng)
    lists = [items[s].copy() for s in SLICES]
    batch = eng.stream_create()
    order = [(q, k) for q in range(2) for k in range(len(lists))]
    launched, kept = [], []
    plan = _plan(eng, lists[0])
    try:
        for i, (q, k) in enumerate(order):
            plan.run(stream=batch)
            launched.append((q, k, plan))
            if i + 1 < len(order):
                plan = _plan(eng, lists[order[i + 1][1]])
            while len(launched) > 1:
                oq, ok, old = launched.pop(0)
                if oq == 1:
                    kept.append((ok, old))
                else:
                    old.close()
        kept.append(launched.pop(0)[1:])
        assert sorted(k for k, _ in kept) == list(range(len(lists)))
        for k, p in kept:
            assert p.fetch().tobytes() == rows[SLICES[k]].tobytes(), SLICES[k]
    finally:
        eng.stream_sync(batch)
        for _, _, p in launched:
            p.close()
        for _, p in kept:
            p.close()


def test_destroy_with_setups_pending(eng):
    """Behind eight launches of a resident plan of 65 536 items the setups of a small plan wait for room: the plan is
    dropped without ever running, made again out of the same pool buffers, and computes what it computes on an idle device."""
    fs = cases.FS
    total = int(2.1 * fs) // 8 * 8
    sats = bench.satellites()
    eng.iq_alloc(total, FMT_CI8)
    eng.code_slots(len(sats))
    for s, sat in enumerate(sats):
        eng.load_gps_code(s, sat["prn"])
    eng.iq_synth(sats, fs, 12.0, 20270201, 0, total)
    items, n_epochs = bench.truth_items(sats, fs, total)
    assert n_epochs >= 2048
    small = items[:4160].copy()
    plan = _plan(eng, small)
    plan.run()
    idle_variant, idle = plan.variant, plan.fetch()
    plan.close()
    resident = _plan(eng, items[:65536].copy())
    batch, second = eng.stream_create(), eng.stream_create()
    try:
        for _ in range(8):
            resident.run(stream=batch)
        _plan(eng, small).close()                           # never run
        again = _plan(eng, small)
        try:
            again.run(stream=second)
            assert again.variant == idle_variant
            assert again.fetch().tobytes() == idle.tobytes()
        finally:
            eng.stream_sync(second)
            again.close()
    finally:
        eng.stream_sync(batch)
        resident.close()


def test_engine_wide_waits_cover_the_setup_stream(golden):
    """sdr_engine_sync, sdr_iq_alloc and the engine's destruction right behind a creation whose setups may still be queued.
    This can only show the absence of a crash or an error: nothing here can tell a wait that was made from one that was not
    needed."""
    rows, _ = golden
    eng = Engine(0)
    try:
        items = _ring(eng)
        plan = _plan(eng, items)
        eng.sync()
        plan.run()
        assert plan.fetch().tobytes() == rows.tobytes()
        plan.close()
        stale = _plan(eng, items)
        eng.iq_alloc(2 * cases.TOTAL, FMT_CI8)              # another size: the plan pool and the ring go
        with pytest.raises(SdrError):
            stale.run()
        stale.close()
        last = _plan(eng, items)                            # (fits the new ring; what the ring holds does not matter)
    finally:
        eng.close()                                         # with `last` alive and its setups perhaps pending
    # (the plan's four device buffers, 4 MB, outlive the engine until the process ends: a destroy needs the engine)
    last._h = ctypes.c_void_p()


def test_a_rejected_list_behind_a_pending_plan(eng, golden):
    rows, _ = golden
    items = _ring(eng)
    good = _plan(eng, items)                                # not run: its setups may be pending
    try:
        bad = items.copy()
        bad["start_sample"][3000] = -1
        with pytest.raises(SdrError) as info:
            _plan(eng, bad)
        assert "item 3000: negative start_sample" in str(info.value)
        good.run()
        assert good.fetch().tobytes() == rows.tobytes()
    finally:
        good.close()
