"""sdr_serial_search, sdr_two_peak_compare_ss and sdr_code_upsample on the catalogue of tests/serial_cases.py, against the
oracle: sampling rates at which the chip index's rounding decides and chips get no sample or two, code lengths up to the
LDS limit, a code too short for its samples, sums of blocks, the ring's seam, many PRN entries, and the second-peak rule in
every corner and on maps of one to four rows.  Maps to 1e-9 of the reference's maximum (per added block), ratios to 1e-9
relative, peak indices exact, ratios the rule makes 1.0 exactly 1.0 (tests/test_serial_cases.py shows on the CPU that a
different index or a neighbouring rule would miss these by decades)."""
import numpy as np
import pytest

import serial_cases as sc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import FMT_CF64, FMT_CI8

pytestmark = pytest.mark.gpu

FS = 4e6
N = 4000
PRN = sc.SAT["prn"]


def _stage_ring(engine, raw, fmt=FMT_CI8, capacity=None):
    # (a ring holds a multiple of 8 samples: 1023 and 38192 * k are rounded up, what lies behind the samples is never read)
    engine.iq_alloc((len(raw) // 2 + 7) // 8 * 8 if capacity is None else capacity, fmt)
    engine.iq_upload(orc.iq_to_complex(raw) if fmt == FMT_CF64 else raw, 0)


def _check(got, k, ref, noncoh=1, what=""):
    """entry k of a search's (peak_bin, peak_code, peak_ratio, map) against the reference map"""
    pb, pc, pr, cmap = got
    peak, ratio = orc.two_peak_compare_ss(ref)
    err = float(np.max(np.abs(cmap[k] - ref)))
    print(f"{what}: map error {err / ref.max():.2e} of the maximum, peak {[int(pb[k]), int(pc[k])]} ratio {pr[k]:.9f} (oracle {ratio:.9f})")
    assert cmap[k].shape == ref.shape, what
    np.testing.assert_allclose(cmap[k], ref, rtol=0, atol=sc.map_atol(ref, noncoh), err_msg=what)
    assert [int(pb[k]), int(pc[k])] == peak, what
    assert pr[k] == pytest.approx(float(ratio), rel=1e-9), what
    return peak, pr[k]


def _bits(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got)


# ------------------------------------------------------------------------------------------------ 1. rates
@pytest.mark.parametrize("rate", sc.RATES, ids=sc.RATE_IDS)
def test_serial_search_at_rates_where_the_index_rounds(engine, rate):
    _stage_ring(engine, sc.samples(rate.fs))
    engine.code_slots(2)
    engine.load_gps_code(0, PRN)
    engine.load_gps_code(1, sc.ABSENT_PRN)
    got = engine.serial_search([0, 1], 0, rate.fs, *sc.GRID, want_map=True)
    assert got[3].shape == (2, 5, 1023)
    peak, _ = _check(got, 0, sc.ref_map(rate.fs, PRN), what=f"{rate.fs / 1e6:g} MHz PRN {PRN}")
    assert peak == sc.PEAK
    _check(got, 1, sc.ref_map(rate.fs, sc.ABSENT_PRN), what=f"{rate.fs / 1e6:g} MHz PRN {sc.ABSENT_PRN} (absent)")


# ------------------------------------------------------------------------------------------------ 2. the upsampler
@pytest.mark.parametrize("rate", sc.RATES, ids=sc.RATE_IDS)
def test_code_upsample_at_the_same_rates(engine, rate):
    engine.code_slots(2, 2046)
    engine.load_gps_code(0, 19)
    engine.set_code(1, sc.random_code(2046))
    index = orc.upsample_index(rate.fs)
    assert len(index) == rate.n
    assert np.array_equal(engine.upsample(0, rate.fs, rate.n), orc.gold_code(19).astype(np.int8)[index])
    assert np.array_equal(engine.upsample(1, rate.fs, rate.n), sc.random_code(2046)[index])


# ------------------------------------------------------------------------------------------------ 4. code lengths
@pytest.mark.parametrize("length", sc.LENGTHS)
def test_serial_search_code_lengths(engine, length):
    _stage_ring(engine, sc.samples(FS))
    engine.code_slots(1, 4096)
    engine.set_code(0, sc.random_code(length))
    for grid, bins in ((sc.ONE_BIN, 1), (sc.GRID, 5)):
        got = engine.serial_search([0], 0, FS, *grid, want_map=True)
        assert got[3].shape == (1, bins, length)
        _check(got, 0, sc.ref_map(FS, ("random", length), grid), what=f"{length} chips, {bins} bin(s)")


def test_serial_search_refuses_a_code_shorter_than_its_samples_reach(engine):
    """1022 chips: refused at 4 MHz, where sample 3999 lies on chip 1022 (the reference raises IndexError), without anything
    reaching the device; searched at 1.0 MHz, where the highest index is 1021."""
    engine.code_slots(1, 4096)
    engine.set_code(0, sc.random_code(sc.SHORT))
    _stage_ring(engine, sc.samples(FS))
    engine.prof_enable(True)
    engine.prof_reset()
    try:
        for want_map in (False, True):
            with pytest.raises(_lib.SdrError) as err:
                engine.serial_search([0], 0, FS, *sc.GRID, want_map=want_map)
            assert err.value.status == -1 and "1022" in str(err.value) and "1023" in str(err.value), str(err.value)
        assert engine.prof_read("ss_")[1] == 0 and engine.prof_read("")[1] == 0       # nothing was launched
    finally:
        engine.prof_enable(False)
        engine.prof_reset()
    _stage_ring(engine, sc.samples(1.0e6))
    got = engine.serial_search([0], 0, 1.0e6, *sc.GRID, want_map=True)
    _check(got, 0, sc.ref_map(1.0e6, ("random", sc.SHORT)), what="1022 chips at 1.0 MHz")


def test_serial_search_sizes_its_map_from_the_staged_code(engine):
    _stage_ring(engine, sc.samples(FS))
    engine.code_slots(1, 4096)
    engine.set_code(0, sc.random_code(2046))
    pb, pc, pr, cmap = engine.serial_search([0], 0, FS, *sc.GRID, want_map=True)
    assert cmap.shape == (1, 5, 2046)
    assert engine.serial_search([0], 0, FS, *sc.GRID, want_map=True, n_chips=2046)[3].shape == (1, 5, 2046)
    engine.prof_enable(True)
    engine.prof_reset()
    try:
        with pytest.raises(ValueError, match="1023"):
            engine.serial_search([0], 0, FS, *sc.GRID, want_map=True, n_chips=1023)
        assert engine.prof_read("ss_")[1] == 0                                      # refused before the search was called
    finally:
        engine.prof_enable(False)
        engine.prof_reset()


# ------------------------------------------------------------------------------------------------ 5. blocks, seam, many PRNs
@pytest.mark.parametrize("noncoh", sc.NONCOH)
def test_serial_search_adds_blocks_in_order(engine, noncoh):
    blocks = max(sc.NONCOH)
    _stage_ring(engine, sc.samples(FS, blocks))
    engine.code_slots(1)
    engine.load_gps_code(0, PRN)
    got = engine.serial_search([0], 0, FS, *sc.GRID, noncoh=noncoh, want_map=True)
    peak, _ = _check(got, 0, sc.ref_map(FS, PRN, sc.GRID, noncoh, blocks), noncoh, what=f"{noncoh} block(s)")
    assert peak == sc.PEAK


@pytest.mark.parametrize("fmt", [FMT_CI8, FMT_CF64], ids=["ci8", "cf64"])
def test_serial_search_across_the_ring_seam(engine, fmt):
    cap, start, noncoh = sc.SEAM["capacity"], sc.SEAM["start"], sc.SEAM["noncoh"]
    raw = sc.samples(FS, noncoh)
    engine.code_slots(2)
    engine.load_gps_code(0, PRN)
    engine.load_gps_code(1, sc.ABSENT_PRN)
    _stage_ring(engine, raw, fmt)
    flat = engine.serial_search([0, 1], 0, FS, *sc.GRID, noncoh=noncoh, want_map=True)
    # the same samples from an odd start, the second block across the ring's end, uploaded in two pieces
    first = cap - start
    assert N < first < 2 * N
    engine.iq_alloc(cap, fmt)
    pieces = (raw[:2 * first], raw[2 * first:])
    if fmt == FMT_CF64:
        pieces = tuple(orc.iq_to_complex(p) for p in pieces)
    engine.iq_upload(pieces[0], start)
    engine.iq_upload(pieces[1], 0)
    seam = engine.serial_search([0, 1], start, FS, *sc.GRID, noncoh=noncoh, want_map=True)
    assert _bits(seam) == _bits(flat)
    peak, _ = _check(seam, 0, sc.ref_map(FS, PRN, sc.GRID, noncoh), noncoh, what=f"seam, format {fmt}")
    assert peak == sc.PEAK
    _check(seam, 1, sc.ref_map(FS, sc.ABSENT_PRN, sc.GRID, noncoh), noncoh, what=f"seam, format {fmt}, absent PRN")


def test_serial_search_of_forty_entries(engine):
    prns, noncoh = sc.MANY["prns"], sc.MANY["noncoh"]
    entries = sc.many_entries()
    _stage_ring(engine, sc.samples(FS, noncoh))
    engine.code_slots(len(prns))
    for slot, prn in enumerate(prns):
        engine.load_gps_code(slot, prn)
    alone = [engine.serial_search([slot], 0, FS, *sc.GRID, noncoh=noncoh, want_map=True) for slot in range(len(prns))]
    got = engine.serial_search(entries, 0, FS, *sc.GRID, noncoh=noncoh, want_map=True)
    assert got[3].shape == (len(entries), 5, 1023)
    for i, slot in enumerate(entries):
        assert _bits(a[i:i + 1] for a in got) == _bits(alone[int(slot)]), (i, int(slot))
    for i in sc.MANY["oracle_entries"]:
        prn = prns[int(entries[i])]
        _check(got, i, sc.ref_map(FS, prn, sc.GRID, noncoh), noncoh, what=f"entry {i}, PRN {prn}")
    assert len({_bits(a) for a in alone}) == len(prns)


# ------------------------------------------------------------------------------------------------ 6. the peak rule
@pytest.mark.parametrize("doppler", list(sc.CORNER_DOPPLERS))
def test_second_peak_in_every_corner_through_the_search(engine, doppler):
    engine.code_slots(1)
    engine.load_gps_code(0, PRN)
    for phase, col in sc.CORNER_PHASES.items():
        _stage_ring(engine, sc.samples(FS, 1, doppler, phase))
        got = engine.serial_search([0], 0, FS, *sc.GRID, want_map=True)
        peak, ratio = _check(got, 0, sc.ref_map(FS, PRN, sc.GRID, 1, 1, doppler, phase), what=f"Doppler {doppler}, phase {phase}")
        assert peak == [sc.CORNER_DOPPLERS[doppler], col]
        if peak[0] == 0 or peak[1] == 0:
            assert ratio == 1.0
        else:
            assert sc.INTERIOR_RATIO[0] < ratio < sc.INTERIOR_RATIO[1]


@pytest.mark.parametrize("shape", sc.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_second_peak_on_small_maps(engine, shape):
    count = 0
    for m in sc.small_maps(shape):
        assert engine.two_peak_compare_ss(m) == orc.two_peak_compare_ss(m), (np.argwhere(m == sc.TOP), np.argwhere(m == sc.SECOND))
        count += 1
    assert count == shape[0] * shape[1] * (shape[0] * shape[1] - 1)


def test_second_peak_ties(engine):
    for name, m in sc.tie_maps():
        with np.errstate(invalid="ignore", divide="ignore"):
            peak, ratio = orc.two_peak_compare_ss(m)
        got_peak, got_ratio = engine.two_peak_compare_ss(m)
        first = np.unravel_index(int(np.argmax(m)), m.shape)
        assert got_peak == peak == [int(first[0]), int(first[1])], name
        if name == "all zero":
            assert got_peak == [0, 0] and np.isnan(ratio) and np.isnan(got_ratio)
        else:
            assert got_ratio == ratio, name
