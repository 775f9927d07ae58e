"""sdr_pcps_signal on the device against its NumPy statement (sydr_amd/dsp/signalsearch.py): indices equal, maps within
1e-9 * map.max() (the bar of tests/test_gpu_pcps.py), ratios within 1e-9 relative -- three geometries (mixed radix with 11
and 31, a doubled BOC code, chirp-z), circular and zero-padded, one and three non-coherent blocks; the window across the
ring's end, with and without a map, the lags at and beyond one period, the C/A descriptor against Engine.pcps bit for bit,
the cached spectra across circular / padded / re-staged calls, every refusal, and a padded search that starts a closed loop."""
import ctypes as C

import numpy as np
import pytest

import signal_search_cases as sc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.dsp import signalsearch as ss
from sydr_amd.engine import FMT_CI8, Engine

pytestmark = pytest.mark.gpu

N_PRN, PERIODS = 2, 4
_SCENES, _STATEMENTS = {}, {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = sc.scene(name, N_PRN, PERIODS)
    return _SCENES[name]


def statement(name, pad, noncoh, coh=1):
    key = (name, pad, noncoh, coh)
    if key not in _STATEMENTS:
        raw, codes = scene(name)
        _STATEMENTS[key] = sc.statement(name, raw, codes, pad, noncoh, coh)
    return _STATEMENTS[key]


def stage(e, name, raw=None):
    fs, chips, rate, n_code, boc, excl = sc.GEOMETRIES[name]
    r, codes = scene(name)
    raw = r if raw is None else raw
    e.iq_alloc(raw.size // 2, FMT_CI8)
    e.iq_upload(raw, 0)
    e.code_slots(N_PRN + 1, chips)
    for p in range(N_PRN):
        e.set_code(p, codes[p])
    return codes


def search(e, name, pad, noncoh=1, coh=1, start=0, want_map=True, slots=None, **kw):
    fs, chips, rate, n_code, boc, excl = sc.GEOMETRIES[name]
    return e.pcps_signal(list(range(N_PRN)) if slots is None else slots, start, fs, 0.0, sc.RANGE, sc.STEP, rate, pad=pad,
                         excl_samples=kw.pop("excl", excl), coh=coh, noncoh=noncoh, want_map=want_map, n_chips=chips, **kw)


def held_to(got, want):
    pb, pc, pr, cmap = got
    rb, rc, rr, rmap = want
    assert cmap.shape == rmap.shape
    err = np.abs(cmap - rmap).max()
    print(f"map error {err / rmap.max():.3e} of the maximum; ratios {pr} against {rr}")
    assert err <= 1e-9 * rmap.max()
    assert np.array_equal(pb, rb) and np.array_equal(pc, rc)
    assert np.all(np.abs(pr - rr) <= 1e-9 * rr)


@pytest.mark.parametrize("pad,coh,noncoh", [(0, 1, 1), (0, 1, 3), (0, 2, 1), (0, 2, 2), (1, 1, 1), (1, 1, 3)])
@pytest.mark.parametrize("name", list(sc.GEOMETRIES))
def test_against_the_statement(engine, name, pad, coh, noncoh):
    stage(engine, name)
    got = search(engine, name, pad, noncoh, coh)
    held_to(got, statement(name, pad, noncoh, coh))
    if pad == 1:      # the point of it: the true bin and code sample of every PRN, with a flip at every period
        assert np.all(got[0] == sc.TRUE_BIN) and list(got[1]) == [sc.code_start(name, p) for p in range(N_PRN)]
    again = search(engine, name, pad, noncoh, coh)
    assert all(np.array_equal(u, v) for u, v in zip(got, again)), "two identical calls, other bits"


@pytest.mark.parametrize("name", ["a_16368", "c_2038"])
@pytest.mark.parametrize("pad,noncoh", [(0, 2), (1, 1), (1, 2)])
def test_window_across_the_rings_end(engine, name, pad, noncoh):
    """A window that crosses the ring's end == the same samples laid out flat (bit for bit), and the statement."""
    fs, chips, rate, n_code, boc, excl = sc.GEOMETRIES[name]
    raw, codes = scene(name)
    start = (PERIODS - 1) * n_code + 501
    stage(engine, name)
    wrapped = search(engine, name, pad, noncoh, start=start)
    x = raw.reshape(-1, 2)
    stage(engine, name, np.ascontiguousarray(np.roll(x, -start, axis=0)).reshape(-1))
    flat = search(engine, name, pad, noncoh)
    assert all(np.array_equal(u, v) for u, v in zip(wrapped, flat))
    held_to(wrapped, sc.statement(name, raw, codes, pad, noncoh, start=start))


@pytest.mark.parametrize("name", list(sc.GEOMETRIES))
@pytest.mark.parametrize("pad", [0, 1])
def test_with_and_without_a_map(engine, name, pad):
    stage(engine, name)
    pb, pc, pr, cmap = search(engine, name, pad)
    qb, qc, qr, none = search(engine, name, pad, want_map=False)
    assert none is None and np.array_equal(pb, qb) and np.array_equal(pc, qc)
    # (the padded search takes the map route either way; the circular one may run map-free: other additions, rounding apart)
    assert np.array_equal(pr, qr) if pad else np.all(np.abs(pr - qr) <= 1e-9 * pr)


@pytest.mark.parametrize("name", ["a_16368", "c_2038"])
def test_lags_at_and_beyond_one_period_stay_out(engine, name):
    """A noise-free signal whose only strong lag is N + 5 of the two-period transform: the N-column map neither shows that
    peak nor anything of its size, and is the statement's."""
    fs, chips, rate, n_code, boc, excl = sc.GEOMETRIES[name]
    codes = sc.codes_for(name, N_PRN)
    rep = ss.replica(codes[0].astype(np.float64), fs, rate, n_code)
    total = (2 * n_code + 7) // 8 * 8
    x = np.zeros(total, dtype=np.complex128)
    x[n_code + 5:2 * n_code] = 9.0 * rep[:n_code - 5]                 # the period that starts at lag N + 5, as far as the window goes
    raw = np.zeros(2 * total, dtype=np.int8)
    raw[0::2] = x.real
    stage(engine, name, raw)
    got = search(engine, name, 1)
    want = ss.pcps_signal_statement(x, codes, fs, 0.0, sc.RANGE, sc.STEP, rate, pad=1, excl_samples=excl)
    held_to(got, want)
    strong = 9.0 * (n_code - 5)                                       # what lag N + 5 holds at the bin of 0 Hz
    assert got[3].shape[2] == n_code and got[3].max() < 0.25 * strong
    # the circular search of the second period alone does see it, at lag 5: the signal is there
    pb, pc, pr, cmap = search(engine, name, 0, start=n_code, slots=[0])
    assert int(pc[0]) == 5 and cmap.max() > 0.9 * strong


@pytest.mark.parametrize("fs,want_map,coh,noncoh", [(4e6, True, 1, 1), (4e6, True, 2, 2), (10e6, False, 1, 1), (10e6, False, 1, 2)])
def test_ca_descriptor_is_engine_pcps(engine, fs, want_map, coh, noncoh):
    """{1.023e6, pad 0, excl 0} on 1023-chip slots: sdr_pcps's plan, route and bits."""
    n_code = orc.samples_per_code(fs)
    prns = (7, 19, 3)
    raw = orc.synth_iq(fs, 4 * n_code, [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=8.0),
                                        dict(prn=19, doppler=-2250.0, code_phase=811.5, phase=0.7, amp=7.0)], 20.0, 20260003)
    engine.iq_alloc(4 * n_code, FMT_CI8)
    engine.iq_upload(raw, 0)
    engine.code_slots(3)
    for s, p in enumerate(prns):
        engine.load_gps_code(s, p)
    for start in (0, 3 * n_code + 17 if coh * noncoh == 1 else 17):
        a = engine.pcps([0, 1, 2], start, fs, 0.0, 5000.0, 250.0, coh, noncoh, want_map=want_map)
        b = engine.pcps_signal([0, 1, 2], start, fs, 0.0, 5000.0, 250.0, 1.023e6, coh=coh, noncoh=noncoh, want_map=want_map,
                               n_chips=1023)
        for u, v in zip(a, b):
            assert (u is None and v is None) or np.array_equal(u, v)
    assert int(a[0][0]) == 13 and int(a[0][1]) == 29                   # PRN 7 at 1750 Hz, PRN 19 at -2250 Hz: found


# ------------------------------------------------------------------------------------------------ history: the cached spectra
def _stage_history(e):
    fs, n_code = 4e6, 4000
    raw = orc.synth_iq(fs, 4 * n_code, [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=8.0),
                                        dict(prn=19, doppler=-2250.0, code_phase=811.5, phase=0.7, amp=7.0)], 20.0, 20260004)
    e.iq_alloc(4 * n_code, FMT_CI8)
    e.iq_upload(raw, 0)
    e.code_slots(2)
    e.load_gps_code(0, 7)
    e.load_gps_code(1, 19)


_HISTORY_CALLS = {
    "pcps": lambda e: e.pcps([0, 1], 0, 4e6, 0.0, 5000.0, 250.0, 1, 2, want_map=True),
    "pad0": lambda e: e.pcps_signal([0, 1], 0, 4e6, 0.0, 5000.0, 250.0, 1.023e6, pad=0, noncoh=2, want_map=True, n_chips=1023),
    "pad1": lambda e: e.pcps_signal([0, 1], 0, 4e6, 0.0, 5000.0, 250.0, 1.023e6, pad=1, noncoh=2, want_map=True, n_chips=1023),
    # the same chips read at half the chip rate over the same N would be another replica: another chip rate alone
    "rate": lambda e: e.pcps_signal([0, 1], 0, 4e6, 0.0, 5000.0, 250.0, 1.023e6 * (1 + 1e-6), pad=0, noncoh=2, want_map=True,
                                    n_chips=1023),
}


def _bytes(out):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in out if a is not None)


def test_history_circular_padded_restaged():
    """pcps, pcps_signal pad 0, pad 1, pad 0, pcps on the same slots and fs, one slot re-staged in between: each call's bits
    are a fresh engine's (the cached spectra's key holds the chip rate and the padding)."""
    fresh = {}
    for name, call in _HISTORY_CALLS.items():
        e = Engine(0)
        try:
            _stage_history(e)
            fresh[name] = _bytes(call(e))
        finally:
            e.close()
    assert fresh["pcps"] == fresh["pad0"] and fresh["pad0"] != fresh["pad1"]
    e = Engine(0)
    try:
        _stage_history(e)
        for step in ["pcps", "pad0", "pad1", "pad0", "pcps", "rate", "pad0", "restage", "pad1", "pad0", "restage", "pcps", "pad1", "rate"]:
            if step == "restage":
                e.load_gps_code(1, 19)                                 # the same chips, another stamp
                continue
            assert _bytes(_HISTORY_CALLS[step](e)) == fresh[step], step
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_change_nothing(engine):
    name = "c_2038"
    fs, chips, rate, n_code, boc, excl = sc.GEOMETRIES[name]
    raw, codes = scene(name)
    stage(engine, name)
    engine.code_slots(4, 4092)
    for p in range(N_PRN):
        engine.set_code(p, codes[p])
    engine.set_code(2, np.ones(4092, dtype=np.int8))                  # another length; slot 3 stays empty
    before = search(engine, name, 1, 2)
    INVALID, UNSUPPORTED, RANGE = -1, -4, -5
    base = dict(code_slots=[0, 1], start_sample=0, fs=fs, if_hz=0.0, doppler_range=sc.RANGE, doppler_step=sc.STEP, chip_rate_hz=rate,
                pad=1, excl_samples=0, coh=1, noncoh=2, want_map=False, n_chips=chips)
    nan, inf = float("nan"), float("inf")
    cases = [(INVALID, dict(chip_rate_hz=v)) for v in (nan, inf, -inf, 0.0, -1.023e6)]
    cases += [(INVALID, dict(pad=2)), (INVALID, dict(pad=-1)), (INVALID, dict(excl_samples=-1)),
              (INVALID, dict(reserved=(1, 0))), (INVALID, dict(reserved=(0, 7))), (INVALID, dict(coh=2)),
              (INVALID, dict(code_slots=[0, 2])), (INVALID, dict(excl_samples=n_code // 2)), (INVALID, dict(excl_samples=(n_code - 1) // 2 + 1)),
              # sdr_pcps's own causes
              (INVALID, dict(code_slots=[])), (INVALID, dict(fs=0.0)), (INVALID, dict(fs=nan)), (INVALID, dict(noncoh=0)),
              (INVALID, dict(pad=0, coh=0)), (INVALID, dict(doppler_step=0.0)), (INVALID, dict(doppler_range=-1.0)),
              (INVALID, dict(code_slots=[0, 3])), (INVALID, dict(code_slots=[0, 4])), (INVALID, dict(code_slots=[-1])),
              (UNSUPPORTED, dict(chip_rate_hz=1.0)),                                   # N = fs * 1023: far above 2^24
              (UNSUPPORTED, dict(chip_rate_hz=rate * n_code / 9e6)),                   # N = 9e6, T = 18e6 > 2^24
              (UNSUPPORTED, dict(chip_rate_hz=1e12)),                                  # N = 0
              (UNSUPPORTED, dict(doppler_range=40000.0, doppler_step=1.0)),            # 80001 bins
              (RANGE, dict(pad=0, chip_rate_hz=rate * n_code / 9e6)),                  # the same N circular: longer than the ring
              (RANGE, dict(noncoh=PERIODS)), (RANGE, dict(pad=0, noncoh=PERIODS + 1)), (RANGE, dict(pad=0, coh=2, noncoh=3)),
              (RANGE, dict(start_sample=-1))]
    for status, change in cases:
        with pytest.raises(_lib.SdrError) as err:
            engine.pcps_signal(**{**base, **change})
        assert err.value.status == status, (change, err.value)
    # the largest windows that fit are served
    engine.pcps_signal(**{**base, "noncoh": PERIODS - 1})
    engine.pcps_signal(**{**base, "pad": 0, "noncoh": PERIODS})
    # NULL descriptor, NULL outputs
    slots = np.array([0, 1], dtype=np.int32)
    out = [np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2)]
    sig = _lib.AcqSignal(rate, 1, 0, (C.c_int32 * 2)(0, 0))
    tail = (2, 0, fs, 0.0, sc.RANGE, sc.STEP, 1, 2)
    lib = engine._lib
    assert lib.sdr_pcps_signal(engine._h, None, slots.ctypes.data, *tail, *(a.ctypes.data for a in out), None, None, None) == INVALID
    assert lib.sdr_pcps_signal(engine._h, C.byref(sig), None, *tail, *(a.ctypes.data for a in out), None, None, None) == INVALID
    assert lib.sdr_pcps_signal(engine._h, C.byref(sig), slots.ctypes.data, *tail, None, out[1].ctypes.data, out[2].ctypes.data, None,
                               None, None) == INVALID
    nb, nc = C.c_int(0), C.c_int(0)
    assert lib.sdr_pcps_signal(engine._h, C.byref(sig), slots.ctypes.data, *tail, *(a.ctypes.data for a in out), None, C.byref(nb),
                               C.byref(nc)) == 0 and (nb.value, nc.value) == (9, n_code)
    # nothing changed: the ring, and the spectra of the last good search are still the cached ones (no code transform runs)
    search(engine, name, 1, 2)
    with pytest.raises(_lib.SdrError):
        engine.pcps_signal(**{**base, "pad": 2})
    assert np.array_equal(engine.iq_download(raw.size // 2, 0), raw)
    engine.prof_enable(True)
    try:
        engine.prof_reset()
        after = search(engine, name, 1, 2)
        assert engine.prof_read("pcps_code_fft")[1] == 0 and engine.prof_read("pcps_upsample")[1] == 0
        assert engine.prof_read("pcps_inv_fft")[1] == 2 and engine.prof_read("pcps_fwd_fft")[1] == 2       # sdr_pcps's inner scopes
        engine.prof_enable(True, calls_only=True)
        engine.prof_reset()
        assert all(np.array_equal(u, v) for u, v in zip(after, search(engine, name, 1, 2)))
        assert engine.prof_read("call_pcps_signal")[1] == 1 and engine.prof_read("call_")[1] == 1           # its own scope, once
    finally:
        engine.prof_enable(False)
    assert all(np.array_equal(u, v) for u, v in zip(before, after))


def test_function_level_call(engine):
    """dsp.signalsearch.PCPSSignal: one code over complex samples, in the shape of dsp.acquisition.PCPS."""
    name = "c_2038"
    fs, chips, rate, n_code, boc, excl = sc.GEOMETRIES[name]
    raw, codes = scene(name)
    cmap, peak, ratio = ss.PCPSSignal(sc.to_complex(raw), 0.0, fs, codes[0], rate, sc.RANGE, sc.STEP, pad=1, nonCoherentIntegration=2)
    rb, rc, rr, rmap = ss.pcps_signal_statement(sc.to_complex(raw), codes[:1], fs, 0.0, sc.RANGE, sc.STEP, rate, pad=1, noncoh=2)
    assert peak == [int(rb[0]), int(rc[0])] and abs(ratio - rr[0]) <= 1e-9 * rr[0]
    assert np.abs(cmap - rmap[0]).max() <= 1e-9 * rmap.max()


# ------------------------------------------------------------------------------------------------ end to end
def test_padded_search_starts_the_closed_loop(engine):
    """sdr_iq_synth writes a 4092-chip slot code with a BOC(1,1) sub-carrier at 4.092 MHz (its data sign changes every code
    period), Doppler on the grid, code start on a whole sample; the padded search with the doubled code returns both, and the
    closed loop started from them completes and ends in the lock state of the loop started from the truth."""
    import test_gpu_multignss as mg
    fs, epochs, n_code = 4.092e6, 40, 16368
    n = (epochs + 3) * n_code // 8 * 8
    rng = np.random.default_rng(20261020)
    code = np.where(rng.random(4092) < 0.5, -1, 1).astype(np.int8)
    dop, first = 500.0, 8221                                            # the code period starts at sample 8221
    cstep = 1.023e6 * (1.0 + dop / 1575.42e6) / fs
    cp0 = 4092.0 - first * cstep
    engine.iq_alloc(n, FMT_CI8)
    engine.code_slots(2, 8184)
    engine.set_code(0, code)
    engine.set_code(1, ss.boc_doubled(code).astype(np.int8))
    engine.iq_synth([dict(slot=0, boc=True, doppler=dop, code_phase=cp0, phase=0.1, amp=7.0)], fs, 14.0, 4043, 0, n)
    pb, pc, pr, _ = engine.pcps_signal([1], 0, fs, 0.0, 1000.0, 250.0, 2.046e6, pad=1, excl_samples=4, noncoh=2)
    bins = np.arange(-1000.0, 1001.0, 250.0)
    doppler = -bins[int(pb[0])]                                         # postAcquisitionUpdate's sign
    assert doppler == dop and int(pc[0]) == first and pr[0] > 2.5
    c = mg.KAPLAN_4MS
    wide, narrow = mg.FIVE, tuple(0.5 * s for s in mg.FIVE)
    cfg = mg.general_cfg(1, fs, c, wide, narrow, 8184.0, 1, 4e-3)
    ends = []
    for carrier0, start in ((doppler, int(pc[0])), (dop, first)):
        states, traj, bits, done = engine.track_closed_loop_ex([mg.general_state(1, fs, 1, carrier0, start, 2.046e6, 8184.0, c)], cfg,
                                                               epochs, want_bits=True, epochs_per_bit=1)
        assert done[0] == epochs
        ends.append((int(traj[0]["lock_state"][-1]), float(traj[0]["carrier_hz"][-1])))
    print(f"final carrier from the search {ends[0][1]:.6f} Hz, from the truth {ends[1][1]:.6f} Hz, difference {ends[0][1] - ends[1][1]:.3e}")
    assert ends[0][0] == ends[1][0]
