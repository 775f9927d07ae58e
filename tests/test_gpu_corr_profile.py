"""sdr_corr_profile on the MI355X against its NumPy statement (tests/corr_cases.py: the oracle's EPL on the tap grid; the CPU
file tests/test_corr_profile.py shows that the inputs are fair and that the run walk is exact): parity of every output within
1e-9 of the item's maximum, in the default form and with the per-sample form forced; the exact-phase trap; the library
against itself (sdr_epl_batch); determinism; the shape of a peak; the host layers end to end; ordering behind a queued
slab; argument errors."""
import numpy as np
import pytest

import corr_cases as cc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import FMT_CF64, FMT_CI8, make_items

pytestmark = pytest.mark.gpu

PARITY = [n for n in cc.parity_cases() if not n.startswith("exact_phase")]


def stage(engine, case, empty_slots=0):
    """The case's ring and codes on the device (+ `empty_slots` allocated slots nothing is loaded into) -> its items."""
    engine.iq_alloc(case["capacity"], case["fmt"])
    engine.iq_upload(case["ring"], 0)
    engine.code_slots(max(2, len(case["codes"])) + empty_slots, case["max_chips"], case["max_periods"])
    for slot, (prn, chips) in enumerate(zip(case["prns"], case["codes"])):
        if prn is None:
            engine.set_code(slot, chips)
        else:
            engine.load_gps_code(slot, prn)
    return make_items(*(np.array(col) for col in zip(*case["items"])))


def run_case(engine, case, per_sample):
    items = stage(engine, case)
    engine.set_option("corr_profile_per_sample", 1 if per_sample else 0)
    try:
        got = engine.corr_profile(items, case["first"], case["step"], case["n_taps"], case["fs"])
    finally:
        engine.set_option("corr_profile_per_sample", 0)
    assert got.shape == (len(items), case["n_taps"], 2)
    err = cc.worst_error(got, cc.case_model(case))
    print(f"{case['name']} ({'per-sample form' if per_sample else 'default form'}): worst |error| / item maximum = "
          f"{err.max():.2e} over {len(items)} items x {case['n_taps']} taps (cap {cc.CAP:.0e})")
    return err


@pytest.mark.parametrize("per_sample", [False, True], ids=["default", "per_sample"])
@pytest.mark.parametrize("name", PARITY)
def test_parity_against_the_model(engine, name, per_sample):
    err = run_case(engine, cc.parity_cases()[name], per_sample)
    assert (err <= cc.CAP).all(), err


@pytest.mark.parametrize("per_sample", [False, True], ids=["default", "per_sample"])
def test_exact_phase_case(engine, per_sample):
    """4.092 MHz, rem_code 0, dyadic spacings: code_step is exactly 1/4, so every fourth sample of most taps sits on a chip
    edge (ceil of a whole number: SURVEY H3)."""
    case = cc.parity_cases()["exact_phase_4.092MHz"]
    it = case["items"][0]
    y = np.linspace(it[5] + 0.25, it[6] * it[1] + it[5] + 0.25, it[1], endpoint=False)
    assert np.count_nonzero(y == np.floor(y)) > it[1] // 5
    err = run_case(engine, case, per_sample)
    assert (err <= cc.CAP).all(), err


@pytest.mark.parametrize("name", ["rate_25MHz_65", "rate_4MHz_65", "taps_129_10MHz", "grid_non_dyadic_16.368MHz"])
def test_profile_equals_epl_batch_in_chunks_of_eight(engine, name):
    case = cc.parity_cases()[name]
    items = stage(engine, case)
    got = engine.corr_profile(items, case["first"], case["step"], case["n_taps"], case["fs"])
    spacings = cc.grid(case["first"], case["step"], case["n_taps"])
    ref = np.concatenate([engine.epl_batch(items, spacings[k:k + 8], case["fs"]).reshape(len(items), -1, 2)
                          for k in range(0, case["n_taps"], 8)], axis=1)
    err = cc.worst_error(got, ref)
    print(f"{name}: profile against sdr_epl_batch in chunks of 8: worst |difference| / item maximum = {err.max():.2e}")
    assert (err <= cc.CAP).all(), err


@pytest.mark.parametrize("per_sample", [False, True], ids=["default", "per_sample"])
def test_two_identical_calls_return_identical_bytes(engine, per_sample):
    case = cc.parity_cases()["items_32_10MHz"]
    items = stage(engine, case)
    engine.set_option("corr_profile_per_sample", int(per_sample))
    try:
        a = engine.corr_profile(items, case["first"], case["step"], case["n_taps"], case["fs"])
        b = engine.corr_profile(items, case["first"], case["step"], case["n_taps"], case["fs"])
    finally:
        engine.set_option("corr_profile_per_sample", 0)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("fs", [4e6, 25e6])
def test_shape_of_a_strong_satellites_peak(engine, fs):
    """An aligned epoch of a strong satellite: |profile| peaks at the tap nearest 0 and is under 10 % of the peak beyond
    +-1 chip (the triangle of a C/A code and its sidelobes; the model gives 0.059 of the peak at 4 MHz, 0.056 at 25 MHz)."""
    prn, dop, phase = 7, 1750.0, 300.25
    N = orc.samples_per_code(fs)
    raw = orc.synth_iq(fs, 4 * N // 8 * 8, [dict(prn=prn, doppler=dop, code_phase=phase, phase=0.1, amp=40.0)], 10.0, 77)
    engine.iq_alloc(4 * N // 8 * 8, FMT_CI8)
    engine.iq_upload(raw, 0)
    engine.code_slots(2)
    engine.load_gps_code(0, prn)
    cstep = orc.CODE_RATE * (1.0 + dop / 1575.42e6) / fs
    start = int(np.ceil((orc.CODE_CHIPS - phase) / cstep))
    rem = phase + start * cstep - orc.CODE_CHIPS            # the satellite's code phase at `start`: the epoch is aligned
    n = orc.required_samples(rem, cstep)
    prof = engine.corr_profile(make_items(0, n, start, dop, 0.0, rem, cstep), -2.0, 1.0 / 16, 65, fs)[0]
    mag = np.hypot(prof[:, 0], prof[:, 1])
    s = cc.grid(-2.0, 1.0 / 16, 65)
    assert s[32] == 0.0 and int(mag.argmax()) == 32, int(mag.argmax())
    assert mag[np.abs(s) > 1.0].max() < 0.1 * mag.max()
    assert mag[np.abs(s) <= 0.5].min() > 0.4 * mag.max()


def test_manager_profiles_equal_the_last_epochs_correlators(engine):
    """A manager tracks two synthetic satellites for a block: correlationProfiles(-0.5, 0.5, 3) -- one library call -- is
    each channel's last record `corr` (E, P, L) again; correlationProfile raises before a channel's first epoch."""
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.channel.multidevice import MultiDeviceChannelManager
    from sydr_amd.utils.enumerations import ChannelState
    from test_host_layer import KAPLAN_INI, channel_config, rf_signal
    fs, spms = 4e6, 4000
    sats = [dict(prn=p, doppler=d, code_phase=c, phase=0.1, amp=8.0) for p, d, c in ((7, 1750.0, 300.25), (12, -3000.0, 17.5))]
    raw = orc.synth_iq(fs, 60 * spms, sats, 20.0, 99)
    for multi in (False, True):
        mgr = ChannelManager(rf_signal(fs), engines=[engine]) if multi else ChannelManager(rf_signal(fs), engine=engine)
        assert isinstance(mgr, MultiDeviceChannelManager) == multi
        try:
            mgr.addChannel(ChannelL1CA_Kaplan, channel_config(KAPLAN_INI), 3)
            chans = [mgr.requestTracking(s["prn"]) for s in sats]
            with pytest.raises(ValueError, match="no tracking epoch"):
                chans[0].correlationProfile(-0.5, 0.5, 3)
            assert mgr.correlationProfiles(-0.5, 0.5, 3) == {}
            k = 0
            while k < 20 or not all(ch.channelState is ChannelState.TRACKING for ch in chans):
                mgr.addNewRFData(raw[2 * k * spms:2 * (k + 1) * spms])
                mgr.run()
                k += 1
                assert k < 30
            for _ in range(20):                                   # a block: the ring filled ahead, one launch
                mgr.addNewRFData(raw[2 * k * spms:2 * (k + 1) * spms])
                k += 1
            assert len(mgr.runBlock(20)) > 0
            profiles = mgr.correlationProfiles(-0.5, 0.5, 3)
            assert sorted(profiles) == [ch.channelID for ch in chans]
            for ch in chans:
                last = np.array(ch.correlatorsResults[:6]).reshape(3, 2)
                peak = np.hypot(last[:, 0], last[:, 1]).max()
                err = np.abs(profiles[ch.channelID] - last).max() / peak
                one = ch.correlationProfile(-0.5, 0.5, 3)
                print(f"channel {ch.channelID}: profile against the last epoch's E, P, L: {err:.2e} of the maximum")
                assert err <= cc.CAP and one.tobytes() == profiles[ch.channelID].tobytes()
            wide = mgr.correlationProfiles(-2.0, 1.0 / 16, 65)
            for ch in chans:
                mag = np.hypot(wide[ch.channelID][:, 0], wide[ch.channelID][:, 1])
                assert abs(int(mag.argmax()) - 32) <= 5
        finally:
            mgr.close()


def test_profile_sees_the_slab_queued_right_before_it(engine):
    """A slab handed over with iq_upload_begin is in the ring for a profile of those samples made right after it."""
    case = cc.parity_cases()["rate_10MHz_65"]
    items = stage(engine, case)
    ref = cc.case_model(case)
    it = case["items"][0]
    lo = it[2] // 8 * 8
    count = (it[1] + 16) // 8 * 8
    engine.iq_upload(np.zeros(2 * count, dtype=np.int8), lo)           # the window wiped ...
    wiped = engine.corr_profile(items[:1], case["first"], case["step"], case["n_taps"], case["fs"])
    assert cc.worst_error(wiped, ref[:1]).max() > 0.5
    engine.iq_upload_begin(np.ascontiguousarray(case["ring"][2 * lo:2 * (lo + count)]), lo)    # ... and queued again
    got = engine.corr_profile(items[:1], case["first"], case["step"], case["n_taps"], case["fs"])
    assert (cc.worst_error(got, ref[:1]) <= cc.CAP).all()


def test_not_a_number_in_the_window_gives_non_finite_outputs_for_that_item_only(engine):
    case = cc.parity_cases()["fmt_cf64_4MHz"]
    rf = case["rf"].copy()
    it = case["items"][1]
    others = [k for k, o in enumerate(case["items"]) if o[2] + o[1] <= it[2] + 100 or o[2] >= it[2] + 200]
    rf[it[2] + 150] = np.nan
    assert others
    items = stage(engine, case)
    engine.iq_upload(rf, 0)
    got = engine.corr_profile(items, case["first"], case["step"], case["n_taps"], case["fs"])
    assert not np.isfinite(got[1]).any()
    ref = cc.case_model(case)
    assert (cc.worst_error(got[others], ref[others]) <= cc.CAP).all()


def test_argument_errors_leave_the_engine_usable(engine):
    case = cc.parity_cases()["rate_10MHz_65"]
    items = stage(engine, case, empty_slots=1)
    assert len(case["codes"]) == 2 and engine.n_slots == 3
    fs = case["fs"]
    good = engine.corr_profile(items, -2.0, 1.0 / 16, 65, fs)
    INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6

    def status_of(its=items, first=-2.0, step=1.0 / 16, n_taps=65, rate=fs):
        with pytest.raises(_lib.SdrError) as err:
            engine.corr_profile(its, first, step, n_taps, rate)
        assert str(err.value)
        return err.value.status

    def changed(**fields):
        its = items[:2].copy()
        for k, v in fields.items():
            its[k][1] = v
        return its
    assert status_of(n_taps=0) == INVALID and status_of(n_taps=1025) == INVALID
    assert status_of(first=np.nan) == INVALID and status_of(step=np.inf) == INVALID
    assert status_of(rate=0.0) == INVALID and status_of(rate=-1.0) == INVALID
    assert status_of(changed(code_slot=2)) == INVALID                             # allocated, nothing staged in it
    assert status_of(changed(code_slot=3)) == INVALID                             # beyond the allocated slots
    assert status_of(changed(code_slot=-1)) == INVALID
    assert status_of(changed(n_samples=0)) == INVALID
    assert status_of(changed(code_step=0.0)) == INVALID and status_of(changed(code_step=np.nan)) == INVALID
    assert status_of(changed(code_step=-0.04)) == INVALID and status_of(changed(code_step=np.inf)) == INVALID
    for field in ("rem_carrier", "carrier_hz", "rem_code"):
        for bad in (np.nan, np.inf, -np.inf):
            assert status_of(changed(**{field: bad})) == INVALID, (field, bad)
    assert status_of(changed(n_samples=case["capacity"] + 1)) == RANGE            # a window longer than the ring
    assert status_of(changed(start_sample=-1)) == RANGE
    assert status_of(first=2.0 ** 30) == UNSUPPORTED and status_of(changed(rem_code=-2.0 ** 31)) == UNSUPPORTED
    assert status_of(first=0.0, step=2.0 ** 21, n_taps=1024) == UNSUPPORTED
    lib = _lib.load()
    out = np.zeros((len(items), 65, 2))
    assert lib.sdr_corr_profile(engine._h, None, 1, -2.0, 1.0 / 16, 65, fs, _lib.ptr(out)) == INVALID
    assert lib.sdr_corr_profile(engine._h, _lib.ptr(items), len(items), -2.0, 1.0 / 16, 65, fs, None) == INVALID
    assert lib.sdr_corr_profile(engine._h, _lib.ptr(items), 0, -2.0, 1.0 / 16, 65, fs, _lib.ptr(out)) == INVALID
    assert lib.sdr_corr_profile(None, _lib.ptr(items), 1, -2.0, 1.0 / 16, 65, fs, _lib.ptr(out)) == INVALID
    from sydr_amd.engine import Engine
    fresh = Engine(engine.device_id)                       # neither ring nor code slots
    try:
        with pytest.raises(_lib.SdrError) as err:
            fresh.corr_profile(items, -2.0, 1.0 / 16, 65, fs)
        assert err.value.status == STATE
        fresh.iq_alloc(1024, FMT_CF64)
        with pytest.raises(_lib.SdrError) as err:
            fresh.corr_profile(items, -2.0, 1.0 / 16, 65, fs)
        assert err.value.status == STATE
    finally:
        fresh.close()
    # the largest grid the call accepts, and the engine is as it was
    assert engine.corr_profile(items[:1], -8.0, 1.0 / 64, 1024, fs).shape == (1, 1024, 2)
    assert engine.corr_profile(items, -2.0, 1.0 / 16, 65, fs).tobytes() == good.tobytes()


def test_profile_scopes_are_recorded(engine):
    case = cc.parity_cases()["rate_25MHz_65"]
    items = stage(engine, case)
    engine.prof_enable(True)
    try:
        engine.prof_reset()
        engine.corr_profile(items, -2.0, 1.0 / 16, 65, case["fs"])
        ms, launches = engine.prof_read("corr_walk_kernel")
        assert launches == 1 and ms > 0.0
        assert engine.prof_read("corr_items_upload")[1] == 1
        engine.prof_enable(True, calls_only=True)
        engine.prof_reset()
        engine.corr_profile(items, -2.0, 1.0 / 16, 65, case["fs"])
        assert engine.prof_read("call_corr_profile")[1] == 1 and engine.prof_read("corr_")[1] == 0
    finally:
        engine.prof_enable(False)


def test_function_level_correlation_profile():
    from sydr_amd.dsp.tracking import EPL, CorrelationProfile
    case = cc.parity_cases()["rate_4MHz_65"]
    it = case["items"][0]
    x = case["rf"][it[2]:it[2] + it[1]]
    code = orc.pad_code(case["codes"][it[0]])
    prof = CorrelationProfile(x, code, case["fs"], it[3], it[4], it[5], it[6], -2.0, 1.0 / 16, 65)
    assert prof.shape == (65, 2)
    assert (cc.worst_error(prof[None], cc.case_model(case)[:1]) <= cc.CAP).all()
    epl = np.array(EPL(x, code, case["fs"], it[3], it[4], it[5], it[6], (-0.5, 0.0, 0.5))).reshape(3, 2)
    assert np.abs(prof[[24, 32, 40]] - epl).max() <= cc.CAP * np.hypot(prof[:, 0], prof[:, 1]).max()
