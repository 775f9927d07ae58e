"""sdr_ddm on the MI355X against its statement (tests/ddm_cases.py: the oracle's EPL per segment, the second stage in
NumPy; the CPU file tests/test_ddm.py shows that the inputs are fair): parity of the segment sums, the map and the result
record, in the default form and with the per-sample form forced; determinism; the optional tables; what the peak means; a
NaN in the window; argument errors; the receiver's reacquisition."""
import numpy as np
import pytest

import ddm_cases as dc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import FMT_CF64, make_items

pytestmark = pytest.mark.gpu

NAMES = list(dc.parity_cases())
# the model's peak over second_value on the noise-only window is 1.0126 (tests/test_ddm.py asserts it): twice that
NOISE_RATIO_CAP = 2 * 1.0126


def stage(engine, case, empty_slots=0):
    engine.iq_alloc(case["capacity"], case["fmt"])
    engine.iq_upload(case["ring"], 0)
    engine.code_slots(max(2, len(case["codes"])) + empty_slots)
    for slot, prn in enumerate(case["prns"]):
        engine.load_gps_code(slot, prn)
    return make_items(*(np.array(col) for col in zip(*case["items"])))


def call(engine, case, items, **kw):
    return engine.ddm(items, case["fs"], case["B"], case["S"], case["first"], case["step"], case["T"], case["span"],
                      case["step_hz"], **kw)


def check_against_model(case, res, cmap, z, rows=None):
    models = dc.case_model(case)
    for i in (range(len(models)) if rows is None else rows):
        m, r = models[i], models[i]["result"]
        zmax = np.abs(m["z"]).max()
        bound = dc.CAP_MAP * case["B"] * (case["S"] * zmax) ** 2
        ez = np.abs(z[i] - m["z"]).max() / zmax
        em = np.abs(cmap[i] - m["map"]).max() / bound
        ev = max(abs(res[k][i] - r[k]) for k in ("peak_value", "second_value", "noise_mean")) / bound
        if i < 3:
            print(f"{case['name']} item {i}: |z error| / max|z| = {ez:.2e} (cap {dc.CAP_Z:.0e}); map error / bound = {em:.2e}; "
                  f"value error / bound = {ev:.2e}; peak ({res['peak_bin'][i]}, {res['peak_tap'][i]}) model "
                  f"({r['peak_bin']}, {r['peak_tap']})")
        assert ez <= dc.CAP_Z, (i, ez)
        assert em <= 1.0 and ev <= 1.0, (i, em, ev)
        assert (res["peak_bin"][i], res["peak_tap"][i]) == (r["peak_bin"], r["peak_tap"]), i
        assert res["peak_hz"][i] == r["peak_hz"] and res["peak_chips"][i] == r["peak_chips"], i


@pytest.mark.parametrize("name", NAMES)
def test_parity_against_the_model(engine, name):
    case = dc.parity_cases()[name]
    items = stage(engine, case)
    res, cmap, z = call(engine, case, items, want_segments=True)
    K = 2 * int(np.floor(case["span"] / case["step_hz"])) + 1
    assert cmap.shape == (len(items), K, case["T"]) and z.shape == (len(items), case["B"] * case["S"], case["T"])
    check_against_model(case, res, cmap, z)


@pytest.mark.parametrize("name", [n for n in NAMES if "10MHz" in n or "25MHz" in n])
def test_per_sample_form_agrees(engine, name):
    """The chip-run form's cases again with the per-sample form forced: both forms within the cap of the model (and so
    of each other)."""
    case = dc.parity_cases()[name]
    items = stage(engine, case)
    walk = call(engine, case, items, want_segments=True)
    engine.set_option("ddm_per_sample", 1)
    try:
        res, cmap, z = call(engine, case, items, want_segments=True)
    finally:
        engine.set_option("ddm_per_sample", 0)
    check_against_model(case, res, cmap, z)
    assert z.tobytes() != walk[2].tobytes()                      # (another summation order: the option took effect)
    zmax = np.abs(walk[2]).max(axis=(1, 2), keepdims=True)
    assert (np.abs(z - walk[2]) <= 2 * dc.CAP_Z * zmax).all()


@pytest.mark.parametrize("name", ["items_32_4MHz", "acq_10MHz_row0_B2_S8"])
def test_identical_calls_identical_bytes_and_the_tables_are_optional(engine, name):
    case = dc.parity_cases()[name]
    items = stage(engine, case)
    a = call(engine, case, items, want_segments=True)
    b = call(engine, case, items, want_segments=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    bare = call(engine, case, items, want_map=False, want_segments=False)
    assert bare[1] is None and bare[2] is None and bare[0].tobytes() == a[0].tobytes()


@pytest.mark.parametrize("fs", [4e6, 10e6])
def test_the_peak_is_the_satellite(engine, fs):
    """rem_code off by +1.5 chips, the coarse bin's carrier: rem_code + peak_chips is the true phase to a tap step, peak_hz
    the true Doppler to one grid step (12.5 Hz over 4 ms blocks), the peak at least 10 x what lies a chip or more away."""
    case = dc.parity_cases()[f"acq_{fs / 1e6:g}MHz_row0_B2_S8"]
    items = stage(engine, case)
    res, _, _ = call(engine, case, items)
    it, truth = case["items"][0], case["truth"]
    assert it[5] == 1.5
    assert abs(dc.wrap_chips(it[5] + res["peak_chips"][0] - truth["phase"])) <= case["step"]
    assert abs(res["peak_hz"][0] - truth["doppler"]) <= case["step_hz"]
    assert res["peak_value"][0] / res["second_value"][0] >= 10.0


def test_noise_alone_has_no_peak(engine):
    case = dc.noise_case()
    items = stage(engine, case)
    res, _, _ = call(engine, case, items)
    ratio = res["peak_value"][0] / res["second_value"][0]
    print(f"noise alone: peak / second = {ratio:.4f} (cap {NOISE_RATIO_CAP})")
    assert ratio < NOISE_RATIO_CAP < 3.0


def test_not_a_number_in_one_window_is_reported_for_that_item_only(engine):
    base = dc.parity_cases()["fmt_cf64_4MHz"]
    it = base["items"][0]
    N = orc.samples_per_code(4e6)
    other = (0, 2 * N + 9, it[2] + it[1] + 16, it[3], 0.4, 0.5, it[6])          # a window behind the first one
    case = dict(base, name="nan_cf64", items=[it, other])
    rf = case["rf"].copy()
    rf[it[2] + 1234] = np.nan
    items = stage(engine, case)
    engine.iq_upload(rf, 0)
    res, cmap, z = call(engine, case, items, want_segments=True)
    K = cmap.shape[1]
    assert not np.isfinite(cmap[0]).any()
    assert np.isnan(res["peak_value"][0]) and np.isnan(res["second_value"][0]) and np.isnan(res["noise_mean"][0])
    assert (res["peak_bin"][0], res["peak_tap"][0]) == ((K - 1) // 2, 0)
    assert res["peak_hz"][0] == it[3] and res["peak_chips"][0] == case["first"]
    check_against_model(case, res, cmap, z, rows=[1])


def test_argument_errors_leave_the_engine_usable(engine):
    case = dc.parity_cases()["acq_4MHz_row0_B2_S8"]
    items = stage(engine, case, empty_slots=1)
    assert engine.n_slots == 3
    good = call(engine, case, items)
    lib = _lib.load()
    INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6
    res = np.zeros(len(items), dtype=_lib.DDM_RESULT_DTYPE)
    untouched = res.tobytes()
    tab_map, tab_z = np.full((len(items), 41, 33), -7.5), np.full((len(items), 16, 33, 2), -7.5)     # what a good call would fill
    tables = tab_map.tobytes() + tab_z.tobytes()
    base = dict(fs=case["fs"], first_chips=-4.0, step_chips=0.25, span_hz=250.0, step_hz=12.5, n_taps=33, n_blocks=2, n_segments=8)

    def status_of(its=items, **fields):
        c = dict(base, **fields)
        cfg = _lib.DdmCfg(c["fs"], c["first_chips"], c["step_chips"], c["span_hz"], c["step_hz"], c["n_taps"], c["n_blocks"],
                          c["n_segments"], 0)
        its = np.ascontiguousarray(its)
        rc_ = lib.sdr_ddm(engine._h, _lib.ptr(its), len(its), _lib.C.byref(cfg), _lib.ptr(res), _lib.ptr(tab_map), _lib.ptr(tab_z))
        assert rc_ != 0 and lib.sdr_last_error()
        assert res.tobytes() == untouched and tab_map.tobytes() + tab_z.tobytes() == tables   # a refused call writes nothing
        return rc_

    def changed(**fields):
        its = items.copy()
        for k, v in fields.items():
            its[k][0] = v
        return its
    cfg = _lib.DdmCfg(case["fs"], -4.0, 0.25, 250.0, 12.5, 33, 2, 8, 0)
    assert lib.sdr_ddm(engine._h, None, 1, _lib.C.byref(cfg), _lib.ptr(res), None, None) == INVALID
    assert lib.sdr_ddm(engine._h, _lib.ptr(items), 1, None, _lib.ptr(res), None, None) == INVALID
    assert lib.sdr_ddm(engine._h, _lib.ptr(items), 1, _lib.C.byref(cfg), None, None, None) == INVALID
    assert lib.sdr_ddm(engine._h, _lib.ptr(items), 0, _lib.C.byref(cfg), _lib.ptr(res), None, None) == INVALID
    many = np.zeros(65536, dtype=items.dtype)                                        # more than 65 535 items in one call
    many[:] = items[0]
    assert lib.sdr_ddm(engine._h, _lib.ptr(many), 65536, _lib.C.byref(cfg), _lib.ptr(res), None, None) == INVALID
    assert res.tobytes() == untouched
    assert status_of(n_taps=0) == INVALID and status_of(n_taps=1025) == INVALID
    assert status_of(first_chips=np.nan) == INVALID and status_of(step_chips=np.inf) == INVALID
    assert status_of(fs=0.0) == INVALID and status_of(fs=-1.0) == INVALID and status_of(fs=np.inf) == INVALID
    assert status_of(step_hz=0.0) == INVALID and status_of(step_hz=-5.0) == INVALID and status_of(span_hz=-1.0) == INVALID
    assert status_of(step_hz=np.nan) == INVALID and status_of(span_hz=np.inf) == INVALID and status_of(step_hz=np.inf) == INVALID
    assert status_of(n_blocks=0) == INVALID and status_of(n_segments=0) == INVALID and status_of(n_segments=65) == INVALID
    assert status_of(n_segments=1) == INVALID                                       # K = 41 frequencies from one segment per block
    assert status_of(changed(code_slot=2)) == INVALID and status_of(changed(code_slot=3)) == INVALID
    assert status_of(changed(code_slot=-1)) == INVALID
    assert status_of(changed(n_samples=0)) == INVALID
    assert status_of(changed(code_step=0.0)) == INVALID and status_of(changed(code_step=np.nan)) == INVALID
    for field in ("rem_carrier", "carrier_hz", "rem_code"):
        for bad in (np.nan, np.inf):
            assert status_of(changed(**{field: bad})) == INVALID, (field, bad)
    assert status_of(span_hz=2050 * 12.5) == UNSUPPORTED                             # K = 4101
    assert status_of(n_blocks=65, n_segments=64) == UNSUPPORTED                      # Q = 4160
    assert status_of(changed(n_samples=15)) == UNSUPPORTED                           # Q = 16 > W
    assert status_of(first_chips=2.0 ** 30) == UNSUPPORTED and status_of(changed(rem_code=-2.0 ** 31)) == UNSUPPORTED
    assert status_of(changed(n_samples=case["capacity"] + 1)) == RANGE
    assert status_of(changed(start_sample=-1)) == RANGE
    from sydr_amd.engine import Engine
    fresh = Engine(engine.device_id)                       # neither ring nor code slots
    try:
        assert lib.sdr_ddm(fresh._h, _lib.ptr(items), 1, _lib.C.byref(cfg), _lib.ptr(res), None, None) == STATE
        fresh.iq_alloc(1024, FMT_CF64)
        assert lib.sdr_ddm(fresh._h, _lib.ptr(items), 1, _lib.C.byref(cfg), _lib.ptr(res), None, None) == STATE
        # (a code too long for the LDS cannot be staged: sdr_code_slots stops at 32 768 chips, which fit beside the tile)
    finally:
        fresh.close()
    assert res.tobytes() == untouched
    again = call(engine, case, items)
    assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes()


def test_ddm_scopes_are_recorded(engine):
    case = dc.parity_cases()["acq_10MHz_row0_B2_S8"]
    items = stage(engine, case)
    engine.prof_enable(True)
    try:
        engine.prof_reset()
        call(engine, case, items)
        for scope in ("ddm_items_upload", "ddm_segments_kernel", "ddm_map_kernel", "ddm_peak_kernel"):
            ms, launches = engine.prof_read(scope)
            assert launches == 1 and ms > 0.0, scope
        engine.prof_enable(True, calls_only=True)
        engine.prof_reset()
        call(engine, case, items)
        assert engine.prof_read("call_ddm")[1] == 1 and engine.prof_read("ddm_")[1] == 0
    finally:
        engine.prof_enable(False)


def test_function_level_delay_doppler_map():
    from sydr_amd.dsp.ddm import DelayDopplerMap
    case = dc.parity_cases()["acq_4MHz_row1_B1_S4"]
    it, m = case["items"][0], dc.case_model(case)[0]
    x = case["rf"][it[2]:it[2] + it[1]]
    phase, hz, cmap, rec = DelayDopplerMap(x, case["codes"][0], case["fs"], it[3], it[4], it[5], it[6], nbBlocks=1, nbSegments=4,
                                           frequencySpan=250.0, frequencyStep=12.5)
    assert cmap.shape == m["map"].shape and hz == m["result"]["peak_hz"] and phase == it[5] + m["result"]["peak_chips"]
    assert np.abs(cmap - m["map"]).max() <= dc.CAP_MAP * (4 * np.abs(m["z"]).max()) ** 2
    assert int(rec["peak_tap"]) == m["result"]["peak_tap"]


# ------------------------------------------------------------------------------------------------ the receiver
LOSS_FS, LOSS_SPMS, LOSS_TRACK_MS, LOSS_GAP_MS, LOSS_AFTER_MS = 4e6, 4000, 100, 30, 200
LOSS_DOPPLER = 1630.0


def _loss_stream():
    """A satellite for 100 ms, 30 ms of noise alone, the satellite again (its code, carrier and data running on)."""
    n_ms = LOSS_TRACK_MS + LOSS_GAP_MS + LOSS_AFTER_MS
    bits = np.random.default_rng(5).integers(0, 2, 40) * 2 - 1
    sat = dict(prn=7, doppler=LOSS_DOPPLER, code_phase=300.25, phase=0.3, amp=8.0, data=bits)
    raw = orc.synth_iq(LOSS_FS, n_ms * LOSS_SPMS, [sat], 20.0, 41).copy()
    lo, hi = 2 * LOSS_TRACK_MS * LOSS_SPMS, 2 * (LOSS_TRACK_MS + LOSS_GAP_MS) * LOSS_SPMS
    raw[lo:hi] = orc.synth_iq(LOSS_FS, LOSS_GAP_MS * LOSS_SPMS, [], 20.0, 42)
    cstep = orc.CODE_RATE * (1.0 + LOSS_DOPPLER / 1575.42e6) / LOSS_FS

    def data_bit(sample):        # the synthesised symbol of the code period that holds `sample`
        return bits[int(np.floor((300.25 + sample * cstep) / orc.CODE_CHIPS)) // orc.MS_PER_BIT]
    return raw, n_ms, data_bit


def _run_loss(engine, multi, reacquire):
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.utils.enumerations import ChannelMessage, ChannelState
    from test_host_layer import KAPLAN_INI, channel_config, rf_signal
    raw, n_ms, data_bit = _loss_stream()
    mgr = ChannelManager(rf_signal(LOSS_FS), engines=[engine]) if multi else ChannelManager(rf_signal(LOSS_FS), engine=engine)
    try:
        mgr.addChannel(ChannelL1CA_Kaplan, channel_config(KAPLAN_INI), 1)
        ch = mgr.requestTracking(7)
        rows, states, warm, reported = [], [], [], []
        for k in range(n_ms):
            if reacquire and k == LOSS_TRACK_MS + LOSS_GAP_MS + 2:
                assert ch.channelState is ChannelState.TRACKING
                mgr.reacquire(ch.channelID)
                assert ch.channelState is ChannelState.ACQUIRING
            mgr.addNewRFData(raw[2 * k * LOSS_SPMS:2 * (k + 1) * LOSS_SPMS])
            start = ch.currentSample
            p_track, flags = None, 0
            for p in mgr.run():
                if p["type"] is ChannelMessage.TRACKING_UPDATE:
                    p_track = p
                    rows.append((k, p["carrier_frequency"], p["i_prompt"], p["q_prompt"], p["i_early"], p["q_early"], p["i_late"],
                                 p["q_late"], data_bit(start + 2000)))
                elif p["type"] is ChannelMessage.ACQUISITION_UPDATE:
                    warm.append(p.get("warm_start", False))
                elif p["type"] is ChannelMessage.CHANNEL_UPDATE:
                    flags = int(p["tracking_flags"])
            # what the channel itself reports in this tick: the loop's lock state and indicators (TRACKING_UPDATE, when an
            # epoch ran) and the flags of its CHANNEL_UPDATE
            if p_track is not None:
                reported.append((k, int(p_track["lock_state"]), p_track["pll_lock"], p_track["fll_lock"], p_track["cn0"], flags))
            states.append(ch.channelState)
        return np.array(rows, dtype=np.float64), states, warm, np.array(reported, dtype=np.float64)
    finally:
        mgr.close()


def _locked_again(rows):
    """Carrier and code lock over the last 100 ms, with the navigation bits' signs as synthesised: the NCO carrier within
    25 Hz of the satellite's on average (the loop's own jitter on this signal is +-10 Hz; a false lock sits a multiple of
    500 Hz off), the prompt above early and late in at least 90 % of the epochs, and the in-phase prompt changing sign from one
    epoch to the next exactly where the synthesised symbols do in at least 95 % of the epochs (the signs themselves are
    the symbols' only up to a Costas loop's half-cycle ambiguity, which a frequency-assisted loop in pull-in may slip)."""
    tail = rows[rows[:, 0] >= LOSS_TRACK_MS + LOSS_GAP_MS + LOSS_AFTER_MS - 100]
    carrier = abs(tail[:, 1].mean() - LOSS_DOPPLER) <= 25.0
    prompt, early, late = np.hypot(tail[:, 2], tail[:, 3]), np.hypot(tail[:, 4], tail[:, 5]), np.hypot(tail[:, 6], tail[:, 7])
    code = np.mean((prompt > early) & (prompt > late)) >= 0.9
    agree = np.mean(np.sign(tail[1:, 2]) * np.sign(tail[:-1, 2]) == tail[1:, 8] * tail[:-1, 8])
    print(f"last 100 ms: carrier {tail[:, 1].mean():.1f} Hz, prompt on top in {np.mean((prompt > early) & (prompt > late)):.2f}, "
          f"sign changes as synthesised in {agree:.2f}")
    return bool(carrier and code and agree >= 0.95)


def _reports_lock(reported, since):
    """What the channel REPORTS behind tick `since`: -> (first tick with lock_state past PULL_IN, first tick with CODE_LOCK in
    tracking_flags), None where it never does.  The Kaplan loop leaves PULL_IN when its frequency-lock indicator (a slow
    average that a fresh loop state restarts at 0) passes fll_threshold_wide = 0.5, and sets CODE_LOCK in the epoch after,
    once C/N0 is over dll_threshold; its phase-lock indicator rises only from there on and does not reach
    pll_threshold_wide inside 200 ms -- neither behind a cold acquisition (the oracle's loops: 0.00 at 100 ms)."""
    from sydr_amd.utils.enumerations import LoopLockState, TrackingFlags
    tail = reported[reported[:, 0] >= since]
    state = tail[tail[:, 1] > int(LoopLockState.PULL_IN)]
    code = tail[(tail[:, 5].astype(np.int64) & int(TrackingFlags.CODE_LOCK)) != 0]
    last = tail[-1]
    print(f"reported behind tick {since}: lock_state past PULL_IN from tick {int(state[0, 0]) if len(state) else None}, CODE_LOCK "
          f"from tick {int(code[0, 0]) if len(code) else None}; at the end lock_state {int(last[1])}, pll_lock {last[2]:.2f}, "
          f"fll_lock {last[3]:.2f}, cn0 {last[4]:.1f}, flags {int(last[5])}")
    return (int(state[0, 0]) if len(state) else None, int(code[0, 0]) if len(code) else None)


@pytest.mark.parametrize("multi", [False, True], ids=["one_manager", "multi_device_manager"])
def test_reacquire_recovers_a_channel_that_lost_its_signal(engine, multi):
    """A channel tracks, the signal is gone for 30 ms (the loops run on noise: the NCO carrier wanders some hundred hertz),
    the signal returns.  With `reacquire` right behind the gap the channel goes through a warm acquisition -- no cold
    search -- and is locked again inside the 200 ms that follow; the same receiver without the call is not: its frequency
    loop settles on a side lobe of the 1 ms correlation, ~500 Hz off (the oracle's loops on the CPU show the same).
    "Locked again" is asked twice: of what the channel REPORTS -- `reacquire` zeroes the state row, the flags and the
    decoder, so lock_state must leave PULL_IN and CODE_LOCK must come back inside the 200 ms -- and of the signal itself
    (_locked_again).  The control without the call is held to the second only: its indicators DO report lock (lock_state
    WIDE_TRACK, CODE_LOCK and BIT_SYNC ~110 ms behind the gap) although it sits 500 Hz off -- C/N0 and the frequency-lock
    indicator of the Kaplan loop cannot tell a side lobe of the 1 ms correlation from the main lobe, which is what the map
    is for.  The figures are printed."""
    from sydr_amd.utils.enumerations import ChannelState
    behind = LOSS_TRACK_MS + LOSS_GAP_MS + 2                              # the tick `reacquire` is called in front of
    rows, states, warm, reported = _run_loss(engine, multi, reacquire=True)
    past_pull_in, code_lock = _reports_lock(reported, behind)
    assert past_pull_in is not None and past_pull_in < behind + LOSS_AFTER_MS
    assert code_lock is not None and code_lock < behind + LOSS_AFTER_MS
    assert warm == [False, True]                                          # the cold acquisition, then the warm one
    # (ACQUIRING is asserted right behind the call in _run_loss: the ring already holds the slab, so the warm search runs
    # in the same tick and the state read after it is TRACKING again)
    assert all(s is ChannelState.TRACKING for s in states[LOSS_TRACK_MS + LOSS_GAP_MS:])
    assert _locked_again(rows)
    if not multi:
        rows, states, warm, reported = _run_loss(engine, multi, reacquire=False)
        _reports_lock(reported, behind)                                   # (printed: see the docstring)
        assert warm == [False] and not _locked_again(rows)


MAP_SATS = [dict(prn=p, doppler=d, code_phase=c, phase=0.1 * k, amp=12.0)
            for k, (p, d, c) in enumerate(((7, 1750.0, 300.25), (12, -3000.0, 17.5), (19, 2380.0, 900.0), (27, -1113.0, 250.25)))]


def run_delay_doppler_maps(make_manager):
    """Four satellites tracked for 40 ms -> {channel: (result, map)} of delayDopplerMaps(4), after the checks every kind
    of manager and engine shares."""
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.utils.enumerations import ChannelState
    from test_host_layer import KAPLAN_INI, channel_config
    raw = orc.synth_iq(4e6, 60 * 4000, MAP_SATS, 20.0, 99)
    mgr = make_manager()
    try:
        mgr.addChannel(ChannelL1CA_Kaplan, channel_config(KAPLAN_INI), 5)
        chans = [mgr.requestTracking(s["prn"]) for s in MAP_SATS]
        assert mgr.delayDopplerMaps(4) == {}                             # nobody tracks yet: nothing raised, nothing returned
        for k in range(40):
            mgr.addNewRFData(raw[2 * k * 4000:2 * (k + 1) * 4000])
            mgr.run()
            if k == 3:
                assert mgr.delayDopplerMaps(4) == {}                     # tracking, but the ring does not hold 4 ms behind them yet
        assert all(ch.channelState is ChannelState.TRACKING for ch in chans)
        out = mgr.delayDopplerMaps(4)
        assert sorted(out) == [ch.channelID for ch in chans]
        for ch in chans:
            res, cmap = out[ch.channelID]
            item = ch.delayDopplerItem(4)
            assert cmap.shape == (21, 17) and item[1] == 16000
            print(f"channel {ch.channelID}: peak_chips {float(res['peak_chips']):+.2f}, bin {int(res['peak_bin']) - 10:+d}, "
                  f"peak / second {float(res['peak_value'] / res['second_value']):.1f}")
            assert abs(float(res["peak_chips"])) <= 0.25 and abs(int(res["peak_bin"]) - 10) <= 1
            assert float(res["peak_hz"]) == item[3] + (int(res["peak_bin"]) - 10) * 25.0
            assert float(res["peak_value"] / res["second_value"]) >= 10.0
        return out
    finally:
        mgr.close()


@pytest.mark.parametrize("multi", [False, True], ids=["one_manager", "multi_device_manager"])
def test_delay_doppler_maps_of_four_tracking_channels(engine, multi):
    from sydr_amd.channel.manager import ChannelManager
    from test_host_layer import rf_signal
    run_delay_doppler_maps(lambda: ChannelManager(rf_signal(4e6), engines=[engine]) if multi
                           else ChannelManager(rf_signal(4e6), engine=engine))
