"""sdr_acq_refine on the MI355X against its NumPy statement (tests/refine_cases.py; the CPU file tests/test_refine.py
shows that the inputs are fair): parity of segment sums, power table and indices; recovery of the true Doppler and the
data-bit edge; the reason for the feature end to end (the Borre plugin locks on an off-grid satellite); argument errors."""
import numpy as np
import pytest

import refine_cases as rc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI16, FMT_CI8, make_refine_items
from test_host_layer import BORRE_INI, channel_config
from test_refine import MARGIN, SINGLE_CASES, SPAN, STEP

pytestmark = pytest.mark.gpu


def check_parity(res, power, z, model, M, S, tag=""):
    """One item of a call against the model's (fine, h, k, P, z): the tolerances of the issue."""
    fine_m, h_m, k_m, P_m, z_m = model
    assert rc.margin(P_m) > MARGIN, tag                           # (the indices are then decided beyond rounding)
    zmax = np.abs(z_m).max()
    err_z = np.abs(z - z_m).max() / zmax
    bound_p = 4e-9 * (M * S * zmax) ** 2
    err_p = np.abs(power - P_m).max()
    print(f"{tag}: max|dz|/max|z| = {err_z:.2e} (cap 1e-9), max|dP| = {err_p:.3e} (cap {bound_p:.3e}), idx {res['fine_idx']},{res['bit_edge']}")
    assert err_z <= 1e-9, tag
    assert err_p <= bound_p, tag
    assert (int(res["fine_idx"]), int(res["bit_edge"])) == (k_m, h_m), tag
    assert res["fine_hz"] == fine_m and abs(res["power"] - P_m[h_m, k_m]) <= bound_p, tag
    assert abs(res["power_no_edge"] - P_m[0].max()) <= bound_p, tag


def stage(engine, raw, fmt=FMT_CI8, capacity=None, offset=0, n_slots=1, prns=(rc.PRN,)):
    n = raw.size if np.iscomplexobj(raw) else raw.size // 2
    engine.iq_alloc(capacity or (n + 7) // 8 * 8, fmt)
    engine.iq_upload(raw, offset)
    engine.code_slots(max(n_slots, len(prns)))
    for slot, prn in enumerate(prns):
        engine.load_gps_code(slot, prn)


@pytest.mark.parametrize("fs,M,S,row", SINGLE_CASES)
def test_parity_rates_and_shapes(engine, fs, M, S, row):
    c = rc.acquired(fs, *rc.SATELLITES[row])
    stage(engine, c["raw"])
    res, power, z = engine.acq_refine(make_refine_items(0, c["s0"], c["f0"]), fs, M, S, SPAN, STEP, want_tables=True)
    model = rc.refine_model(c["rf"], c["s0"], c["code"], fs, c["f0"], M, S, SPAN, STEP)
    check_parity(res[0], power[0], z[0], model, M, S, f"fs={fs / 1e6} M={M} S={S}")
    # two identical calls: identical bits
    res2, power2, z2 = engine.acq_refine(make_refine_items(0, c["s0"], c["f0"]), fs, M, S, SPAN, STEP, want_tables=True)
    assert res.tobytes() == res2.tobytes() and power.tobytes() == power2.tobytes() and z.tobytes() == z2.tobytes()
    # ... and the tables are optional
    assert engine.acq_refine(make_refine_items(0, c["s0"], c["f0"]), fs, M, S, SPAN, STEP).tobytes() == res.tobytes()


@pytest.mark.parametrize("fmt_name", ["ci16", "cf32", "cf64"])
def test_parity_other_ring_formats(engine, fmt_name):
    fs = 4e6
    if fmt_name == "ci16":
        c = rc.acquired(fs, *rc.SATELLITES[0], dtype=np.int16)
        stage(engine, c["raw"], FMT_CI16)
    else:
        c = rc.acquired(fs, *rc.SATELLITES[0])
        stage(engine, c["rf"], FMT_CF32 if fmt_name == "cf32" else FMT_CF64)      # (small integers: exact in float32)
    res, power, z = engine.acq_refine(make_refine_items(0, c["s0"], c["f0"]), fs, 10, 8, SPAN, STEP, want_tables=True)
    check_parity(res[0], power[0], z[0], rc.refine_model(c["rf"], c["s0"], c["code"], fs, c["f0"], 10, 8, SPAN, STEP), 10, 8, fmt_name)


@pytest.mark.parametrize("fmt", [FMT_CI8, FMT_CF64])
def test_parity_window_across_the_rings_end(engine, fmt):
    """The recording sits in the ring so that the window starts four and a half periods before the ring's end; the item's
    start_sample is given a whole turn of the ring too high (indices are taken modulo the capacity)."""
    fs = 4e6
    c = rc.acquired(fs, *rc.SATELLITES[1])
    cap = c["raw"].size // 2
    assert cap % 8 == 0
    offset = (cap - c["s0"] - 4 * c["N"] - c["N"] // 2) % cap
    stage(engine, c["raw"] if fmt == FMT_CI8 else c["rf"], fmt, capacity=cap, offset=offset)
    ring = np.roll(c["rf"], offset)
    s0 = (c["s0"] + offset) % cap
    assert s0 + 10 * c["N"] > cap > s0
    res, power, z = engine.acq_refine(make_refine_items(0, s0 + cap, c["f0"]), fs, 10, 8, SPAN, STEP, want_tables=True)
    check_parity(res[0], power[0], z[0], rc.refine_model(ring, s0, c["code"], fs, c["f0"], 10, 8, SPAN, STEP), 10, 8, "wrap")


def test_parity_32_items_in_one_call(engine):
    fs = 4e6
    raw, rf, items = rc.many_items(fs)
    stage(engine, raw, prns=[s["prn"] for s in rc.MANY_SATS])
    rec = make_refine_items([k for k, _, _ in items], [s for _, s, _ in items], [f for _, _, f in items])
    assert len(rec) == 32
    res, power, z = engine.acq_refine(rec, fs, 10, 8, SPAN, STEP, want_tables=True)
    for i, (k, s0, f0) in enumerate(items):
        model = rc.refine_model(rf, s0, orc.gold_code(rc.MANY_SATS[k]["prn"]), fs, f0, 10, 8, SPAN, STEP)
        check_parity(res[i], power[i], z[i], model, 10, 8, f"item {i}")
        assert abs(res[i]["fine_hz"] - rc.MANY_SATS[k]["doppler"]) <= STEP


def test_parity_4092_chip_code(engine):
    fs = 4e6
    raw, rf, code, s0, f0 = rc.long_code_case(fs)
    engine.iq_alloc(raw.size // 2, FMT_CI8)
    engine.iq_upload(raw, 0)
    engine.code_slots(2, 4092)
    engine.set_code(1, code.astype(np.int8))
    res, power, z = engine.acq_refine(make_refine_items(1, s0, f0), fs, 5, 8, SPAN, STEP, want_tables=True)
    check_parity(res[0], power[0], z[0], rc.refine_model(rf, s0, code, fs, f0, 5, 8, SPAN, STEP), 5, 8, "4092 chips")
    assert abs(res[0]["fine_hz"] - rc.LONG_DOPPLER) <= STEP and res[0]["bit_edge"] == 0


@pytest.mark.parametrize("fs", rc.RATES)
def test_recovers_true_doppler_and_bit_edge(engine, fs):
    for seed, dop, later in rc.RECOVERY:
        c = rc.acquired(fs, seed, dop, later)
        stage(engine, c["raw"])
        res = engine.acq_refine(make_refine_items(0, c["s0"], c["f0"]), fs, 10, 8, 150.0, STEP)[0]
        print(f"fs={fs / 1e6} true {dop}: coarse {c['f0']} fine {res['fine_hz']} edge {res['bit_edge']} (true {c['true_edge'](10)})")
        assert abs(res["fine_hz"] - dop) <= STEP
        assert res["bit_edge"] == c["true_edge"](10)
        assert res["power"] >= res["power_no_edge"]


def _borre_run(engine, tmp_path, seed, dop, fine_ms):
    """800 epochs of the Borre plugin on a 4 MHz recording file of one satellite -> (last carrier, IP, QP of every epoch)."""
    from sydr_amd.channel.l1ca_borre import ChannelL1CA
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.signal.iqsource import RFSignal
    from sydr_amd.utils.enumerations import ChannelMessage
    fs, spms, ms = 4e6, 4000, 830
    path = tmp_path / f"iq_{seed}.bin"
    if not path.exists():
        orc.synth_iq(fs, ms * spms, [dict(prn=rc.PRN, doppler=dop, code_phase=rc.CODE_PHASE, phase=0.3, amp=8.0,
                                          data=rc.ALTERNATING)], rc.SIGMA, seed).tofile(path)
    rf = RFSignal(dict(filepath=str(path), sampling_frequency=fs, is_complex="true", intermediate_frequency=0.0, data_size=8))
    cfg = channel_config(BORRE_INI)
    if fine_ms:
        cfg["ACQUISITION"]["fine_frequency_ms"] = str(fine_ms)
    mgr = ChannelManager(rf, engine=engine)
    try:
        mgr.addChannel(ChannelL1CA, cfg, 1)
        ch = mgr.requestTracking(rc.PRN)
        acq, trk = [], []
        for _ in range(ms):
            mgr.addNewRFData(rf.getMilliseconds(1))
            for p in mgr.run():
                if p["type"] is ChannelMessage.ACQUISITION_UPDATE:
                    acq.append(p)
                elif p["type"] is ChannelMessage.TRACKING_UPDATE and len(trk) < 800:
                    trk.append((p["carrier_frequency"], p["i_prompt"], p["q_prompt"]))
        assert len(acq) == 1 and len(trk) == 800
        return acq[0], np.array(trk)
    finally:
        mgr.close()


@pytest.mark.parametrize("seed,dop", [(1, 1630.0), (2, -2381.0), (4, 877.0)])
def test_borre_plugin_locks_with_the_fine_search_and_not_without(engine, tmp_path, seed, dop):
    """The reason for the feature.  With fine_frequency_ms = 10 the Costas loop starts within a grid step of the truth and
    locks (CPU oracle: mean|QP| / mean|IP| = 0.04); without the key it starts on the 250 Hz grid and never pulls in (the
    oracle ends ~130 Hz off)."""
    acq, trk = _borre_run(engine, tmp_path, seed, dop, 10)
    ip, qp = np.abs(trk[400:, 1]).mean(), np.abs(trk[400:, 2]).mean()
    print(f"true {dop}: refined start {acq['carrierFrequency']} (idx {acq['fine_frequency_idx']}, edge {acq['bit_edge']}), "
          f"carrier after 800 epochs {trk[-1, 0]:.1f}, mean|IP| {ip:.0f}, mean|QP| {qp:.0f}")
    assert abs(acq["carrierFrequency"] - dop) <= STEP and 0 <= acq["bit_edge"] < 10
    assert abs(trk[-1, 0] - dop) <= 5.0
    assert qp <= 0.2 * ip
    acq0, trk0 = _borre_run(engine, tmp_path, seed, dop, 0)
    print(f"true {dop}: coarse start {acq0['carrierFrequency']}, carrier after 800 epochs {trk0[-1, 0]:.1f}")
    assert "fine_frequency_idx" not in acq0 and "bit_edge" not in acq0
    assert abs(trk0[-1, 0] - dop) > 100.0


def test_manager_over_a_device_list_refines_its_own_channels(engine, tmp_path):
    """`ChannelManager(rfSignal, engines=[...])` is the manager of several devices (here: one): each device's part goes
    through the same acquisition, so two channels with the key set are refined in one call of their device."""
    from sydr_amd.channel.l1ca_borre import ChannelL1CA
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.channel.multidevice import MultiDeviceChannelManager
    from sydr_amd.utils.enumerations import ChannelMessage
    from test_host_layer import rf_signal
    fs, spms = 4e6, 4000
    sats = [dict(prn=p, doppler=d, code_phase=c, phase=0.2, amp=8.0, data=rc.ALTERNATING)
            for p, d, c in ((7, 1630.0, 300.25), (12, -2381.0, 17.5))]
    raw = orc.synth_iq(fs, 40 * spms, sats, rc.SIGMA, 31)
    cfg = channel_config(BORRE_INI)
    cfg["ACQUISITION"]["fine_frequency_ms"] = "10"
    mgr = ChannelManager(rf_signal(fs), engines=[engine])
    assert isinstance(mgr, MultiDeviceChannelManager)
    try:
        mgr.addChannel(ChannelL1CA, cfg, 2)
        for s in sats:
            mgr.requestTracking(s["prn"])
        acq = {}
        for k in range(40):
            mgr.addNewRFData(raw[2 * k * spms:2 * (k + 1) * spms])
            for p in mgr.run():
                if p["type"] is ChannelMessage.ACQUISITION_UPDATE:
                    acq[p["cid"]] = (k, p)
        assert sorted(acq) == [0, 1]
        for cid, s in enumerate(sats):
            tick, p = acq[cid]
            assert tick == 11 and abs(p["carrierFrequency"] - s["doppler"]) <= STEP and "bit_edge" in p, (cid, tick, p["carrierFrequency"])
    finally:
        mgr.close()


def test_not_a_number_in_the_window_is_reported_not_guessed(engine):
    fs = 4e6
    c = rc.acquired(fs, *rc.SATELLITES[0])
    rf = c["rf"].copy()
    rf[c["s0"] + 5 * c["N"] + 17] = np.nan
    stage(engine, rf, FMT_CF64)
    res = engine.acq_refine(make_refine_items(0, c["s0"], c["f0"]), fs, 10, 8, SPAN, STEP)[0]
    assert np.isnan(res["power"]) and np.isnan(res["power_no_edge"])
    assert res["fine_hz"] == c["f0"] and res["fine_idx"] == 50 and res["bit_edge"] == 0


def test_argument_errors_leave_the_engine_usable(engine):
    fs = 4e6
    c = rc.acquired(fs, *rc.SATELLITES[0])
    stage(engine, c["raw"], n_slots=4)
    item = make_refine_items(0, c["s0"], c["f0"])
    good = engine.acq_refine(item, fs, 10, 8, SPAN, STEP)
    INVALID, UNSUPPORTED, RANGE = -1, -4, -5
    for kwargs, status in ((dict(n_periods=0), INVALID), (dict(n_periods=21), INVALID), (dict(n_segments=0), INVALID),
                           (dict(n_segments=65), INVALID), (dict(step_hz=0.0), INVALID), (dict(span_hz=50000.0), UNSUPPORTED)):
        args = dict(n_periods=10, n_segments=8, span_hz=SPAN, step_hz=STEP)
        args.update(kwargs)
        with pytest.raises(_lib.SdrError) as err:
            engine.acq_refine(item, fs, **args)
        assert err.value.status == status and str(err.value), kwargs
    with pytest.raises(_lib.SdrError) as err:                    # S > N: 64 segments in a period of 40 samples
        engine.acq_refine(item, 40e3, 10, 64, SPAN, STEP)
    assert err.value.status == UNSUPPORTED
    with pytest.raises(_lib.SdrError) as err:                    # a slot nothing was staged in
        engine.acq_refine(make_refine_items(3, c["s0"], c["f0"]), fs, 10, 8, SPAN, STEP)
    assert err.value.status == INVALID and "not staged" in str(err.value)
    with pytest.raises(_lib.SdrError) as err:                    # a window longer than the ring
        engine.acq_refine(item, 40e6, 20, 8, SPAN, STEP)
    assert err.value.status == RANGE
    lib = _lib.load()
    rc_null = lib.sdr_acq_refine(engine._h, _lib.ptr(item), 1, fs, 10, 8, SPAN, STEP, None, None, None)
    assert rc_null == INVALID and b"results" in lib.sdr_last_error()
    res = np.zeros(1, dtype=_lib.REFINE_RESULT_DTYPE)
    assert lib.sdr_acq_refine(engine._h, None, 1, fs, 10, 8, SPAN, STEP, _lib.ptr(res), None, None) == INVALID
    assert engine.acq_refine(item, fs, 10, 8, SPAN, STEP).tobytes() == good.tobytes()      # the engine is as it was


def test_function_level_fine_frequency_search():
    from sydr_amd.dsp.acquisition import FineFrequencySearch
    fs = 4e6
    c = rc.acquired(fs, *rc.SATELLITES[2])
    fine, edge, power = FineFrequencySearch(c["rf"][c["s0"]:c["s0"] + 10 * c["N"]], c["code"], fs, c["f0"], 150.0, STEP)
    assert abs(fine - c["doppler"]) <= STEP and edge == c["true_edge"](10) and power.shape == (10, 61)
