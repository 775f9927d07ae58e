"""sdr_acq_deep_detect on the MI355X.  The yardstick of the peaks and the noise figures is the statement
(sydr_amd/dsp/deepsearch.py: deep_detect) applied to the corr_map THE SAME CALL returned: indices and values are then exact
and near-ties between NumPy's map and the device's play no part (the map itself is held to NumPy by test_gpu_deep.py).  mean
and variance are held to math.fsum of the same cells within (n_cells + 4) * 2^-53, the bound of a fixed-order fp64 sum of
non-negative terms; nothing here is tuned."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as tc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import Engine
from test_host_layer import KAPLAN_INI, channel_config

pytestmark = pytest.mark.gpu

INVALID = -1


def _stage(engine, name):
    c, image, cap = tc.gpu_input(name)
    engine.iq_alloc(cap, c["fmt"])
    engine.iq_upload(image, 0)
    engine.code_slots(max(2, len(c["prns"])))
    for s, p in enumerate(c["prns"]):
        engine.load_gps_code(s, int(p))
    return c


def _detect(engine, c, slots, want_map=True, **over):
    a = dict(c)
    a.update(over)
    return engine.acq_deep_detect(slots, 0, a["fs"], a["if_hz"], a["R"], a["S"], a["C"], a["K"], a["G"], a["rf"], a["n_peaks"],
                                  a["excl_code"], a["excl_bins"], want_map=want_map)


def _hold(tag, c, res, peaks, noise, cmap):
    """One call's figures of every PRN against the statement on the map the call returned."""
    N = cmap.shape[3]
    for k in range(len(res)):
        want, _ = tc.deep_detect(cmap[k], c["n_peaks"], c["excl_code"], c["excl_bins"])
        got = [(int(p["group"]), int(p["bin"]), int(p["code"]), float(p["value"])) for p in peaks[k]]
        assert got == [(w["group"], w["bin"], w["code"], w["value"]) for w in want], tag
        assert (got[0][0], got[0][1], got[0][2], got[0][3]) == (int(res[k]["peak_group"]), int(res[k]["peak_bin"]),
                                                                int(res[k]["peak_code"]), float(res[k]["peak_value"]))
        for p in peaks[k]:
            end = (int(p["code"]) + tc_shift(c, int(p["bin"]), N)) % N
            assert int(p["code_end"]) == end and int(p["reserved"]) == 0
            assert float(p["z"]) == tc.host_z(p["value"], noise[k]["mean"], noise[k]["variance"])
        columns = tc.noise_columns(peaks[k], N, c["excl_code"])
        mean, var = float(noise[k]["mean"]), float(noise[k]["variance"])
        n_cells, total, squares = tc.exact_moments(cmap[k], columns, mean)
        bound = tc.moment_bound(n_cells)
        err_mean, err_var = abs(mean - total / n_cells) / (total / n_cells), abs(var - squares / n_cells) / (squares / n_cells)
        print(f"{tag} PRN {k}: peaks {[(g[1], g[2]) for g in got]} n_cells {n_cells} mean {mean:.6g} (off {err_mean:.2e}) variance "
              f"{var:.6g} (off {err_var:.2e}), bound {bound:.2e}; z {[round(float(p['z']), 2) for p in peaks[k]]}")
        assert int(noise[k]["n_cells"]) == n_cells
        assert err_mean <= bound and err_var <= bound


def tc_shift(c, b, N):
    from sydr_amd.dsp.deepsearch import deep_shift
    return deep_shift(c["R"], c["S"], N, c["C"], c["rf"], b, c["K"])


@pytest.mark.parametrize("name", sorted(tc.GPU_CASES))
def test_figures_are_the_statements_on_the_returned_map(engine, name):
    c = _stage(engine, name)
    slots = np.arange(len(c["prns"]))
    ref, ref_map = engine.acq_deep(slots, 0, c["fs"], c["if_hz"], c["R"], c["S"], c["C"], c["K"], c["G"], c["rf"], want_map=True)
    res, peaks, noise, cmap = _detect(engine, c, slots)
    assert res.tobytes() == ref.tobytes() and cmap.tobytes() == ref_map.tobytes()
    assert peaks.shape == (len(slots), c["n_peaks"])
    _hold(name, c, res, peaks, noise, cmap)
    N = cmap.shape[3]
    if "edges" in name:       # the zones wrap at n = 0 / N - 1 and clip at bin 0 / the last bin
        assert [(int(r["peak_bin"]), int(r["peak_code"])) for r in res] == [(0, 1), (cmap.shape[2] - 1, N - 2)]
    if "one_row" in name:
        assert cmap.shape[1:3] == (1, 1)


def test_carrier_compensation_moves_code_end_of_every_peak(engine):
    c = _stage(engine, "cf64_edges_wrap_and_clip")
    res, peaks, noise, cmap = _detect(engine, c, np.arange(2), rf=1e6, n_peaks=3)
    c = dict(c, rf=1e6, n_peaks=3)
    _hold("rf", c, res, peaks, noise, cmap)
    assert any(int(p["code_end"]) != int(p["code"]) for p in peaks.ravel())


@pytest.mark.parametrize("name", ["ci8_two_prns_8_peaks", "cf64_odd_4001"])
def test_two_calls_return_the_same_bits_and_a_prn_depends_on_its_own_map(engine, name):
    """(N = 4001, 3 rows: PRN 1's map starts on an odd element in the two-PRN call and on an even one alone)"""
    c = _stage(engine, name)
    a = _detect(engine, c, np.arange(2))
    b = _detect(engine, c, np.arange(2))
    nomap = _detect(engine, c, np.arange(2), want_map=False)
    for x, y, z in zip(a, b, nomap[:3]):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert a[3].tobytes() == b[3].tobytes() and nomap[3] is None
    for k in range(2):
        res, peaks, noise, cmap = _detect(engine, c, [k])
        assert cmap[0].tobytes() == a[3][k].tobytes()              # the same map rows ...
        assert peaks[0].tobytes() == a[1][k].tobytes() and noise[0].tobytes() == a[2][k].tobytes()      # ... the same figures
        assert res[0].tobytes() == a[0][k].tobytes()


def test_refusals_touch_nothing_and_the_search_alone_keeps_its_scopes(engine):
    c = _stage(engine, "ci8_two_prns_8_peaks")
    good = _detect(engine, c, np.arange(2))
    lib = _lib.load()
    slots = np.arange(2, dtype=np.int32)
    res = np.full(2, 7, dtype=_lib.DEEP_RESULT_DTYPE)
    peaks = np.full((2, 8), 7, dtype=_lib.DETECT_PEAK_DTYPE)
    noise = np.full(2, 7, dtype=_lib.DETECT_NOISE_DTYPE)
    untouched = (res.tobytes(), peaks.tobytes(), noise.tobytes())

    def call(det_null=False, peaks_p=_lib.ptr(peaks), noise_p=_lib.ptr(noise), n_peaks=8, excl_code=4, excl_bins=1, reserved=0,
             **over):
        a = dict(fs=c["fs"], if_hz=0.0, R=c["R"], S=c["S"], rf=0.0, C=c["C"], K=c["K"], G=c["G"])
        a.update(over)
        cfg = _lib.DeepCfg(a["fs"], a["if_hz"], a["R"], a["S"], a["rf"], a["C"], a["K"], a["G"], 0)
        det = _lib.DetectCfg(n_peaks, excl_code, excl_bins, reserved)
        return lib.sdr_acq_deep_detect(engine._h, _lib.ptr(slots), 2, 0, C.byref(cfg), None if det_null else C.byref(det),
                                       _lib.ptr(res), peaks_p, noise_p, None)

    engine.prof_enable(True)
    engine.prof_reset()
    try:
        for kwargs in (dict(det_null=True), dict(peaks_p=None), dict(noise_p=None), dict(n_peaks=0), dict(n_peaks=9),
                       dict(excl_code=-1), dict(excl_bins=-1), dict(reserved=1), dict(n_peaks=8, excl_code=250),
                       dict(n_peaks=1, excl_code=2000), dict(C=0), dict(G=3), dict(S=0.0)):
            assert call(**kwargs) == INVALID and lib.sdr_last_error(), kwargs
        assert call(n_peaks=8, excl_code=250) == INVALID and b"noise cell" in lib.sdr_last_error()     # 8 x 501 >= 4000
        assert engine.prof_read("")[1] == 0                             # no kernel, no scope: nothing reached the device
        assert call(n_peaks=8, excl_code=249) == 0                      # 8 x 499 < 4000: the largest window that fits
        assert engine.prof_read("")[1] > 0
    finally:
        engine.prof_enable(False)
        engine.prof_reset()
    res[:], peaks[:], noise[:] = 7, 7, 7
    for kwargs in (dict(n_peaks=9), dict(n_peaks=8, excl_code=250)):
        assert call(**kwargs) == INVALID
    assert (res.tobytes(), peaks.tobytes(), noise.tobytes()) == untouched
    again = _detect(engine, c, np.arange(2))                            # the engine is as it was
    for x, y in zip(good, again):
        assert x.tobytes() == y.tobytes()

    names = ("deep_fold", "deep_fwd_fft", "deep_inv_fft", "deep_shift_acc", "deep_peak", "deep_detect_peaks", "deep_detect_noise",
             "call_acq_deep", "call_acq_deep_detect")

    def counts(e, run):
        out = {}
        for calls_only in (False, True):
            e.prof_enable(True, calls_only=calls_only)
            e.prof_reset()
            try:
                run(e)
                out[calls_only] = {s: e.prof_read(s)[1] for s in names}
            finally:
                e.prof_enable(False)
                e.prof_reset()
        return out

    def search(e):
        e.acq_deep(np.arange(2), 0, c["fs"], c["if_hz"], c["R"], c["S"], c["C"], c["K"], c["G"], c["rf"])

    after_detect = counts(engine, search)
    detect = counts(engine, lambda e: _detect(e, c, np.arange(2), want_map=False))
    fresh = Engine(0)
    try:
        _, image, cap = tc.gpu_input("ci8_two_prns_8_peaks")
        fresh.iq_alloc(cap, c["fmt"])
        fresh.iq_upload(image, 0)
        fresh.code_slots(2)
        for s, p in enumerate(c["prns"]):
            fresh.load_gps_code(s, int(p))
        search(fresh)                                                    # (the code spectra are cached from here on, as above)
        on_fresh = counts(fresh, search)
    finally:
        fresh.close()
    assert after_detect == on_fresh
    assert after_detect[False]["deep_detect_peaks"] == after_detect[False]["deep_detect_noise"] == 0
    assert after_detect[True]["call_acq_deep_detect"] == 0 and after_detect[True]["call_acq_deep"] == 1
    assert (detect[False]["deep_detect_peaks"], detect[False]["deep_detect_noise"], detect[False]["deep_peak"]) == (1, 1, 1)
    assert detect[True]["call_acq_deep_detect"] == 1


def test_function_level_detect():
    from sydr_amd.dsp.deepsearch import DeepDetect
    c, image, _ = tc.gpu_input("cf64_two_prns_8_peaks")
    n = orc.samples_per_code(c["fs"])
    win = np.asarray(image[:c["C"] * c["K"] * n])
    peaks, noise, cmap = DeepDetect(win, c["if_hz"], c["fs"], orc.gold_code(c["prns"][0]), c["R"], c["S"], n, c["C"], c["K"], c["G"],
                                    c["rf"], n_peaks=3, excl_code=4, excl_bins=1, want_map=True)
    want, _ = tc.deep_detect(cmap, 3, 4, 1)
    assert [(p["group"], p["bin"], p["code"], p["value"]) for p in peaks] == [(w["group"], w["bin"], w["code"], w["value"]) for w in want]
    assert noise["n_cells"] == int(tc.noise_columns(peaks, n, 4).sum()) * cmap.shape[0] * cmap.shape[1]
    assert [p["z"] for p in peaks] == [tc.host_z(p["value"], noise["mean"], noise["variance"]) for p in peaks]


# ------------------------------------------------------------------------------------------------ through the channel manager
class _Spy:
    """The engine's search calls counted (patched on the instance, taken off again on exit)."""

    def __init__(self, engine):
        self._e, self.calls = engine, {"pcps": [], "acq_deep": [], "acq_deep_detect": []}

    def __enter__(self):
        for name, log in self.calls.items():
            def wrapped(*a, _name=name, _log=log, **k):
                _log.append((a, k))
                return getattr(type(self._e), _name)(self._e, *a, **k)
            setattr(self._e, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name in self.calls:
            delattr(self._e, name)


def _run(engine, extra, raw, ms, prns):
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.signal.iqsource import RFSignal
    from sydr_amd.utils.enumerations import ChannelMessage
    cfg = channel_config(KAPLAN_INI)
    cfg["ACQUISITION"].update(dict(doppler_range="500", doppler_steps="100", coherent_integration="5",
                                   non_coherent_integration="40", threshold="1.5"))
    cfg["ACQUISITION"].update(extra)
    rf = RFSignal(dict(filepath="none", sampling_frequency=4e6, is_complex="true", intermediate_frequency=0.0, data_size=16))
    mgr = ChannelManager(rf, engine=engine, ring_ms=300)
    try:
        mgr.addChannel(ChannelL1CA_Kaplan, cfg, len(prns))
        chans = [mgr.requestTracking(p) for p in prns]
        acq, trk = {}, {ch.channelID: 0 for ch in chans}
        with _Spy(engine) as spy:
            for k in range(ms):
                mgr.addNewRFData(raw[2 * k * 4000:2 * (k + 1) * 4000])
                for p in mgr.run():
                    if p["type"] is ChannelMessage.ACQUISITION_UPDATE:
                        acq[p["cid"]] = p
                    elif p["type"] is ChannelMessage.TRACKING_UPDATE:
                        trk[p["cid"]] += 1
        return spy, [ch.channelState for ch in chans], acq, trk, mgr.acquisitionDetections(), [ch.acq_threshold for ch in chans]
    finally:
        mgr.close()


TAIL_MS = 6         # milliseconds fed behind the 200 ms search window: the first tracking epochs
WEAK_SEED = 5       # ratio 1.389 and z_0 10.15 on the quantised stream (seeds 1 and 3: 1.478 / 11.53 and 1.460 / 11.12)


@pytest.fixture(scope="module")
def weak_quantised():
    """The 27 dB-Hz stream as complex int16 (scaled by 16, rounded) and the statement's figures on exactly those values."""
    w = tc.WEAK
    raw, x = tc.quantised(tc.weak_stream(WEAK_SEED))
    raw = np.concatenate([raw, tc.quantised(tc.weak_tail(WEAK_SEED, TAIL_MS))[0]])       # (the search sees the first 200 ms)
    rows = {}
    for prn in (w["prn"], w["absent"]):
        m = tc.weak_map(x, prn)
        peaks, _ = tc.deep_detect(m, 1, w["excl_code"], w["excl_bins"])
        rows[prn] = (peaks[0], tc.two_peak_ratio(m, w["fs"]))
    print({prn: (p["bin"], p["code"], round(p["z"], 3), round(r, 4)) for prn, (p, r) in rows.items()})
    # the seed is one where the two rules part with margin: the ratio below 1.5 by 5 %, z_0 above 7 by 2 sigma and more
    assert rows[w["prn"]][1] < 1.43 and rows[w["prn"]][0]["z"] > 9.0 and rows[w["absent"]][0]["z"] < 6.0
    return raw, rows


def test_manager_acquires_on_the_noise_floor_what_the_ratio_rule_misses(engine, weak_quantised):
    """PRN 7 at 27 dB-Hz and the absent PRN 12, 5 ms x 40 blocks.
    With `threshold = 1.5` alone the search is the reference's and so is what follows it: the packet's peak_ratio is below the
    threshold -- the two-peak rule does not acquire PRN 7, nor PRN 12 -- and that is all `threshold` ever did here: like the
    reference's channels (channel_l1ca_kaplan.py parses acq_threshold and never reads it) a channel without
    `detection_sigmas` starts tracking whatever it found, which the feature must not change.
    With `detection_sigmas = 7` PRN 7 is acquired at the statement's cell and tracks; PRN 12 is rejected and its channel IDLE."""
    from sydr_amd.utils.enumerations import ChannelState
    w = tc.WEAK
    raw, rows = weak_quantised
    want, want_ratio = rows[w["prn"]]
    spy, states, acq, trk, detections, thresholds = _run(engine, {}, raw, 200 + TAIL_MS, (w["prn"], w["absent"]))
    print(f"threshold alone: ratios {[acq[c]['peak_ratio'] for c in (0, 1)]} states {states}")
    assert len(spy.calls["pcps"]) == 1 and not spy.calls["acq_deep_detect"] and not detections
    assert (acq[0]["frequency_idx"], acq[0]["code_idx"]) == (want["bin"], want["code"])
    assert acq[0]["peak_ratio"] == pytest.approx(want_ratio, rel=1e-6)
    assert all(acq[c]["peak_ratio"] < thresholds[c] == 1.5 for c in (0, 1))                # not acquired by the ratio rule
    assert states == [ChannelState.TRACKING, ChannelState.TRACKING]                        # ... which, as ever, decides nothing

    spy, states, acq, trk, detections, _ = _run(engine, dict(detection_sigmas="7"), raw, 200 + TAIL_MS, (w["prn"], w["absent"]))
    print(f"detection_sigmas = 7: {detections} states {states} tracking epochs {trk}")
    assert len(spy.calls["acq_deep_detect"]) == 1 and not spy.calls["pcps"] and not spy.calls["acq_deep"]     # one call for both
    assert spy.calls["acq_deep_detect"][0][0][-3:] == (1, 4, 1)          # one peak, rint(1.0 * 4e6 / 1.023e6) = 4 samples, 1 bin
    d7, d12 = detections[0], detections[1]
    assert d7["acquired"] and states[0] is ChannelState.TRACKING and trk[0] > 0
    assert (acq[0]["frequency_idx"], acq[0]["code_idx"]) == (want["bin"], want["code"]) == (d7["peaks"][0]["bin"], d7["peaks"][0]["code"])
    assert d7["peaks"][0]["z"] == pytest.approx(want["z"], rel=1e-6) and d7["noise"]["n_cells"] == 11 * (4000 - 9)
    assert acq[0]["peak_ratio"] < 1.5 and acq[0]["carrierFrequency"] == w["doppler"]
    assert not d12["acquired"] and d12["peaks"][0]["z"] < 6.0 and states[1] is ChannelState.IDLE and trk[1] == 0
    assert set(acq[1]) == set(acq[0])                                    # the packet of a rejected search has the same keys


def test_manager_reports_both_replicas(engine):
    w, r = tc.WEAK, tc.REPLICA
    raw = np.concatenate([tc.quantised(tc.weak_stream(r["seed"], True))[0], tc.quantised(tc.weak_tail(r["seed"], TAIL_MS, True))[0]])
    from sydr_amd.utils.enumerations import ChannelState
    spy, states, acq, trk, detections, _ = _run(engine, dict(detection_sigmas="7", detection_peaks="4"), raw, 200 + TAIL_MS, (w["prn"],))
    d = detections[0]
    print([(p["bin"], p["code"], round(p["z"], 2)) for p in d["peaks"]])
    assert len(d["peaks"]) == 4 and d["acquired"] and states == [ChannelState.TRACKING]
    assert ((d["peaks"][0]["bin"], d["peaks"][0]["code"]), (d["peaks"][1]["bin"], d["peaks"][1]["code"])) == r["cells"]
    assert d["peaks"][1]["z"] > 7.0 and d["peaks"][2]["z"] < 6.0
