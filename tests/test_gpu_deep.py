"""sdr_acq_deep on the MI355X against its NumPy statement (sydr_amd/dsp/deepsearch.py through tests/deep_cases.py; the CPU
file tests/test_deep.py holds the statement against the oracle): maps to 1e-9 of the statement's maximum -- the project's
MAP_RTOL -- ratios to 1e-9 relative, every integer equal.  Every case's statement has its two largest values more than
1e-6 apart (asserted here, never skipped on), so rounding cannot move an index."""
import ctypes as C

import numpy as np
import pytest

import deep_cases as dc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import FMT_CI8
from test_gpu_pcps import ALL_FMTS, FORMAT_GRID, MAP_RTOL, bits_per_ring_format
from test_host_layer import KAPLAN_INI, channel_config, rf_signal

pytestmark = pytest.mark.gpu

INVALID, RANGE, STATE = -1, -5, -6


def _stage(engine, image, cap, fmt, prns):
    engine.iq_alloc(cap, fmt)
    engine.iq_upload(image, 0)
    engine.code_slots(max(2, len(prns)))
    for s, p in enumerate(prns):
        engine.load_gps_code(s, int(p))


def _deep(engine, c, n_prn, start=0, want_map=True, **over):
    a = dict(c)
    a.update(over)
    return engine.acq_deep(np.arange(n_prn), start, a["fs"], a["if_hz"], a["R"], a["S"], a["C"], a["K"], a["G"], a["rf"],
                           want_map=want_map)


def _hold(tag, res, cmap, maps, c):
    """The device's results and maps of every PRN against the statement's."""
    for k, m in enumerate(maps):
        margin = dc.top2_margin(m)
        g, b, n, end, value, ratio = dc.statement_results(m, c["fs"], c)
        err = np.abs(cmap[k] - m).max() / m.max()
        r = res[k]
        print(f"{tag} PRN {k}: margin {margin:.2e}, map error {err:.2e} of the maximum, peak ({g}, {b}, {n}) end {end} "
              f"ratio {ratio:.6f} (device {r['peak_ratio']:.6f})")
        assert margin > dc.MARGIN
        assert cmap[k].shape == m.shape and err <= MAP_RTOL
        assert (int(r["peak_group"]), int(r["peak_bin"]), int(r["peak_code"]), int(r["peak_code_end"])) == (g, b, n, end)
        assert r["peak_ratio"] == pytest.approx(ratio, rel=1e-9)
        assert r["peak_value"] == cmap[k][g, b, n] and r["peak_value"] == pytest.approx(value, rel=MAP_RTOL)


@pytest.mark.parametrize("name", sorted(dc.PARITY))
def test_parity_with_the_statement(engine, name):
    c, image, cap, start, _ = dc.parity_input(name)
    _stage(engine, image, cap, c["fmt"], c["prns"])
    for opt, v in c["options"]:
        engine.set_option(opt, v)
    try:
        res, cmap = _deep(engine, c, len(c["prns"]), start)
    finally:
        for opt, _ in c["options"]:
            engine.set_option(opt, 0)
    _hold(name, res, cmap, dc.parity_statement(name), c)


def test_shifts_of_several_code_periods_both_ways(engine):
    """carrier_rf_hz = 1e6: |q| up to 8400 samples on a 4000-sample code, negative on the lower bins, 0 (mod N) at blocks 10
    and 20; PRN 0 peaks at n = 0 of the top bin, PRN 1 at n = N - 1 of the bottom one (tests/deep_cases.py SHIFT)."""
    c, raw, _ = dc.shift_input()
    _stage(engine, raw, raw.size // 2, FMT_CI8, c["prns"])
    res, cmap = _deep(engine, c, 2)
    _hold("shift", res, cmap, dc.shift_statement(), c)
    assert [(int(r["peak_bin"]), int(r["peak_code"])) for r in res] == [(4, 0), (0, 3999)]
    # peak_code_end = peak_code + q[b][K] = 0 + 8400 and 3999 - 8400 (mod 4000)
    assert [int(r["peak_code_end"]) for r in res] == [400, 3599]


@pytest.mark.parametrize("name", ["ci8_c2_k3_g2", "cf64_c20_k5_g1", "n25000", "chirpz_4006"])
def test_without_groups_and_shift_it_is_the_parents_search(engine, name):
    """G = 1, carrier_rf_hz = 0 against sdr_pcps(coh, noncoh, want_map) on the same ring: the folded route adds the same
    terms in another order -- 2e-9 of the maximum, the same peak."""
    c, image, cap, start, _ = dc.parity_input(name)
    _stage(engine, image, cap, c["fmt"], c["prns"])
    n_prn = len(c["prns"])
    res, cmap = _deep(engine, c, n_prn, start, G=1, rf=0.0)
    pb, pc, pr, ref = engine.pcps(np.arange(n_prn), start, c["fs"], c["if_hz"], c["R"], c["S"], c["C"], c["K"], want_map=True)
    for k in range(n_prn):
        err = np.abs(cmap[k, 0] - ref[k]).max() / ref[k].max()
        print(f"{name} PRN {k}: {err:.2e} of the maximum; ratio {res[k]['peak_ratio']:.9f} / {pr[k]:.9f}")
        assert err <= 2e-9
        assert (int(res[k]["peak_bin"]), int(res[k]["peak_code"]), int(res[k]["peak_group"])) == (int(pb[k]), int(pc[k]), 0)
        assert res[k]["peak_code_end"] == res[k]["peak_code"]


def test_two_calls_return_the_same_bits(engine):
    c, image, cap, start, _ = dc.parity_input("ci8_c2_k3_g2")
    _stage(engine, image, cap, c["fmt"], c["prns"])
    res1, map1 = _deep(engine, c, 2, rf=1e6)
    res2, map2 = _deep(engine, c, 2, rf=1e6)
    res3, none = _deep(engine, c, 2, rf=1e6, want_map=False)
    assert none is None and map1.tobytes() == map2.tobytes()
    assert res1.tobytes() == res2.tobytes() == res3.tobytes()


def test_same_bits_from_every_ring_format(engine):
    """C = 2, K = 2, G = 1: the fold kernel's load is the only code that knows the ring's format."""
    def run(start):
        res, cmap = engine.acq_deep(np.arange(2), start, 4e6, 0.0, *FORMAT_GRID, 2, 2, 1, 0.0, want_map=True)
        assert cmap.shape == (2, 1, 5, 4000) and [int(r["peak_bin"]) for r in res] == [1, 4]
        return res, cmap
    bits = bits_per_ring_format(engine, 4, run)
    for fmt in ALL_FMTS[1:]:
        assert bits[fmt] == bits[FMT_CI8], f"ring format {fmt}"


def test_long_window_keeps_its_peak(engine):
    """One second at 4 MHz from the device's synthesiser, one satellite at +4500 Hz and 30 dB-Hz: C = 1, K = 1000, +-5 kHz by
    500 Hz, compensation on.  The code slides 11.4 samples over the window; sdr_pcps(coh = 1, noncoh = 1000) smears its peak
    over them (CPU check with NumPy noise: ratio 1.01-1.02 against 1.33)."""
    fs, n, dop, cp, sigma = 4e6, 4000, 4500.0, 1023 - 1000.25, 30.0
    amp = sigma * np.sqrt(2 * 10 ** 3.0 / fs)
    engine.iq_alloc(1000 * n, FMT_CI8)
    engine.code_slots(2)
    engine.load_gps_code(0, 7)
    engine.iq_synth([dict(prn=7, doppler=dop, code_phase=cp, phase=0.1, amp=amp)], fs, sigma, 20260018, 0, 1000 * n)
    res, _ = engine.acq_deep([0], 0, fs, 0.0, 5000.0, 500.0, 1, 1000, 1, dc.L1)
    pb, pc, pr, _ = engine.pcps([0], 0, fs, 0.0, 5000.0, 500.0, 1, 1000)
    r = res[0]
    true_bin, true_code = int(round((-dop + 5000.0) / 500.0)), int(np.ceil(1000.25 * fs / orc.CODE_RATE))
    print(f"deep: bin {r['peak_bin']} code {r['peak_code']} end {r['peak_code_end']} ratio {r['peak_ratio']:.4f}; "
          f"sdr_pcps: bin {pb[0]} code {pc[0]} ratio {pr[0]:.4f}; true bin {true_bin} code {true_code}")
    assert int(r["peak_bin"]) == true_bin and abs(int(r["peak_code"]) - true_code) <= 1
    assert int(r["peak_code_end"]) == (int(r["peak_code"]) - 11) % n       # nearbyint(-4500 * 4e6 / 1575.42e6) = -11
    assert r["peak_ratio"] > pr[0]


def test_argument_errors_touch_nothing(engine):
    c, image, cap, start, _ = dc.parity_input("ci8_c2_k3_g2")
    _stage(engine, image, cap, c["fmt"], c["prns"])
    good, good_map = _deep(engine, c, 2)
    lib = _lib.load()
    slots = np.arange(2, dtype=np.int32)
    res = np.full(2, 7, dtype=_lib.DEEP_RESULT_DTYPE)
    untouched = res.tobytes()

    def call(slots_p=_lib.ptr(slots), n_prn=2, start=0, cfg_null=False, res_p=_lib.ptr(res), **over):
        a = dict(fs=c["fs"], if_hz=0.0, R=c["R"], S=c["S"], rf=0.0, C=c["C"], K=c["K"], G=c["G"])
        a.update(over)
        cfg = _lib.DeepCfg(a["fs"], a["if_hz"], a["R"], a["S"], a["rf"], a["C"], a["K"], a["G"], 0)
        return lib.sdr_acq_deep(engine._h, slots_p, n_prn, start, None if cfg_null else C.byref(cfg), res_p, None)

    engine.prof_enable(True)
    engine.prof_reset()
    try:
        for kwargs in (dict(slots_p=None), dict(cfg_null=True), dict(res_p=None), dict(n_prn=0), dict(C=0), dict(C=21), dict(K=0),
                       dict(G=0), dict(G=3), dict(K=1, G=2), dict(S=0.0), dict(R=-1.0), dict(R=float("nan")), dict(rf=-1.0),
                       dict(rf=float("inf")), dict(rf=float("nan")), dict(fs=0.0)):
            assert call(**kwargs) == INVALID and lib.sdr_last_error(), kwargs
        bad = np.array([0, 5], dtype=np.int32)            # a slot nothing was staged in / outside the slots
        assert call(slots_p=_lib.ptr(bad)) == INVALID and b"not staged" in lib.sdr_last_error()
        assert call(start=-1) == RANGE and call(K=4) == RANGE           # 2 x 4 x 4000 samples in a ring of 24 000
        assert engine.prof_read("")[1] == 0                             # no kernel, no scope: nothing reached the device
    finally:
        engine.prof_enable(False)
        engine.prof_reset()
    assert res.tobytes() == untouched
    again, again_map = _deep(engine, c, 2)                              # the engine is as it was
    assert again.tobytes() == good.tobytes() and again_map.tobytes() == good_map.tobytes()


def test_calls_before_their_state_exists():
    from sydr_amd.engine import Engine
    e = Engine(0)
    try:
        with pytest.raises(_lib.SdrError) as err:
            e.acq_deep([0], 0, 4e6, 0.0, 1000.0, 250.0, 2, 2)
        assert err.value.status == STATE and "ring" in str(err.value)
        e.iq_alloc(16000, FMT_CI8)
        with pytest.raises(_lib.SdrError) as err:
            e.acq_deep([0], 0, 4e6, 0.0, 1000.0, 250.0, 2, 2)
        assert err.value.status == STATE and "slots" in str(err.value)
    finally:
        e.close()


def test_profiling_scopes(engine):
    """The per-stage scopes record with sdr_prof_enable(e, 1), the whole call's scope with (e, 2) -- the library records one
    kind or the other (engine.hip ProfScope), as for every other call."""
    c, image, cap, start, _ = dc.parity_input("ci8_c2_k3_g2")
    _stage(engine, image, cap, c["fmt"], c["prns"])
    _deep(engine, c, 2)
    names = ("deep_fold", "deep_fwd_fft", "deep_inv_fft", "deep_shift_acc", "deep_peak", "call_acq_deep", "call_pcps")
    counts = {}
    for calls_only in (False, True):
        engine.prof_enable(True, calls_only=calls_only)
        engine.prof_reset()
        try:
            _deep(engine, c, 2)
            counts[calls_only] = {s: engine.prof_read(s)[1] for s in names}
        finally:
            engine.prof_enable(False)
            engine.prof_reset()
    assert counts[False] == dict(deep_fold=3, deep_fwd_fft=3, deep_inv_fft=3, deep_shift_acc=3, deep_peak=1, call_acq_deep=0,
                                 call_pcps=0)
    assert counts[True] == dict(deep_fold=0, deep_fwd_fft=0, deep_inv_fft=0, deep_shift_acc=0, deep_peak=0, call_acq_deep=1,
                                call_pcps=0)


def test_function_level_deep_search():
    from sydr_amd.dsp.deepsearch import DeepSearch
    c, _, _, _, win = dc.parity_input("ci8_c2_k3_g2")
    n = orc.samples_per_code(c["fs"])
    ref = dc.parity_statement("ci8_c2_k3_g2")[0]
    for code in (orc.gold_code(c["prns"][0]), orc.code_spectrum(orc.gold_code(c["prns"][0]), c["fs"])):
        got = DeepSearch(win, c["if_hz"], c["fs"], code, c["R"], c["S"], n, c["C"], c["K"], c["G"], c["rf"])
        assert got.shape == ref.shape and np.abs(got - ref).max() <= MAP_RTOL * ref.max()


# ------------------------------------------------------------------------------------------------ the plugins, end to end
class _Spy:
    """The engine's two search calls counted (patched on the instance, taken off again on exit)."""

    def __init__(self, engine):
        self._e, self.pcps_args, self.deep_args = engine, [], []

    def __enter__(self):
        def pcps(*a, **k):
            self.pcps_args.append((a, k))
            return type(self._e).pcps(self._e, *a, **k)

        def acq_deep(*a, **k):
            self.deep_args.append((a, k))
            return type(self._e).acq_deep(self._e, *a, **k)

        self._e.pcps, self._e.acq_deep = pcps, acq_deep
        return self

    def __exit__(self, *exc):
        del self._e.pcps, self._e.acq_deep


def _run(engine, extra, raw, ms, ring_ms=100):
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.utils.enumerations import ChannelMessage
    cfg = channel_config(KAPLAN_INI)
    cfg["ACQUISITION"].update(extra)
    mgr = ChannelManager(rf_signal(4e6), engine=engine, ring_ms=ring_ms)
    try:
        mgr.addChannel(ChannelL1CA_Kaplan, cfg, 1)
        ch = mgr.requestTracking(7)
        acq, trk = [], []
        with _Spy(engine) as spy:
            for k in range(ms):
                mgr.addNewRFData(raw[2 * k * 4000:2 * (k + 1) * 4000])
                for p in mgr.run():
                    if p["type"] is ChannelMessage.ACQUISITION_UPDATE:
                        acq.append(p)
                    elif p["type"] is ChannelMessage.TRACKING_UPDATE:
                        trk.append(p)
        return spy, ch, acq, trk, ch.channelState
    finally:
        mgr.close()


def test_manager_acquires_deep_and_tracks_from_the_windows_end(engine):
    """bit_edge_groups = 2, code_doppler_compensation = 1, 10 ms x 20 blocks on a satellite at -4750 Hz: over the 200 ms window
    the code slides 2.4 samples (0.6 chip).  Tracking starts behind the window, from peak_code_end: its first epochs hold the
    prompt power (amplitude x samples = 32 000 per axis sum; a start 0.6 chip off would hold 0.4 of it)."""
    from sydr_amd.utils.enumerations import ChannelState
    fs, dop, amp = 4e6, -4750.0, 8.0
    alternating = np.resize([1, -1], 40)
    raw = orc.synth_iq(fs, 230 * 4000, [dict(prn=7, doppler=dop, code_phase=300.25, phase=0.1, amp=amp, data=alternating)],
                       20.0, 20260019)
    spy, ch, acq, trk, state = _run(engine, dict(bit_edge_groups="2", code_doppler_compensation="1", coherent_integration="10",
                                                 non_coherent_integration="20"), raw, 230, ring_ms=300)
    assert len(spy.deep_args) == 1 and not spy.pcps_args and len(acq) == 1 and state is ChannelState.TRACKING
    a = acq[0]
    prompt = np.array([np.hypot(p["i_prompt"], p["q_prompt"]) for p in trk[:10]])
    print(f"bin {a['frequency_idx']} code {a['code_idx']} -> offset {a['codeOffset']} group {a['bit_edge_group']} ratio "
          f"{a['peak_ratio']:.2f}; |prompt| of the first epochs {np.round(prompt)}")
    assert a["frequency_idx"] == int(round((-dop + 5000.0) / 250.0)) and a["carrierFrequency"] == dop
    assert a["codeOffset"] == (a["code_idx"] + 2) % 4000 and a["bit_edge_group"] in (0, 1)      # nearbyint(4750 * 8e5 / 1575.42e6) = 2
    assert a["correlation_map"].shape == (41, 4000)
    assert len(prompt) == 10 and prompt.mean() >= 0.7 * amp * 4000


def test_manager_without_the_keys_is_the_parents(engine):
    """No key, no new call: the ACQUISITION_UPDATE packet is sdr_pcps's result on the same samples, bit for bit, under the
    parent's keys."""
    fs = 4e6
    raw = orc.synth_iq(fs, 12 * 4000, [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=8.0)], 20.0, 99)
    spy, ch, acq, trk, _ = _run(engine, {}, raw, 12)
    assert not spy.deep_args and len(spy.pcps_args) == 1 and len(acq) == 1 and trk
    assert spy.pcps_args[0] == (([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1), dict(want_map=True))
    a = acq[0]
    assert set(a) == {"cid", "type", "carrierFrequency", "codeOffset", "frequency_idx", "code_idx", "correlation_map", "peak_ratio"}
    engine.iq_alloc(4000, FMT_CI8)
    engine.iq_upload(raw[:8000], 0)
    engine.code_slots(1)
    engine.load_gps_code(0, 7)
    pb, pc, pr, cmap = engine.pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1, want_map=True)
    assert (a["frequency_idx"], a["code_idx"], a["codeOffset"], a["peak_ratio"]) == (int(pb[0]), int(pc[0]), int(pc[0]), float(pr[0]))
    assert a["correlation_map"].tobytes() == cmap[0].tobytes()
