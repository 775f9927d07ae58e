"""The delay-Doppler map (sdr_ddm), the CPU side: the two entry points and the two records in the ABI; the oracle-built
model (tests/ddm_cases.py) alone on the inputs the GPU tests use -- the proof that those inputs are fair -- and held equal
to the NumPy statement users read (sydr_amd.dsp.ddm.ddm_statement); the receiver's warm acquisition and `reacquire` on
the oracle engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ddm_cases as dc
import refine_cases as rc
from conftest import REPO
from fake_engine import OracleEngine
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.dsp.ddm import ddm_bins, ddm_statement
from test_abi import declared_symbols
from test_host_layer import KAPLAN_INI, channel_config, drive, rf_signal

NAMES = list(dc.parity_cases())


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_ddm_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("sdr_ddm", "sdr_ddm_bins"):
        assert name in declared_symbols() and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.sdr_abi_version() == 5 == _lib.ABI_VERSION


def test_ddm_bins_host_helper():
    lib = _lib.load()
    for span, step in ((500.0, 25.0), (250.0, 12.5), (125.0, 10.0), (100.0, 7.0), (3.0, 5.0), (0.0, 1.0), (2000.0, 500.0)):
        assert lib.sdr_ddm_bins(span, step) == 2 * int(np.floor(span / step)) + 1 == ddm_bins(span, step)
    for span, step in ((100.0, 0.0), (-1.0, 5.0), (100.0, -5.0), (np.nan, 5.0), (100.0, np.nan), (np.inf, 5.0), (100.0, np.inf)):
        assert lib.sdr_ddm_bins(span, step) == 0 == ddm_bins(span, step), (span, step)


def test_ddm_struct_layouts(tmp_path):
    assert C.sizeof(_lib.DdmCfg) == 56 == _lib.DDM_CFG_DTYPE.itemsize
    assert C.sizeof(_lib.DdmResult) == 48 == _lib.DDM_RESULT_DTYPE.itemsize
    for ct, dt in ((_lib.DdmCfg, _lib.DDM_CFG_DTYPE), (_lib.DdmResult, _lib.DDM_RESULT_DTYPE)):
        for name, (_, off) in dt.fields.items():
            assert getattr(ct, name).offset == off
    fields = [("sdr_ddm_cfg", n) for n, _ in _lib.DdmCfg._fields_] + [("sdr_ddm_result", n) for n, _ in _lib.DdmResult._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu", '
                   "sizeof(sdr_ddm_cfg), sizeof(sdr_ddm_result));\n"
                   + "".join(f'printf(" %zu", offsetof({s}, {n}));\n' for s, n in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    want = [56, 48] + [getattr(_lib.DdmCfg if s == "sdr_ddm_cfg" else _lib.DdmResult, n).offset for s, n in fields]
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == want


# ------------------------------------------------------------------------------------------------ 2. the model alone
@pytest.mark.parametrize("name", NAMES)
def test_model_maximum_is_distinct_on_the_parity_cases(name):
    """The indices are decided beyond rounding: the device must return the model's (peak_bin, peak_tap)."""
    for i, m in enumerate(dc.case_model(dc.parity_cases()[name])):
        if i < 2:
            print(f"{name} item {i}: margin {dc.margin(m['map']):.2e}")
        assert dc.margin(m["map"]) > dc.MARGIN, (name, i)


@pytest.mark.parametrize("name", NAMES)
def test_statement_equals_the_oracle_model(name):
    """sydr_amd.dsp.ddm.ddm_statement (plain NumPy, what users read) against the model built on the oracle's EPL: the
    same sums, so equal to a few ulp of the largest |z|, the same peak and the same record."""
    case = dc.parity_cases()[name]
    for it, m in zip(case["items"], dc.case_model(case)):
        s = ddm_statement(case["rf"], case["codes"][it[0]], case["fs"], (it[2], it[1]) + tuple(it[3:]), case["B"], case["S"],
                          case["first"], case["step"], case["T"], case["span"], case["step_hz"])
        zmax = np.abs(m["z"]).max()
        assert np.abs(s.z - m["z"]).max() <= 1e-12 * zmax and np.array_equal(s.tau, m["tau"])
        assert np.abs(s.map - m["map"]).max() <= 1e-12 * case["B"] * (case["S"] * zmax) ** 2
        for key in ("peak_bin", "peak_tap", "peak_hz", "peak_chips"):
            assert s.result[key] == m["result"][key], key
        for key in ("peak_value", "second_value", "noise_mean"):
            assert abs(s.result[key] - m["result"][key]) <= 1e-12 * m["result"]["peak_value"], key


def test_statement_takes_one_sample_segments_and_refuses_what_the_call_refuses():
    case = dc.parity_cases()["tiny_W131_B8_S8"]
    it = case["items"][0]
    s = ddm_statement(case["rf"], case["codes"][0], case["fs"], (it[2], 64) + tuple(it[3:]), 8, 8, -1.0, 0.5, 5, 2000.0, 500.0)
    assert s.z.shape == (64, 5) and np.isfinite(s.map).all()            # every segment is one sample
    for bad in (dict(S=1), dict(T=0), dict(B=0), dict(W=63), dict(step_hz=0.0)):
        a = dict(W=131, B=8, S=8, T=5, step_hz=500.0)
        a.update(bad)
        with pytest.raises(ValueError):
            ddm_statement(case["rf"], case["codes"][0], case["fs"], (it[2], a["W"]) + tuple(it[3:]), a["B"], a["S"], -1.0, 0.5,
                          a["T"], 2000.0, a["step_hz"])


@pytest.mark.parametrize("fs", [4e6, 10e6])
def test_model_recovers_phase_and_doppler(fs):
    """rem_code off by +1.5 chips, the coarse bin's carrier: the model returns the true phase to a tap step and the true
    Doppler to one grid step (12.5 Hz over 4 ms blocks), the peak at least 10 x what lies a chip or more away."""
    case = dc.parity_cases()[f"acq_{fs / 1e6:g}MHz_row0_B2_S8"]
    it, truth, r = case["items"][0], case["truth"], dc.case_model(case)[0]["result"]
    assert it[5] == 1.5
    assert abs(dc.wrap_chips(it[5] + r["peak_chips"] - truth["phase"])) <= case["step"]
    assert abs(r["peak_hz"] - truth["doppler"]) <= case["step_hz"]
    assert r["peak_value"] / r["second_value"] >= 10.0


def test_model_on_noise_alone():
    """The value tests/test_gpu_ddm.py takes its cap from (twice this, below 3)."""
    r = dc.case_model(dc.noise_case())[0]["result"]
    ratio = r["peak_value"] / r["second_value"]
    print(f"noise alone: peak / second = {ratio:.4f}")
    assert abs(ratio - 1.0126) < 1e-3


# ------------------------------------------------------------------------------------------------ 3. the receiver
class DdmOracleEngine(OracleEngine):
    """The oracle engine with `ddm`: the model of tests/ddm_cases.py on its ring."""

    def __init__(self):
        super().__init__()
        self.calls["ddm"] = 0
        self.ddm_items = []

    def ddm(self, items, fs, n_blocks, n_segments, first_chips, step_chips, n_taps, span_hz, step_hz, want_map=True,
            want_segments=False):
        self.calls["ddm"] += 1
        raw = self.ring.astype(np.float64)
        rf = raw[0::2] + 1j * raw[1::2]
        res = np.zeros(len(items), dtype=_lib.DDM_RESULT_DTYPE)
        maps = []
        for k, it in enumerate(np.atleast_1d(items)):
            self.ddm_items.append(it.copy())
            row = (int(it["code_slot"]), int(it["n_samples"]), int(it["start_sample"]), float(it["carrier_hz"]),
                   float(it["rem_carrier"]), float(it["rem_code"]), float(it["code_step"]))
            m = dc.ddm_model(rf, self.codes[row[0]], fs, row, n_blocks, n_segments, first_chips, step_chips, n_taps, span_hz, step_hz)
            for key, v in m["result"].items():
                res[key][k] = v
            maps.append(m["map"])
        return res, (np.stack(maps) if want_map else None), None


# A warm search over the plugin's 1 ms slab estimates the carrier from ONE millisecond: the Cramer-Rao bound of a tone's
# frequency over T = 1 ms at the post-correlation SNR of these recordings (amplitude 8 or 7 in noise of sigma 20 per
# component, 4000 samples: 2 * SNR * N = 640 or 490) is sqrt(6 / (2 * SNR * N)) / (2 * pi * T) = 15 or 18 Hz.  Three of
# those and half a 25 Hz grid step:
WARM_HZ = {8.0: 60.0, 7.0: 65.0}
ACQ_KEYS = {"cid", "type", "carrierFrequency", "codeOffset", "frequency_idx", "code_idx", "correlation_map", "peak_ratio"}


def _manager(n_channels=1):
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    eng = DdmOracleEngine()
    mgr = ChannelManager(rf_signal(4e6), engine=eng)
    mgr.addChannel(ChannelL1CA_Kaplan, channel_config(KAPLAN_INI), n_channels)
    return mgr, eng


def _acquisitions(ticks):
    from sydr_amd.utils.enumerations import ChannelMessage
    return [p for t in ticks for p in t if p["type"] is ChannelMessage.ACQUISITION_UPDATE]


def test_warm_request_searches_with_one_ddm_call_and_lands_where_pcps_lands():
    from sydr_amd.utils.enumerations import ChannelState
    c = rc.acquired(4e6, *rc.SATELLITES[0])
    cold_mgr, cold_eng = _manager()
    cold = cold_mgr.requestTracking(rc.PRN)
    cold_acq = _acquisitions(drive(cold_mgr, c["raw"], 4000, 3))
    assert len(cold_acq) == 1 and cold_eng.calls["pcps"] == 1 and cold_eng.calls["ddm"] == 0

    mgr, eng = _manager()
    cstep = orc.CODE_RATE * (1.0 + c["doppler"] / 1575.42e6) / 4e6
    # the prediction: the satellite's phase at ring sample 1000, 1.5 chips and 180 Hz off the truth
    phase = (rc.CODE_PHASE + 1000 * cstep) % orc.CODE_CHIPS + 1.5
    ch = mgr.requestTrackingWarm(rc.PRN, c["doppler"] + 180.0, phase, 1000)
    acq = _acquisitions(drive(mgr, c["raw"], 4000, 3))
    assert len(acq) == 1 and eng.calls["ddm"] == 1 and eng.calls["pcps"] == 0
    assert set(acq[0]) == ACQ_KEYS | {"warm_start"} and acq[0]["warm_start"] is True
    assert acq[0]["correlation_map"].shape == (41, 33) and acq[0]["peak_ratio"] >= 10.0
    assert acq[0]["frequency_idx"] == int(np.argmax(acq[0]["correlation_map"].max(axis=1)))
    assert abs(acq[0]["carrierFrequency"] - c["doppler"]) <= WARM_HZ[rc.amplitude(4e6)]
    assert abs(acq[0]["code_idx"] - cold_acq[0]["code_idx"]) <= 1
    assert ch.channelState is ChannelState.TRACKING and abs(ch.currentSample - cold.currentSample) <= 1
    assert set(cold_acq[0]) == ACQ_KEYS                                  # a cold acquisition's packet is the parent's


def test_a_ticks_warm_channels_share_one_call():
    raw, _, items = rc.many_items()
    mgr, eng = _manager(3)
    for k in range(3):
        s = rc.MANY_SATS[k]
        cstep = orc.CODE_RATE * (1.0 + s["doppler"] / 1575.42e6) / 4e6
        mgr.requestTrackingWarm(s["prn"], s["doppler"] + 60.0, (s["code_phase"] + 2000 * cstep) % orc.CODE_CHIPS - 0.75, 2000)
    acq = _acquisitions(drive(mgr, raw, 4000, 3))
    assert len(acq) == 3 and eng.calls["ddm"] == 1 and len(eng.ddm_items) == 3 and eng.calls["pcps"] == 0
    for k, p in enumerate(acq):
        assert abs(p["carrierFrequency"] - rc.MANY_SATS[k]["doppler"]) <= WARM_HZ[7.0] and p["peak_ratio"] >= 5.0


def test_reacquire_goes_through_acquiring_and_back():
    from sydr_amd.utils.enumerations import ChannelState
    c = rc.acquired(4e6, *rc.SATELLITES[0])
    mgr, eng = _manager()
    ch = mgr.requestTracking(rc.PRN)
    with pytest.raises(ValueError, match="not tracking"):
        mgr.reacquire(ch.channelID)
    ticks = drive(mgr, c["raw"], 4000, 12)
    assert ch.channelState is ChannelState.TRACKING and eng.calls["pcps"] == 1
    before = (ch.currentSample, ch.carrierFrequency)
    mgr.reacquire(ch.channelID)
    assert ch.channelState is ChannelState.ACQUIRING and not ch.lostLock and ch.currentSample == before[0]
    more = [mgr.run()]                                                   # the ring already holds the slab
    for k in range(12, 16):
        mgr.addNewRFData(c["raw"][2 * k * 4000:2 * (k + 1) * 4000])
        more.append(mgr.run())
    acq = _acquisitions(more)
    assert len(acq) == 1 and acq[0]["warm_start"] is True and eng.calls["ddm"] == 1 and eng.calls["pcps"] == 1
    it = eng.ddm_items[0]
    assert int(it["start_sample"]) == before[0] and float(it["carrier_hz"]) == before[1] and int(it["n_samples"]) == 4000
    assert ch.channelState is ChannelState.TRACKING
    assert abs(ch.carrierFrequency - c["doppler"]) <= WARM_HZ[rc.amplitude(4e6)]
    # the code period it restarts on is the one it was tracking (whole periods on, to a sample)
    assert min((ch.currentSample - before[0]) % 4000, (before[0] - ch.currentSample) % 4000) <= 1


def test_a_manager_that_never_calls_them_emits_the_parents_packets():
    """Recorded in the same test with the three methods absent: the packets are equal, one by one."""
    from sydr_amd.channel.manager import ChannelManager
    c = rc.acquired(4e6, *rc.SATELLITES[0])

    def packets(strip):
        saved = {}
        if strip:
            for name in ("requestTrackingWarm", "reacquire", "delayDopplerMaps"):
                saved[name] = getattr(ChannelManager, name)
                delattr(ChannelManager, name)
        try:
            mgr, eng = _manager()
            mgr.requestTracking(rc.PRN)
            out = [[dict(p) for p in tick] for tick in drive(mgr, c["raw"], 4000, 25)]
            assert eng.calls["ddm"] == 0
            return out
        finally:
            for name, fn in saved.items():
                setattr(ChannelManager, name, fn)
    a, b = packets(True), packets(False)
    assert len(a) == len(b)
    for ta, tb in zip(a, b):
        assert len(ta) == len(tb)
        for pa, pb in zip(ta, tb):
            assert pa.keys() == pb.keys()
            for key in pa:
                assert np.array_equal(np.asarray(pa[key]), np.asarray(pb[key])), key


def test_delay_doppler_maps_on_the_oracle_engine():
    """The GPU test's scenario and checks (tests/test_gpu_ddm.py run_delay_doppler_maps) on the oracle engine: one `ddm`
    call of four items, each the channel's latest epoch carried back to a 4 ms window."""
    from sydr_amd.channel.manager import ChannelManager
    from test_gpu_ddm import run_delay_doppler_maps
    engines = []

    def make():
        engines.append(DdmOracleEngine())
        return ChannelManager(rf_signal(4e6), engine=engines[-1])
    out = run_delay_doppler_maps(make)
    eng = engines[0]
    assert eng.calls["ddm"] == 1 and len(eng.ddm_items) == 4 and len(out) == 4
    for it in eng.ddm_items:
        assert int(it["n_samples"]) == 16000 and float(it["rem_code"]) < -1023.0 * 2.9     # three periods back, and a bit
