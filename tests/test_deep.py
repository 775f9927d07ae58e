"""Deep acquisition (sdr_acq_deep), the CPU side: the two new entry points in the ABI, the NumPy statement against the
oracle's PCPS and against the library's shift helper, the bit-edge scenario on the statement alone, the margins of the
cases the GPU tests use (tests/test_gpu_deep.py) and the plugins' two optional [ACQUISITION] keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deep_cases as dc
from conftest import REPO
from fake_engine import OracleEngine
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
from sydr_amd.channel.manager import ChannelManager
from sydr_amd.utils.enumerations import ChannelMessage, ChannelState
from test_abi import declared_symbols
from test_host_layer import KAPLAN_INI, channel_config, drive, rf_signal


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_deep_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("sdr_acq_deep", "sdr_acq_deep_shift"):
        assert name in declared_symbols() and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.sdr_abi_version() == 5 == _lib.ABI_VERSION


def test_deep_struct_layouts(tmp_path):
    assert C.sizeof(_lib.DeepCfg) == 56 and _lib.DEEP_RESULT_DTYPE.itemsize == 48
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(sdr_deep_cfg),sizeof(sdr_deep_result),offsetof(sdr_deep_cfg,coh),offsetof(sdr_deep_result,peak_group),"
                   "offsetof(sdr_deep_result,peak_ratio),offsetof(sdr_deep_result,peak_value));return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    f = _lib.DEEP_RESULT_DTYPE.fields
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == \
        [56, 48, _lib.DeepCfg.coh.offset, f["peak_group"][1], f["peak_ratio"][1], f["peak_value"][1]]


# ------------------------------------------------------------------------------------------------ 2. the statement
@pytest.mark.parametrize("fs,C_,K,R,S,if_hz", [(4e6, 2, 3, 1000.0, 250.0, 0.0), (4e6, 10, 2, 500.0, 250.0, 1500.0),
                                               (2.046e6, 1, 4, 750.0, 250.0, 0.0), (4e6, 20, 1, 250.0, 250.0, 0.0)])
def test_statement_without_groups_and_shift_is_the_oracles_pcps(fs, C_, K, R, S, if_hz):
    """G = 1, carrier_rf_hz = 0: folding only changes the order of additions (measured: 4e-16 of the maximum)."""
    n = orc.samples_per_code(fs)
    raw = orc.synth_iq(fs, C_ * K * n, [dict(prn=7, doppler=250.0, code_phase=300.25, phase=0.1, amp=6.0)], 20.0, 11)
    rf = orc.iq_to_complex(raw)
    code_fft = orc.code_spectrum(orc.gold_code(7), fs)
    ref = orc.pcps_map(rf.reshape(1, -1), if_hz, fs, code_fft, R, S, n, C_, K)
    got = dc.deep_map(rf, if_hz, fs, code_fft, R, S, n, C_, K, 1, 0.0)
    err = np.abs(got[0] - ref).max() / ref.max()
    print(f"fs={fs / 1e6} C={C_} K={K}: {err:.2e} of the maximum")
    assert got.shape == (1, len(orc.doppler_bins(R, S)), n) and err <= 1e-12


def test_statement_groups_partition_the_blocks():
    """M(G = 1) = M(G = 2)[0] + M(G = 2)[1] with the same shifts (the order of additions aside)."""
    fs, n = 4e6, 4000
    raw = orc.synth_iq(fs, 2 * 5 * n, [dict(prn=7, doppler=-750.0, code_phase=17.5, phase=0.1, amp=6.0)], 20.0, 12)
    rf, code_fft = orc.iq_to_complex(raw), orc.code_spectrum(orc.gold_code(7), fs)
    one = dc.deep_map(rf, 0.0, fs, code_fft, 1000.0, 250.0, n, 2, 5, 1, 1e6)
    two = dc.deep_map(rf, 0.0, fs, code_fft, 1000.0, 250.0, n, 2, 5, 2, 1e6)
    np.testing.assert_allclose(two.sum(axis=0), one[0], rtol=0, atol=1e-12 * one.max())


def test_deep_shift_is_the_librarys():
    """deep_shift against sdr_acq_deep_shift on grids whose products land on and next to .5 (half-even), both signs, block =
    K included; 0 without compensation, for a NULL cfg and for negative arguments."""
    lib = _lib.load()
    for fs, R, S, C_, rf in ((4e6, 5000.0, 50.0, 10, dc.L1), (4e6, 5000.0, 2500.0, 20, 1e6), (25e6, 5000.0, 250.0, 20, dc.L1),
                             (4e6, 5000.0, 1250.0, 1, 1e7), (4e6, 5000.0, 250.0, 3, 0.0)):
        cfg = _lib.DeepCfg(fs, 0.0, R, S, rf, C_, 50, 1, 0)
        n, nbins = orc.samples_per_code(fs), len(orc.doppler_bins(R, S))
        for b in range(nbins):
            for i in (0, 1, 2, 3, 7, 10, 20, 49, 50, 1000):
                assert lib.sdr_acq_deep_shift(C.byref(cfg), b, i) == dc.deep_shift(R, S, n, C_, rf, b, i), (fs, rf, b, i)
    # d * t / rf = 1250 * 4000 i / 1e7 = i / 2: the halves round to even
    cfg = _lib.DeepCfg(4e6, 0.0, 5000.0, 1250.0, 1e7, 1, 50, 1, 0)
    assert [lib.sdr_acq_deep_shift(C.byref(cfg), 5, i) for i in range(6)] == [0, 0, 1, 2, 2, 2]
    assert [lib.sdr_acq_deep_shift(C.byref(cfg), 3, i) for i in range(6)] == [0, 0, -1, -2, -2, -2]
    assert lib.sdr_acq_deep_shift(None, 0, 1) == 0 and lib.sdr_acq_deep_shift(C.byref(cfg), -1, 1) == 0
    assert lib.sdr_acq_deep_shift(C.byref(cfg), 0, -1) == 0


def test_bit_edge_scenario_on_the_statement():
    """4 MHz, PRN 7, +4800 Hz, 30 dB-Hz, data alternating every 20 periods, the window 5 periods into a bit; C = 10, K = 20,
    +-5 kHz by 50 Hz.  Group 0 of G = 2 holds no bit edge: its peak ratio on the true bin beats G = 1's, which beats the
    uncompensated reference's (measured on this input: 2.28 > 1.74 > 1.60; three noise seeds gave 2.28-2.34,
    1.74-1.78, 1.57-1.69).  G = 1 is the sum of the two groups, and the uncompensated reference is the statement with
    G = 1 and no shift -- both identities are held by the tests above, so two evaluations of the statement serve all three."""
    c = dc.BIT_EDGE
    x, true_bin, true_code = dc.bit_edge_signal(0)
    code_fft = orc.code_spectrum(orc.gold_code(c["prn"]), c["fs"])
    grouped = dc.deep_map(x, 0.0, c["fs"], code_fft, c["R"], c["S"], 4000, c["C"], c["K"], 2, dc.L1)
    plain = dc.deep_map(x, 0.0, c["fs"], code_fft, c["R"], c["S"], 4000, c["C"], c["K"], 1, 0.0)[0]
    cfg = dict(R=c["R"], S=c["S"], C=c["C"], K=c["K"], rf=dc.L1)
    g, b, n, end, _, ratio_g2 = dc.statement_results(grouped, c["fs"], cfg)
    _, ratio_g1 = orc.two_peak_compare(grouped.sum(axis=0), 4000, 4)
    _, ratio_ref = orc.two_peak_compare(plain, 4000, 4)
    print(f"group {g} bin {b} (true {true_bin}) code {n} (true {true_code}) end {end}: "
          f"ratio G=2 {ratio_g2:.3f}, G=1 {ratio_g1:.3f}, uncompensated reference {ratio_ref:.3f}")
    assert g == 0 and b == true_bin and abs(n - true_code) <= 1
    assert ratio_g2 > ratio_g1 > ratio_ref
    # the window is 0.2 s long: at +4800 Hz the code has come 2.4 samples early by its end
    assert end == (n - 2) % 4000


@pytest.mark.parametrize("name", sorted(n for n in dc.PARITY if n != "n25000"))
def test_parity_cases_have_a_distinct_maximum(name):
    """The GPU parity test holds integers equal: the statement's two largest values must be further apart than rounding
    (the 25 MHz statement is evaluated once, by the GPU test, which asserts its margin itself)."""
    for m in dc.parity_statement(name):
        print(f"{name}: margin {dc.top2_margin(m):.2e}")
        assert dc.top2_margin(m) > dc.MARGIN


def test_shift_case_peaks_sit_on_the_edges():
    """What the shift case is for: shifts of two code periods both ways, and peaks at n = 0 and n = N - 1."""
    c = dc.SHIFT
    qs = [dc.deep_shift(c["R"], c["S"], 4000, c["C"], c["rf"], b, i) for b in range(5) for i in range(c["K"] + 1)]
    assert min(qs) == -8400 and max(qs) == 8400 and {4000, -4000, 8000, -8000, 0} <= set(qs)
    res = [dc.statement_results(m, c["fs"], c) for m in dc.shift_statement()]
    print(res)
    assert [r[:3] for r in res] == [(0, 4, 0), (0, 0, 3999)]
    assert all(dc.top2_margin(m) > dc.MARGIN for m in dc.shift_statement())


# ------------------------------------------------------------------------------------------------ 3. the plugins' keys
class DeepOracleEngine(OracleEngine):
    """The oracle-backed engine with acq_deep served by the statement; `end_offset` is added to peak_code_end so that the
    test can tell which of the two code indices the channel took."""

    def __init__(self, end_offset=0):
        super().__init__()
        self.calls["acq_deep"] = 0
        self.deep_args, self.pcps_args, self.end_offset = [], [], end_offset

    def pcps(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh=1, noncoh=1, want_map=False):
        self.pcps_args.append((list(code_slots), start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh, want_map))
        return super().pcps(code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh, want_map)

    def acq_deep(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh, groups=1,
                 carrier_rf_hz=0.0, want_map=False):
        self.calls["acq_deep"] += 1
        self.deep_args.append((list(code_slots), start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh, groups,
                               carrier_rf_hz, want_map))
        n = orc.samples_per_code(fs)
        rf = self._complex(start_sample, n * coh * noncoh)
        cfg = dict(R=doppler_range, S=doppler_step, C=coh, K=noncoh, rf=carrier_rf_hz)
        res = np.zeros(len(code_slots), dtype=_lib.DEEP_RESULT_DTYPE)
        maps = []
        for k, s in enumerate(code_slots):
            m = dc.deep_map(rf, if_hz, fs, orc.code_spectrum(self.codes[int(s)], fs), doppler_range, doppler_step, n, coh,
                            noncoh, groups, carrier_rf_hz)
            g, b, c, end, v, ratio = dc.statement_results(m, fs, cfg)
            res[k] = (b, c, (end + self.end_offset) % n, g, 0, ratio, v)
            maps.append(m)
        return res, (np.stack(maps) if want_map else None)


def _acquire(ini_extra, end_offset=0, prns=(7, 12)):
    fs, spms = 4e6, 4000
    sats = [dict(prn=p, doppler=d, code_phase=c, phase=0.1, amp=8.0) for p, d, c in ((7, 1750.0, 300.25), (12, -3000.0, 17.5))]
    raw = orc.synth_iq(fs, 12 * spms, sats, 20.0, 99)
    cfg = channel_config(KAPLAN_INI)
    cfg["ACQUISITION"]["coherent_integration"] = "2"
    cfg["ACQUISITION"]["non_coherent_integration"] = "2"
    for k, v in ini_extra.items():
        cfg["ACQUISITION"][k] = v
    eng = DeepOracleEngine(end_offset)
    mgr = ChannelManager(rf_signal(fs), engine=eng)
    mgr.addChannel(ChannelL1CA_Kaplan, cfg, len(prns))
    chans = [mgr.requestTracking(p) for p in prns]
    ticks = drive(mgr, raw, spms, 12)
    acq = [p for t in ticks for p in t if p["type"] is ChannelMessage.ACQUISITION_UPDATE]
    trk = [p for t in ticks for p in t if p["type"] is ChannelMessage.TRACKING_UPDATE]
    return eng, chans, acq, trk


def test_manager_without_the_keys_searches_as_before():
    eng, chans, acq, _ = _acquire({})
    assert eng.calls["pcps"] == 1 and eng.calls["acq_deep"] == 0
    assert eng.pcps_args == [([0, 1], 0, 4e6, 0.0, 5000.0, 250.0, 2, 2, True)]
    assert len(acq) == 2 and all(set(a) == {"cid", "type", "carrierFrequency", "codeOffset", "frequency_idx", "code_idx",
                                            "correlation_map", "peak_ratio"} for a in acq)
    assert all(a["codeOffset"] == a["code_idx"] and a["correlation_map"].shape == (41, 4000) for a in acq)
    assert all(ch.acq_deep is None for ch in chans)


@pytest.mark.parametrize("extra,deep", [({"bit_edge_groups": "2", "code_doppler_compensation": "1"}, (2, 1575.42e6)),
                                        ({"bit_edge_groups": "2"}, (2, 0.0)), ({"code_doppler_compensation": "1"}, (1, 1575.42e6)),
                                        ({"code_doppler_compensation": "0"}, (1, 0.0))])
def test_manager_with_a_key_searches_deep_once_per_group(extra, deep):
    eng, chans, acq, trk = _acquire(extra, end_offset=-3)
    assert eng.calls["pcps"] == 0 and eng.calls["acq_deep"] == 1
    assert eng.deep_args == [([0, 1], 0, 4e6, 0.0, 5000.0, 250.0, 2, 2, deep[0], deep[1], True)]
    assert len(acq) == 2
    plain = _acquire({})[2]
    for a, ch, ref, dop in zip(acq, chans, plain, (1750.0, -3000.0)):
        assert a["bit_edge_group"] in range(deep[0]) and a["correlation_map"].shape == (41, 4000)
        assert (a["frequency_idx"], a["code_idx"]) == (ref["frequency_idx"], ref["code_idx"])    # the map's own index is reported ...
        assert a["codeOffset"] == a["code_idx"] - 3 == ch.codeOffset     # ... and peak_code_end is what tracking starts from
        assert abs(a["carrierFrequency"] - dop) <= 125.0 and ch.channelState is ChannelState.TRACKING
    assert trk


def test_two_settings_make_two_groups():
    """The settings are part of the group key: channels that differ in them are searched by separate calls."""
    fs, spms = 4e6, 4000
    raw = orc.synth_iq(fs, 6 * spms, [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=8.0)], 20.0, 99)
    eng = DeepOracleEngine()
    mgr = ChannelManager(rf_signal(fs), engine=eng)
    for extra in ({"bit_edge_groups": "1"}, {"bit_edge_groups": "2"}, {}):
        cfg = channel_config(KAPLAN_INI)
        cfg["ACQUISITION"]["non_coherent_integration"] = "2"
        cfg["ACQUISITION"].update(extra)
        mgr.addChannel(ChannelL1CA_Kaplan, cfg, 1)
    for p in (7, 7, 7):
        mgr.requestTracking(p)
    drive(mgr, raw, spms, 6)
    assert eng.calls["acq_deep"] == 2 and eng.calls["pcps"] == 1
    assert sorted(a[8] for a in eng.deep_args) == [1, 2]


def test_bad_key_values_are_refused():
    for extra in ({"bit_edge_groups": "3"}, {"bit_edge_groups": "0"}, {"code_doppler_compensation": "2"},
                  {"bit_edge_groups": "2", "non_coherent_integration": "1"}, {"bit_edge_groups": "1", "coherent_integration": "21"}):
        cfg = channel_config(KAPLAN_INI)
        cfg["ACQUISITION"].update(extra)
        mgr = ChannelManager(rf_signal(4e6), engine=DeepOracleEngine())
        with pytest.raises(ValueError):
            mgr.addChannel(ChannelL1CA_Kaplan, cfg, 1)
