"""The statement of sdr_acq_deep_detect (sydr_amd/dsp/deepsearch.py: deep_detect) on the CPU: against sdr_acq_deep's own
peak, against a brute-force loop over small random maps, its refusals, and the two tables of figures the call was built
for -- a 27 dB-Hz signal the two-peak ratio misses and the noise floor does not, and a second replica of one PRN."""
import math

import numpy as np
import pytest

import deep_cases as dc
import detect_cases as tc


@pytest.mark.parametrize("name", ["ci8_c2_k3_g2", "ci16_c1_k1_g1", "one_bin", "chirpz_4006"])
def test_peak_0_is_the_deep_searchs_peak(name):
    c, _, _, _, _ = dc.parity_input(name)
    for m in dc.parity_statement(name):
        g, b, n, _, value, _ = dc.statement_results(m, c["fs"], c)
        peaks, noise = tc.deep_detect(m, 2, 4, 1)
        p = peaks[0]
        assert (p["group"], p["bin"], p["code"], p["value"]) == (g, b, n, value)
        assert p["z"] == tc.host_z(value, noise["mean"], noise["variance"])
        assert peaks[1]["value"] <= value


def _small_maps():
    rng = np.random.default_rng(20261019)
    for G, B, N in ((1, 1, 8), (2, 5, 13), (2, 3, 16), (1, 4, 17), (2, 1, 9)):
        for _ in range(6):
            m = rng.random((G, B, N))
            # peaks pinned where zones wrap at n = 0 / N - 1 and clip at the first / the last bin, and ties (first one wins)
            m[rng.integers(G), 0, 0] = 3.0
            m[rng.integers(G), B - 1, N - 1] = 2.5
            m[0, B // 2, N // 2] = m[G - 1, B // 2, N // 2] = 2.0
            yield m


def test_zones_and_noise_cells_against_a_brute_force_loop():
    cases = 0
    for m in _small_maps():
        G, B, N = m.shape
        for n_peaks in (1, 2, 3, 8):
            for excl_code in range(0, N // 2 + 1):
                if n_peaks * (2 * excl_code + 1) >= N:
                    continue
                for excl_bins in (0, 1, B):
                    peaks, noise = tc.deep_detect(m, n_peaks, excl_code, excl_bins)
                    want, cells = tc.brute_detect(m, n_peaks, excl_code, excl_bins)
                    assert [(p["group"], p["bin"], p["code"], p["value"]) for p in peaks] == want
                    assert noise["n_cells"] == len(cells) > 0
                    values = [float(m[c]) for c in cells]
                    mean = math.fsum(values) / len(cells)
                    var = math.fsum((v - noise["mean"]) ** 2 for v in values) / len(cells)
                    assert noise["mean"] == pytest.approx(mean, rel=tc.moment_bound(len(cells)), abs=0.0)
                    assert noise["variance"] == pytest.approx(var, rel=tc.moment_bound(len(cells)), abs=0.0)
                    for p in peaks:
                        assert p["z"] == tc.host_z(p["value"], noise["mean"], noise["variance"])
                    cases += 1
    assert cases > 300


def test_a_zone_holds_every_group_and_a_noise_column_every_bin():
    m = np.arange(2 * 3 * 9, dtype=np.float64).reshape(2, 3, 9)
    m[0, 2, 8] = 52.5                   # the same (bin, code) as the maximum 53 at (1, 2, 8), in the other group
    peaks, noise = tc.deep_detect(m, 2, 1, 0)
    assert (peaks[0]["group"], peaks[0]["bin"], peaks[0]["code"]) == (1, 2, 8)
    # the zone takes codes 7, 8, 0 of bin 2 in BOTH groups: not 52.5, and not (1, 2, 7) = 52, but (1, 2, 6) = 51
    assert (peaks[1]["group"], peaks[1]["bin"], peaks[1]["code"], peaks[1]["value"]) == (1, 2, 6, 51.0)
    # columns 7, 8, 0 and 5, 6, 7 are left out in every bin and group: 4 columns x 3 bins x 2 groups
    assert noise["n_cells"] == 24 and noise["mean"] == np.mean(m[:, :, 1:5])


def test_refusals():
    m = np.ones((1, 3, 20))
    for bad in (dict(n_peaks=0), dict(n_peaks=9), dict(excl_code=-1), dict(excl_bins=-1), dict(n_peaks=4, excl_code=2),
                dict(n_peaks=1, excl_code=10)):
        a = dict(n_peaks=2, excl_code=1, excl_bins=1)
        a.update(bad)
        with pytest.raises(ValueError):
            tc.deep_detect(m, **a)
    with pytest.raises(ValueError):
        tc.deep_detect(np.ones((3, 20)), 1, 1, 1)
    tc.deep_detect(m, 3, 2, 1)          # 3 * 5 < 20


@pytest.fixture(scope="module")
def weak_table():
    """Seed -> (peaks, noise, ratio) of PRN 7 and of the absent PRN 12 on the 27 dB-Hz stream."""
    w, rows = tc.WEAK, {}
    for seed in range(8):
        x = tc.weak_stream(seed)
        row = []
        for prn in (w["prn"], w["absent"]):
            m = tc.weak_map(x, prn)
            peaks, noise = tc.deep_detect(m, w["n_peaks"], w["excl_code"], w["excl_bins"])
            row.append((peaks, noise, tc.two_peak_ratio(m, w["fs"])))
        rows[seed] = row
    return rows


def test_weak_signal_the_ratio_misses_and_the_noise_floor_finds(weak_table):
    """Regenerated here (fs = 4 MHz, C = 5, K = 40, +-500 Hz by 100 Hz, PRN 7 at 27 dB-Hz, seeds 0..7):
    peak cell [3, 2827] in all eight; ratio 1.555, 1.478, 1.639, 1.460, 1.599, 1.389, 1.515, 1.571; z_0 12.88, 11.55, 13.34,
    11.13, 13.07, 10.16, 12.38, 11.97; n_cells 43 703; absent PRN 12: largest z_0 4.97, largest ratio 1.06."""
    w = tc.WEAK
    ratios, z0, absent_z, absent_ratio = [], [], [], []
    for seed in range(8):
        (peaks, noise, ratio), (apeaks, _, aratio) = weak_table[seed]
        print(f"seed {seed}: cell [{peaks[0]['bin']}, {peaks[0]['code']}] ratio {ratio:.3f} z {[round(p['z'], 2) for p in peaks]} "
              f"n_cells {noise['n_cells']}; absent z_0 {apeaks[0]['z']:.2f} ratio {aratio:.3f}")
        assert (peaks[0]["bin"], peaks[0]["code"]) == w["cell"]
        assert noise["n_cells"] == 11 * (4000 - 3 * 9) == 43703
        ratios.append(ratio), z0.append(peaks[0]["z"]), absent_z.append(apeaks[0]["z"]), absent_ratio.append(aratio)
    assert all(z >= 7.0 for z in z0)
    assert sum(r <= 1.5 for r in ratios) >= 2
    assert all(z < 6.0 for z in absent_z)


def test_two_replicas_of_one_prn():
    """33 dB-Hz, seed 100, a second copy at 0.8, -300 Hz, 650.0 chips: peaks [3, 2827] (z 30.3) and [8, 1458] (z 19.9),
    peaks 2 and 3 at z about 4.2, ratio 2.63."""
    w, r = tc.WEAK, tc.REPLICA
    m = tc.weak_map(tc.weak_stream(r["seed"], True), w["prn"])
    peaks, noise = tc.deep_detect(m, r["n_peaks"], w["excl_code"], w["excl_bins"])
    print([(p["bin"], p["code"], round(p["z"], 2)) for p in peaks], noise, tc.two_peak_ratio(m, w["fs"]))
    assert ((peaks[0]["bin"], peaks[0]["code"]), (peaks[1]["bin"], peaks[1]["code"])) == r["cells"]
    assert peaks[1]["z"] > 7.0 and peaks[2]["z"] < 6.0


# ------------------------------------------------------------------------------------------------ the ABI
def test_detect_symbol_is_declared_bound_and_exported():
    from test_abi import declared_symbols
    from sydr_amd import _lib
    lib = _lib.load()
    assert "sdr_acq_deep_detect" in declared_symbols() and "sdr_acq_deep_detect" in _lib.exported_symbols()
    assert hasattr(lib, "sdr_acq_deep_detect") and lib.sdr_abi_version() == 5 == _lib.ABI_VERSION


def test_detect_struct_layouts(tmp_path):
    import ctypes as C
    import os
    import subprocess
    from conftest import REPO
    from sydr_amd import _lib
    assert C.sizeof(_lib.DetectCfg) == 16 and _lib.DETECT_PEAK_DTYPE.itemsize == 48 and _lib.DETECT_NOISE_DTYPE.itemsize == 24
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(sdr_detect_cfg),sizeof(sdr_detect_peak),sizeof(sdr_detect_noise),offsetof(sdr_detect_cfg,excl_bins),"
                   "offsetof(sdr_detect_peak,code_end),offsetof(sdr_detect_peak,group),offsetof(sdr_detect_peak,z),"
                   "offsetof(sdr_detect_noise,variance));return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    f, g = _lib.DETECT_PEAK_DTYPE.fields, _lib.DETECT_NOISE_DTYPE.fields
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == \
        [16, 48, 24, _lib.DetectCfg.excl_bins.offset, f["code_end"][1], f["group"][1], f["z"][1], g["variance"][1]]


# ------------------------------------------------------------------------------------------------ the plugins' keys
def _detect_engine():
    from sydr_amd import _lib
    from test_deep import DeepOracleEngine

    class DetectOracleEngine(DeepOracleEngine):
        """The oracle-backed engine with acq_deep_detect served by the statements."""

        def __init__(self):
            super().__init__()
            self.detect_args = []

        def acq_deep_detect(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh, groups=1,
                            carrier_rf_hz=0.0, n_peaks=1, excl_code=0, excl_bins=0, want_map=False):
            self.detect_args.append((list(code_slots), coh, noncoh, groups, carrier_rf_hz, n_peaks, excl_code, excl_bins))
            res, maps = DeepOracleEngine.acq_deep(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh,
                                                  noncoh, groups, carrier_rf_hz, want_map=True)
            self.calls["acq_deep"] -= 1
            peaks = np.zeros((len(code_slots), n_peaks), dtype=_lib.DETECT_PEAK_DTYPE)
            noise = np.zeros(len(code_slots), dtype=_lib.DETECT_NOISE_DTYPE)
            for k, m in enumerate(maps):
                want, nz = tc.deep_detect(m, n_peaks, excl_code, excl_bins)
                for j, p in enumerate(want):
                    end = dc.deep_code_end(p["bin"], p["code"], doppler_range, doppler_step, m.shape[2], coh, noncoh, carrier_rf_hz)
                    peaks[k, j] = (p["bin"], p["code"], end, p["group"], 0, p["value"], p["z"])
                noise[k] = (nz["n_cells"], nz["mean"], nz["variance"])
            return res, peaks, noise, (maps if want_map else None)

    return DetectOracleEngine()


def _manager(configs, prns, ms=12):
    """One channel per (ini extras, PRN) on a stream that holds PRN 7 alone."""
    from oracle import sydr_oracle as orc
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from test_host_layer import KAPLAN_INI, channel_config, drive, rf_signal
    fs, spms = 4e6, 4000
    raw = orc.synth_iq(fs, ms * spms, [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=8.0)], 20.0, 99)
    eng = _detect_engine()
    mgr = ChannelManager(rf_signal(fs), engine=eng)
    for extra in configs:
        cfg = channel_config(KAPLAN_INI)
        cfg["ACQUISITION"].update({"coherent_integration": "2", "non_coherent_integration": "2"})
        cfg["ACQUISITION"].update(extra)
        mgr.addChannel(ChannelL1CA_Kaplan, cfg, 1)
    chans = [mgr.requestTracking(p) for p in prns]
    ticks = drive(mgr, raw, spms, ms)
    return eng, mgr, chans, [p for t in ticks for p in t]


def test_manager_decides_on_sigmas_in_one_call_per_setting():
    from sydr_amd.utils.enumerations import ChannelMessage, ChannelState
    keys = {"detection_sigmas": "7", "detection_peaks": "3", "detection_exclusion_chips": "1.5", "detection_exclusion_bins": "2"}
    eng, mgr, chans, packets = _manager([keys, dict(keys, detection_sigmas="1000"), keys], (7, 7, 12))
    # equal detection settings (the sigmas apart): ONE call for the three channels; rint(1.5 * 4e6 / 1.023e6) = 6 samples
    assert eng.detect_args == [([0, 1, 2], 2, 2, 1, 0.0, 3, 6, 2)] and eng.calls["pcps"] == 0 and eng.calls["acq_deep"] == 0
    assert [ch.acq_detect for ch in chans] == [(7.0, 3, 6, 2), (1000.0, 3, 6, 2), (7.0, 3, 6, 2)]
    det = mgr.acquisitionDetections()
    assert sorted(det) == [0, 1, 2] and all(len(d["peaks"]) == 3 and d["noise"]["n_cells"] > 0 for d in det.values())
    z = [det[c]["peaks"][0]["z"] for c in range(3)]
    print(z)
    assert z[0] == z[1] > 7.0 > z[2]
    assert [det[c]["acquired"] for c in range(3)] == [True, False, False]
    assert [ch.channelState for ch in chans] == [ChannelState.TRACKING, ChannelState.IDLE, ChannelState.IDLE]
    acq = [p for p in packets if p["type"] is ChannelMessage.ACQUISITION_UPDATE]
    assert len(acq) == 3 and len({frozenset(a) for a in acq}) == 1          # rejected or not: the same keys
    assert {p["cid"] for p in packets if p["type"] is ChannelMessage.TRACKING_UPDATE} == {0}
    assert chans[0].acq_threshold == 1.5                                      # parsed as ever
    assert mgr.requestTracking(21) is chans[1]                                # a rejected channel is free again


def test_detection_joins_the_deep_keys_and_differing_settings_make_groups():
    eng, mgr, chans, _ = _manager([{"detection_sigmas": "7", "bit_edge_groups": "2", "code_doppler_compensation": "1"},
                                   {"detection_sigmas": "7"}, {"detection_sigmas": "7", "detection_peaks": "2"},
                                   {"detection_peaks": "4", "detection_exclusion_bins": "3"}], (7, 7, 7, 7))
    assert sorted(eng.detect_args) == sorted([([0], 2, 2, 2, 1575.42e6, 1, 4, 1), ([1], 2, 2, 1, 0.0, 1, 4, 1),
                                              ([2], 2, 2, 1, 0.0, 2, 4, 1)])
    # without detection_sigmas the other keys switch nothing on: the reference's search, no detection kept
    assert eng.calls["pcps"] == 1 and chans[3].acq_detect is None and sorted(mgr.acquisitionDetections()) == [0, 1, 2]


def test_bad_detection_keys_are_refused():
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from test_host_layer import KAPLAN_INI, channel_config, rf_signal
    for extra in ({"detection_sigmas": "0"}, {"detection_sigmas": "-1"}, {"detection_sigmas": "nan"},
                  {"detection_sigmas": "7", "detection_peaks": "0"}, {"detection_sigmas": "7", "detection_peaks": "9"},
                  {"detection_sigmas": "7", "detection_exclusion_chips": "-1"}, {"detection_sigmas": "7", "detection_exclusion_bins": "-1"},
                  {"detection_sigmas": "7", "coherent_integration": "21"}, {"detection_sigmas": "7", "detection_exclusion_chips": "512"},
                  {"detection_sigmas": "7", "bit_edge_groups": "2", "non_coherent_integration": "1"}):
        cfg = channel_config(KAPLAN_INI)
        cfg["ACQUISITION"].update(extra)
        mgr = ChannelManager(rf_signal(4e6), engine=_detect_engine())
        with pytest.raises(ValueError):
            mgr.addChannel(ChannelL1CA_Kaplan, cfg, 1)
