"""Pins the CPU oracle (oracle/sydr_oracle.py) to golden vectors captured from the reference
itself (tests/golden/make_golden.py).  CPU only; runs anywhere."""
import functools
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from oracle import sydr_oracle as orc


# ------------------------------------------------------------------------------------------------ G1 / G2
def test_gold_codes_match_reference():
    g = load_golden("g1_codes.npz")
    for prn, chips, octal in zip(g["prns"], g["chips"], g["first10"]):
        code = orc.gold_code(int(prn))
        assert code.dtype == np.float64
        assert np.array_equal(code.astype(np.int8), chips), f"PRN {prn}"
        assert orc.first_10_chips_octal(int(prn)) == int(octal)


def test_every_gold_code_matches_reference():
    """All 210 PRNs of the G2 delay table (g1_codes.npz holds 42 of them), one bit per chip."""
    g = load_golden("g1_codes_all.npz")
    assert list(g["prns"]) == list(range(1, 211)) and g["packed"].shape == (210, 128)
    chips = np.unpackbits(g["packed"], axis=1)[:, :1023].astype(np.int8) * 2 - 1
    old = load_golden("g1_codes.npz")
    for prn, row in zip(old["prns"], old["chips"]):
        assert np.array_equal(chips[int(prn) - 1], row), f"PRN {prn}"
    for prn in range(1, 211):
        assert np.array_equal(orc.gold_code(prn).astype(np.int8), chips[prn - 1]), f"PRN {prn}"
    assert len({row.tobytes() for row in chips}) == 209          # (PRN 34 and 37 share a delay; every other code is its own)


def test_first_ten_chips_icd_table():
    # IS-GPS-200 table, PRN 1..10 (also printed by the reference's ca.py:137-149)
    expect = [0o1440, 0o1620, 0o1710, 0o1744, 0o1133, 0o1455, 0o1131, 0o1454, 0o1626, 0o1504]
    assert [orc.first_10_chips_octal(p) for p in range(1, 11)] == expect


@pytest.mark.parametrize("fs", [4e6, 10e6, 12e6, 25e6, 50e6])
def test_upsample_index_bit_exact(fs):
    g = load_golden("g1_codes.npz")
    ref = g[f"upsample_idx_{int(fs)}"]
    assert np.array_equal(orc.upsample_index(fs), ref)
    assert orc.samples_per_code(fs) == len(ref)


# ------------------------------------------------------------------------------------------------ G3
@pytest.mark.parametrize("tag", ["a", "b", "c", "d", "e", "f"])
def test_pcps_matches_reference(tag):
    g = load_golden("g3_pcps.npz")
    fs, if_hz, rng_hz, step, coh, noncoh, n, spc = g[f"{tag}_params"]
    coh, noncoh, n, spc = int(coh), int(noncoh), int(n), int(spc)
    rf = orc.iq_to_complex(g[f"{tag}_iq"]).reshape(1, -1)
    for k, prn in enumerate(g[f"{tag}_prns"]):
        spec = orc.code_spectrum(orc.gold_code(int(prn)), fs)
        cmap = orc.pcps_map(rf, if_hz, fs, spec, rng_hz, step, n, coh, noncoh)
        peak, ratio = orc.two_peak_compare(cmap, n, spc)
        assert peak == list(g[f"{tag}_peak"][k])
        # same NumPy primitives in the same order: bit-identical on the build host
        np.testing.assert_allclose(cmap[peak[0]], g[f"{tag}_row"][k], rtol=1e-13, atol=0)
        np.testing.assert_allclose(cmap[:, peak[1]], g[f"{tag}_col"][k], rtol=1e-13, atol=0)
        np.testing.assert_allclose(cmap.sum(axis=1), g[f"{tag}_binsum"][k], rtol=1e-13)
        assert ratio == pytest.approx(float(g[f"{tag}_ratio"][k]), rel=1e-13)


def test_doppler_grid_lengths():
    # float range/step -> 41 bins @250, 101 @100, 34 @300 (asymmetric)
    assert len(orc.doppler_bins(5000.0, 250.0)) == 41
    assert len(orc.doppler_bins(5000.0, 100.0)) == 101
    b = orc.doppler_bins(5000.0, 300.0)
    assert len(b) == 34 and b[-1] == 4900.0


# ------------------------------------------------------------------------------------------------ G4
def test_two_peak_compare_edge_cases():
    g = load_golden("g4_peaks.npz")
    n, bins, spc = (int(v) for v in g["geometry"])
    for m, idx, ratio in zip(g["maps"], g["idx"], g["ratio"]):
        got_idx, got_ratio = orc.two_peak_compare(m.copy(), n, spc)
        assert got_idx == list(idx)
        assert got_ratio == ratio


# ------------------------------------------------------------------------------------------------ G5 / G8
def test_epl_reference_fixture():
    """The reference's own unit-test input (sydr/unitTest/data/i_rfdata.txt: PRN 2, 3700 Hz, 10 MHz)."""
    g = load_golden("g5_epl.npz")
    prn, fs, f, rc, rk, step = g["fixture_params"]
    rf = orc.iq_to_complex(g["fixture_iq"])
    out = orc.epl(rf, orc.pad_code(orc.gold_code(int(prn))), fs, f, rc, rk, step, (-0.5, 0.0, 0.5))
    assert np.array_equal(np.array(out), g["fixture_out"])
    # values quoted in SURVEY.md 8c (probe of the reference)
    np.testing.assert_allclose(out, [-209.48629766813846, -4378.819831485676, -2771.533819861607,
                                     -2997.4691729749657, -924.5637349695502, -3715.3502647689807], rtol=1e-12)


def test_epl_random_cases():
    g = load_golden("g5_epl.npz")
    for tag in g["cases"]:
        prn, fs, f, rc, rk, step, n = g[f"{tag}_params"]
        rf = orc.iq_to_complex(g[f"{tag}_iq"])
        assert len(rf) == int(n)
        sp = tuple(g[f"{tag}_spacing"])
        out = orc.epl(rf, orc.pad_code(orc.gold_code(int(prn))), fs, f, rc, rk, step, sp)
        assert np.array_equal(np.array(out), g[f"{tag}_out"]), tag
        for t, s in enumerate(sp):
            assert np.array_equal(orc.epl_indices(int(n), rk, step, s), g[f"{tag}_idx"][t]), tag


def test_epl_periodic_extension_reduces_to_padded_table():
    """The oracle's generalisation (taps beyond +-1 chip wrap periodically) must not change E/P/L."""
    g = load_golden("g5_epl.npz")
    prn, fs, f, rc, rk, step, n = g["r10_params"]
    rf = orc.iq_to_complex(g["r10_iq"])
    code = orc.pad_code(orc.gold_code(int(prn)))
    five = orc.epl(rf, code, fs, f, rc, rk, step, (-1.0, -0.5, 0.0, 0.5, 1.0))
    assert np.array_equal(np.array(five[2:8]), g["r10_out"])


def test_replica_known_answers():
    """sydr/c_functions/tracking.c:243-247: fs=1e7, f=-1500 Hz, 5 samples, eps 1e-8."""
    g = load_golden("g5_epl.npz")
    truth = np.array([1 + 0j, 0.9999995558678348 + 0.000942477656548699j, 0.9999982234717338 + 0.0018849544759281136j,
                      0.9999960028128805 + 0.002827429620969703j, 0.9999928938932473 + 0.0037699022545064132j])
    assert np.max(np.abs(g["replica_known"] - truth)) < 1e-8
    # our EPL with a constant +1 "code" and unit samples reproduces the replica sum
    ones = np.ones(5, dtype=complex)
    out = orc.epl(ones, np.ones(1025), 1e7, -1500.0, 0.0, 0.0, 0.1, (0.0,))
    assert complex(out[0], out[1]) == pytest.approx(truth.sum(), rel=1e-9)


# ------------------------------------------------------------------------------------------------ G7
def test_scalar_loop_math():
    g = load_golden("g7_loopmath.npz")
    c = g["inputs"]
    with np.errstate(all="ignore"):
        for k, r in enumerate(c):
            assert orc.dll_nneml(r[0], r[1], r[4], r[5]) == g["dll"][k]
            np.testing.assert_equal(orc.pll_costas(r[2], r[3]), g["pll"][k])
            np.testing.assert_equal(orc.fll_atan(r[2], r[3], r[6], r[7], 1e-3), g["fll"][k])
            np.testing.assert_equal(orc.fll_lock_borre(r[2], r[6], r[3], r[7], 0.3, alpha=0.005), g["fll_lock"][k])
            np.testing.assert_equal(orc.pll_lock_borre(r[2], r[3], 0.4, alpha=0.005), g["pll_lock"][k])
            assert orc.cn0_beaulieu(abs(r[0]) * 1e-3 + 1.0, 20, 20e-3, abs(r[1]) * 1e-3) == g["cn0"][k]
            assert orc.borre_filter(r[0] * 1e-5, r[1] * 1e-5, g["coeff"][0, 0], g["coeff"][0, 1], 0.001) == \
                g["borre_filter"][k]
            assert list(orc.fll_assisted_pll_2nd(r[0] * 1e-6, r[1] * 1e-3, 100.0 / 0.25, 25.0 / 0.53, 1.414, 1e-3,
                                                 r[2] * 1e-4)) == list(g["fll_pll"][k])
    for k, (b, z, gain) in enumerate(((2.0, 0.7, 1.0), (1.0, 0.7, 1.0), (8.0, 0.7, 0.25), (15.0, 0.7, 1.5))):
        assert list(orc.loop_coefficients(b, z, gain)) == list(g["coeff"][k])


def test_host_loop_math_drop_ins_match_the_reference():
    """sydr_amd.dsp.tracking / lockindicator host functions (the reference's names and signatures) against the same
    captured values, bit for bit -- including the atan(+-inf) and 0/0 rows."""
    from sydr_amd.dsp import lockindicator as li
    from sydr_amd.dsp import tracking as trk
    g = load_golden("g7_loopmath.npz")
    with np.errstate(all="ignore"):
        for k, r in enumerate(g["inputs"]):
            assert trk.DLL_NNEML(r[0], r[1], r[4], r[5]) == g["dll"][k]
            np.testing.assert_equal(trk.PLL_costa(r[2], r[3]), g["pll"][k])
            np.testing.assert_equal(trk.FLL_ATAN(r[2], r[3], r[6], r[7], 1e-3), g["fll"][k])
            np.testing.assert_equal(li.FLL_Lock_Borre(r[2], r[6], r[3], r[7], 0.3, alpha=0.005), g["fll_lock"][k])
            np.testing.assert_equal(li.PLL_Lock_Borre(r[2], r[3], 0.4, alpha=0.005), g["pll_lock"][k])
            assert li.CN0_Beaulieu(abs(r[0]) * 1e-3 + 1.0, 20, 20e-3, abs(r[1]) * 1e-3) == g["cn0"][k]
            assert trk.BorreLoopFilter(r[0] * 1e-5, r[1] * 1e-5, g["coeff"][0, 0], g["coeff"][0, 1], 0.001) == \
                g["borre_filter"][k]
            assert list(trk.FLLassistedPLL_2ndOrder(r[0] * 1e-6, r[1] * 1e-3, 100.0 / 0.25, 25.0 / 0.53, 1.414, 1e-3,
                                                    r[2] * 1e-4)) == list(g["fll_pll"][k])
    for k, (b, z, gain) in enumerate(((2.0, 0.7, 1.0), (1.0, 0.7, 1.0), (8.0, 0.7, 0.25), (15.0, 0.7, 1.5))):
        assert list(trk.LoopFiltersCoefficients(b, z, gain)) == list(g["coeff"][k])
    # legacy pieces: the replica known answers captured from the reference's generateReplica (g5), and one tap of
    # getCorrelator against the oracle's index rule
    g5 = load_golden("g5_epl.npz")
    rep, rem = trk.generateReplica(np.arange(0, 6) / 1e7, 5, -1500.0, 0.0)
    assert np.array_equal(rep, g5["replica_known"]) and rem == float(g5["replica_rem"])
    rng = np.random.default_rng(5)
    i_sig, q_sig = rng.normal(size=4001), rng.normal(size=4001)
    code = orc.pad_code(orc.gold_code(9))
    idx = orc.epl_indices(4001, 0.1, 0.25575, 0.5)
    assert trk.getCorrelator(i_sig, q_sig, 0.5, code, 0.1, 0.25575, 4001) == (np.sum(code[idx] * i_sig),
                                                                            np.sum(code[idx] * q_sig))
    # third order: collapses onto the second-order arithmetic when the extra terms vanish
    out3, vel3, acc3 = trk.FLLassistedPLL_3rdOrder(0.01, 0.5, 0.0, 10.0, 1.414, 0.0, 1.414, 1e-3, 0.25, 0.0)
    assert acc3 == (0.01 * 10.0**3) * 1e-3 and vel3 == (acc3 + 0.0) * 1e-3 and out3 == vel3 + 0.25 + 0.01 * 1.414 * 10.0
    assert li.CN0_NWPR(30.0, 4.0, 60.0, 2.0) == 10 * np.log10(1e3 * ((900.0 + 16.0) / 62.0 - 1) / (20 - (900.0 + 16.0) / 62.0))
    assert li.lowPassFilter(2.0, 1.0, 0.25) == 1.25


# ------------------------------------------------------------------------------------------------ G6
BORRE_CFG = dict(correlator_early=-0.5, correlator_prompt=0.0, correlator_late=0.5, dll_damping_ratio=0.7,
                 dll_noise_bandwidth=1.0, dll_loop_gain=1.0, dll_pdi=0.001, pll_damping_ratio=0.7,
                 pll_noise_bandwidth=8.0, pll_loop_gain=0.25, pll_pdi=0.001)
KAPLAN_CFG = dict(correlator_epl_wide=0.5, correlator_epl_narrow=0.5, dll_threshold=10.0, dll_damping_ratio=0.7,
                  dll_noise_bandwidth=2.0, dll_loop_gain=1.0, dll_pdi=0.001, pll_bandwidth_wide=25.0,
                  pll_bandwidth_narrow=15.0, pll_threshold_wide=0.5, pll_threshold_narrow=0.8,
                  fll_bandwidth_pullin=100.0, fll_bandwidth_wide=50.0, fll_bandwidth_narrow=15.0,
                  fll_threshold_wide=0.5, fll_threshold_narrow=0.8)


@functools.lru_cache(maxsize=4)
def trajectory_iq(fname="g6_trajectories.npz"):
    g = load_golden(fname)
    fs, n, prn, dop, cph, ph, amp, sigma, seed = g["synth"]
    raw = orc.synth_iq(fs, int(n), [dict(prn=int(prn), doppler=dop, code_phase=cph, phase=ph, amp=amp)], sigma,
                       int(seed))
    digest = np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8)
    assert np.array_equal(digest, g["iq_sha256"]), "seeded IQ differs from the one the golden run used"
    return g, fs, raw


@pytest.mark.parametrize("fname", ["g6_trajectories.npz", "g6c_25mhz.npz"])
@pytest.mark.parametrize("plugin", ["borre", "kaplan"])
def test_closed_loop_trajectory(plugin, fname):
    """BASELINE config 1: 1 channel, 4 MHz, 1 ms PCPS + ~500 ms tracking, vs the reference plugin -- and the same at
    the headline rate of configs 2-3 (25 MHz, ~300 epochs)."""
    g, fs, raw = trajectory_iq(fname)
    rf = orc.iq_to_complex(raw)
    n_code, spc = orc.samples_per_code(fs), round(fs / orc.CODE_RATE)
    code = orc.gold_code(7)
    cmap = orc.pcps_map(rf[:n_code].reshape(1, -1), 0.0, fs, orc.code_spectrum(code, fs), 5000.0, 250.0, n_code)
    peak, ratio = orc.two_peak_compare(cmap, n_code, spc)
    acq = g[f"{plugin}_acq"]
    assert peak == [int(acq[0]), int(acq[1])]
    assert ratio == pytest.approx(acq[2], rel=1e-13)
    track0 = orc.required_samples(0.0, orc.CODE_RATE / fs)
    assert track0 == (4001 if fs == 4e6 else 25000)
    carrier, offset, cur = orc.post_acquisition(0.0, 5000.0, 250.0, peak, 0, n_code, track0)
    assert (carrier, offset, cur, track0) == (acq[3], int(acq[4]), int(acq[5]), int(acq[6]))

    loop = (orc.BorreLoop(fs, code, BORRE_CFG, carrier, cur) if plugin == "borre"
            else orc.KaplanLoop(fs, code, KAPLAN_CFG, carrier, cur))
    ref = g[f"{plugin}_epochs"]
    ring = 100 * int(fs * 1e-3)
    for k, row in enumerate(ref):
        # the reference indexes a 100 ms ring; absolute position = ring index + wraps
        assert loop.current_sample % ring == int(row[0]), k
        assert loop.n == int(row[1]), k
        assert (loop.carrier_hz, loop.rem_carrier, loop.rem_code, loop.code_step) == tuple(row[2:6]), k
        rec = loop.step(rf[loop.current_sample:loop.current_sample + loop.n])
        assert rec["corr"] == list(row[6:12]), k
        assert rec["carrier_hz"] == row[15] and rec["code_hz"] == row[16], k
        assert rec["nav_bit"] == int(row[24]), k     # navigation bit closed by this epoch (or -1)
        if plugin == "kaplan":
            assert (rec["dll"], rec["pll"], rec["fll"]) == tuple(row[12:15]), k
            np.testing.assert_equal([rec["cn0"], rec["pll_lock"], rec["fll_lock"]], row[19:22])
            assert (rec["lock_state"], rec["flags"]) == (int(row[22]), int(row[23])), k
    assert len(ref) >= (500 if fs == 4e6 else 300)


def kaplan_strong_cfg(g):
    cfg = dict(KAPLAN_CFG)
    for k, v in zip(g["track_override_keys"], g["track_override_vals"]):
        cfg[str(k)] = float(v)
    return cfg


def test_closed_loop_kaplan_lock_state_machine():
    """Strong signal + lowered thresholds: PULL_IN -> WIDE -> NARROW (narrow taps), code lock, bit sync."""
    g, fs, raw = trajectory_iq("g6b_kaplan_strong.npz")
    rf = orc.iq_to_complex(raw)
    acq = g["kaplan_acq"]
    loop = orc.KaplanLoop(fs, orc.gold_code(7), kaplan_strong_cfg(g), acq[3], int(acq[5]))
    ref = g["kaplan_epochs"]
    ring = 100 * int(fs * 1e-3)
    for k, row in enumerate(ref):
        assert (loop.current_sample % ring, loop.n) == (int(row[0]), int(row[1])), k
        rec = loop.step(rf[loop.current_sample:loop.current_sample + loop.n])
        assert rec["corr"] == list(row[6:12]), k
        assert (rec["carrier_hz"], rec["code_hz"], rec["dll"], rec["pll"], rec["fll"]) == \
            (row[15], row[16], row[12], row[13], row[14]), k
        np.testing.assert_equal([rec["cn0"], rec["pll_lock"], rec["fll_lock"]], row[19:22])
        assert (rec["lock_state"], rec["flags"]) == (int(row[22]), int(row[23])), k
        assert rec["nav_bit"] == int(row[24]), k
    assert {int(r[22]) for r in ref} == {1, 2, 3} and int(ref[-1][23]) == 3
    assert loop.nav_bits == [int(b) for b in ref[ref[:, 24] >= 0, 24]] and len(loop.nav_bits) >= 40


def test_closed_loop_kaplan_every_lock_edge():
    """The seeded starts of tests/lock_edge_cases.py (cases A-G) in the reference's own plugin (g6d): the downward edges
    3>2, 3>1, 2>1, the direct 1>3, a fallen-back PULL_IN, CODE_LOCK cleared with bits still coming -- branches of
    KaplanLoop that no healthy trajectory takes.  The oracle from the same seeded state, bit for bit."""
    import lock_edge_cases as lec
    g = load_golden("g6d_kaplan_edges.npz")
    raw, stream, (carrier, cur) = lec.cpu_scene()
    assert np.array_equal(np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8), g["iq_sha256"])
    assert {str(k): float(v) for k, v in zip(g["track_override_keys"], g["track_override_vals"])} == lec.OVERRIDES
    assert tuple(str(c) for c in g["cases"]) == lec.GOLDEN_CASES
    ring = 100 * int(lec.FS_CPU * 1e-3)
    edges = set()
    for name in lec.GOLDEN_CASES:
        acq, ref = g[f"{name}_acq"], g[f"{name}_epochs"]
        assert (carrier, cur) == (acq[3], int(acq[5]))
        state, recs, aux, end, bits = lec.cpu_run(name)
        # the golden run started from the state the case module builds today
        assert [float(getattr(state, str(f))) for f in g["seed_fields"]] == list(g[f"{name}_seed"]), name
        assert len(ref) == len(recs) == lec.EPOCHS
        for k, (row, rec) in enumerate(zip(ref, recs)):
            assert (rec["start"] % ring, rec["n"]) == (int(row[0]), int(row[1])), (name, k)
            assert (rec["carrier_hz_in"], rec["rem_carrier_in"], rec["rem_code_in"], rec["code_step_in"]) == tuple(row[2:6]), (name, k)
            assert rec["corr"] == list(row[6:12]), (name, k)
            assert (rec["dll"], rec["pll"], rec["fll"], rec["carrier_hz"], rec["code_hz"], rec["carrier_err"], rec["code_err"]) \
                == tuple(row[12:19]), (name, k)
            np.testing.assert_equal([rec["cn0"], rec["pll_lock"], rec["fll_lock"]], row[19:22])
            assert (rec["lock_state"], rec["flags"], rec["nav_bit"]) == (int(row[22]), int(row[23]), int(row[24])), (name, k)
        assert list(bits) == [int(b) for b in ref[ref[:, 24] >= 0, 24]]
        edges |= lec.observed_edges(state, recs, aux)
    assert lec.ALL_EDGES <= edges           # (H, the Borre case, adds none of its own)


def test_lock_edge_cases_keep_their_conditions():
    """tests/lock_edge_cases.py's own checks, as part of the suite: every case shows the edges it is there for, all
    together show every edge, and the seeds in use pass the 1e-13 perturbation check."""
    import lock_edge_cases as lec
    for name in lec.CASES:
        lec.test_each_case_shows_its_edges(name)
        lec.test_seeds_pass_the_perturbation_check(name)
        lec.test_decisions_keep_clear_of_their_thresholds(name)
    lec.test_all_edges_are_covered()


@pytest.mark.parametrize("plugin", ["borre", "kaplan_strong"])
def test_generalised_loop_reduces_to_the_reference(plugin):
    """Configs 4-5 run 5 taps / multi-period epochs / BOC through the loops' generalised arguments (no reference
    counterpart).  With the reference's constants spelled out, and with two outer taps added around the reference's
    E/P/L, the generalised loop must reproduce the golden trajectory bit for bit: the outer taps are only correlated."""
    g, fs, raw = trajectory_iq("g6_trajectories.npz" if plugin == "borre" else "g6b_kaplan_strong.npz")
    rf = orc.iq_to_complex(raw)
    code = orc.gold_code(7)
    if plugin == "borre":
        acq, ref = g["borre_acq"], g["borre_epochs"]
        five = [-1.0, -0.5, 0.0, 0.5, 1.0]
        loop = orc.BorreLoop(fs, code, BORRE_CFG, acq[3], int(acq[5]), taps=(five, five), epoch_chips=1023,
                             epochs_per_bit=20, code_rate=1.023e6)
    else:
        acq, ref = g["kaplan_acq"], g["kaplan_epochs"]
        c = kaplan_strong_cfg(g)
        w, n = c["correlator_epl_wide"], c["correlator_epl_narrow"]
        loop = orc.KaplanLoop(fs, code, c, acq[3], int(acq[5]), taps=([-2 * w, -w, 0.0, w, 2 * w], [-2 * n, -n, 0.0, n, 2 * n]),
                              epoch_chips=1023, epochs_per_bit=20, dt=1e-3, code_rate=1.023e6)
    for k, row in enumerate(ref[:260]):
        assert loop.n == int(row[1]), k
        rec = loop.step(rf[loop.current_sample:loop.current_sample + loop.n])
        assert len(rec["corr"]) == 10 and rec["corr"][2:8] == list(row[6:12]), k
        assert rec["carrier_hz"] == row[15] and rec["code_hz"] == row[16], k
        assert rec["nav_bit"] == int(row[24]) and rec["flags"] == int(row[23]), k
        if plugin != "borre":
            assert rec["lock_state"] == int(row[22]), k


# ------------------------------------------------------------------------------------------------ G9 SerialSearch
def test_serial_search_matches_reference():
    g = load_golden("g9_serial.npz")
    fs, n, prn, rng_hz, step = g["params"]
    rf = orc.iq_to_complex(g["iq"])
    code = orc.gold_code(int(prn))
    m0 = orc.serial_search(rf[:int(n)].reshape(1, -1), code, rng_hz, step, fs, int(n))
    assert np.array_equal(m0, g["map0"])
    idx, ratio = orc.two_peak_compare_ss(m0)
    assert idx == list(g["peak"]) and ratio == float(g["ratio"])
    for m, i, q in zip(g["edge_maps"], g["edge_idx"], g["edge_ratio"]):
        gi, gq = orc.two_peak_compare_ss(m)
        assert gi == list(i) and gq == q


# ------------------------------------------------------------------------------------------------ G9b rates where the index rounds
def test_upsample_index_bit_exact_where_rounding_matters():
    """below, at and at whole multiples of the chip rate (tests/serial_cases.py): at five of the eight rates the reference's
    floating-point index differs from the exact quotient's for some samples, and the oracle's is the reference's"""
    import serial_cases as sc
    g = load_golden("g9b_serial_rates.npz")
    assert list(g["rates"]) == [r.fs for r in sc.RATES]
    differing = 0
    for rate in sc.RATES:
        ref = g[f"upsample_idx_{int(rate.fs)}"]
        assert ref.dtype == np.int16 and len(ref) == rate.n == orc.samples_per_code(rate.fs)
        assert np.array_equal(orc.upsample_index(rate.fs), ref)
        assert np.count_nonzero(ref != sc.exact_index(rate.fs)) == rate.sensitive
        differing += rate.sensitive > 0
    assert differing == 5


def test_serial_search_matches_reference_where_rounding_matters():
    g = load_golden("g9b_serial_rates.npz")
    code = orc.gold_code(int(g["prn"]))
    for fs in g["map_rates"]:
        raw = g[f"iq_{int(fs)}"]
        n = orc.samples_per_code(float(fs))
        assert len(raw) == 2 * n
        m = orc.serial_search(orc.iq_to_complex(raw).reshape(1, -1), code, *g["grid"], float(fs), n)
        np.testing.assert_allclose(m, g[f"map_{int(fs)}"], rtol=1e-13, atol=0)
    # a 2046-chip code at 2.046 MHz, one bin: the chips past 1022 enter through the circular shift alone
    fs = 2.046e6
    long_code = g["long_code"].astype(np.float64)
    assert len(long_code) == 2046
    m = orc.serial_search(orc.iq_to_complex(g[f"iq_{int(fs)}"]).reshape(1, -1), long_code, *g["long_grid"], fs, 2046)
    assert m.shape == (2046,)
    np.testing.assert_allclose(m, g["long_map"], rtol=1e-13, atol=0)
