"""The NumPy statement of sdr_pcps_signal (sydr_amd/dsp/signalsearch.py pcps_signal_statement), host only, no library:
with the C/A descriptor it is the oracle's PCPS bit for bit, and in the flip scenario -- seeded +-1 codes, amplitude 6 under
noise of sigma 20 per axis, the code starting at N/2 + 37, the sign changing at every period, -500 Hz on +-1000 by 250 Hz -- the
zero-padded search returns the true bin and code sample where the circular one lands in another bin."""
import numpy as np
import pytest

import signal_search_cases as sc
from oracle import sydr_oracle as orc
from sydr_amd.dsp import signalsearch as ss


@pytest.mark.parametrize("coh,noncoh", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_ca_descriptor_is_the_oracles_pcps(coh, noncoh):
    fs, prns = 4e6, (7, 19)
    n_code = orc.samples_per_code(fs)
    raw = orc.synth_iq(fs, 4 * n_code, [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=8.0),
                                        dict(prn=19, doppler=-2250.0, code_phase=811.5, phase=0.7, amp=7.0)], 20.0, 20260001)
    rf = orc.iq_to_complex(raw)
    codes = np.stack([orc.gold_code(p) for p in prns])
    pb, pc, pr, cmap = ss.pcps_signal_statement(rf, codes, fs, 0.0, 5000.0, 250.0, 1.023e6, pad=0, excl_samples=0, coh=coh,
                                                noncoh=noncoh)
    assert cmap.shape == (2, 41, n_code) and ss.samples_per_code(fs, 1023, 1.023e6) == n_code
    for i, code in enumerate(codes):
        assert np.array_equal(ss.replica(code, fs, 1.023e6), orc.upsample_code(code, fs))
        ref = orc.pcps_map(rf, 0.0, fs, orc.code_spectrum(code, fs), 5000.0, 250.0, n_code, coh, noncoh)
        assert np.array_equal(cmap[i], ref)
        peak, ratio = orc.two_peak_compare(ref, n_code, round(fs / orc.CODE_RATE))
        assert [int(pb[i]), int(pc[i])] == peak and pr[i] == ratio


def test_window_wraps_and_starts_anywhere():
    """start_sample and the wrap at the ring's end: the same samples laid out flat give the same bits."""
    raw, codes = sc.scene("c_2038", 1, 3)
    x = sc.to_complex(raw)
    start = 2 * 2038 + 501                              # two periods from here cross the end
    flat = np.roll(x, -start)
    for pad in (0, 1):
        a = ss.pcps_signal_statement(x, codes, 2.038e6, 0.0, sc.RANGE, sc.STEP, 1.023e6, pad=pad, start_sample=start)
        b = ss.pcps_signal_statement(flat, codes, 2.038e6, 0.0, sc.RANGE, sc.STEP, 1.023e6, pad=pad)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_replica_and_lengths():
    # half-even, the chip rate a parameter, the last chip held where rounding runs past the code
    assert ss.samples_per_code(4.092e6, 4092, 1.023e6) == 16368 and ss.samples_per_code(4e6, 8184, 2.046e6) == 16000
    assert ss.samples_per_code(2.038e6, 1023, 1.023e6) == 2038
    assert ss.samples_per_code(2500.0, 1, 1000.0) == 2 and ss.samples_per_code(3500.0, 1, 1000.0) == 4
    code = np.arange(1, 11)
    r = ss.replica(code, 3.0, 1.0)
    assert r.size == 30 and np.array_equal(r, np.repeat(code, 3))
    assert ss.replica(code, 3.0, 1.0, 33)[-1] == 10
    assert np.array_equal(ss.boc_doubled([1, -1, 1]), [1, -1, -1, 1, 1, -1])


@pytest.mark.parametrize("name", list(sc.GEOMETRIES))
def test_flip_scenario_padded_finds_what_circular_misses(name):
    raw, codes = sc.scene(name, 1, 4)
    for noncoh in (1, 3):
        pb, pc, pr, cmap = sc.statement(name, raw, codes, 1, noncoh)
        assert cmap.shape[2] == sc.GEOMETRIES[name][3]
        assert (int(pb[0]), int(pc[0])) == (sc.TRUE_BIN, sc.code_start(name)), (name, noncoh)
        cb, cc, cr, _ = sc.statement(name, raw, codes, 0, noncoh)
        print(f"{name} noncoh {noncoh}: padded bin {pb[0]} code {pc[0]} ratio {pr[0]:.2f}; circular bin {cb[0]} code {cc[0]} "
              f"ratio {cr[0]:.2f}")
        assert int(cb[0]) != sc.TRUE_BIN, (name, noncoh)
        assert pr[0] > cr[0]


def test_padded_map_is_the_linear_correlation():
    """Lag n < N of the padded search is sum_m y[n + m] r[m] over one whole replica -- no wrap: computed directly for a few lags."""
    name = "c_2038"
    fs, chips, rate, n_code, _, _ = sc.GEOMETRIES[name]
    raw, codes = sc.scene(name, 1, 2)
    x = sc.to_complex(raw)
    _, _, _, cmap = sc.statement(name, raw, codes, 1)
    rep = ss.replica(codes[0].astype(np.float64), fs, rate, n_code)
    bins = np.arange(-sc.RANGE, sc.RANGE + 1, sc.STEP)
    for b in (0, sc.TRUE_BIN):
        y = x[:2 * n_code] * np.exp(-1j * (0.0 - bins[b]) * (np.arange(2 * n_code) * 2 * np.pi / fs))
        for lag in (0, 1, sc.code_start(name), n_code - 1):
            direct = abs(np.sum(y[lag:lag + n_code] * rep)) / 1.0
            assert abs(cmap[0, b, lag] - direct) <= 1e-9 * cmap.max()
