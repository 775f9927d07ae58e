"""The per-epoch replay helper (tests/track_replay.py) pinned on the CPU: replaying the oracle loops' own records must give
their correlators bit for bit, their spacing and their NCO hand-over, through a linear stream and through a ring shorter
than the stream; the core classifier gives the known answers on both sides of every threshold and guard."""
import math

import numpy as np
import pytest

from oracle import sydr_oracle as orc
from test_oracle_golden import BORRE_CFG, KAPLAN_CFG, kaplan_strong_cfg, trajectory_iq

import track_replay as tr

GOLDEN = {"g6": "g6_trajectories.npz", "g6b": "g6b_kaplan_strong.npz", "g6c": "g6c_25mhz.npz"}


def _oracle_run(name, kind, epochs, rf=None):
    g, fs, raw = trajectory_iq(GOLDEN[name])
    rf = orc.iq_to_complex(raw) if rf is None else rf
    acq = g["kaplan_acq" if kind == 1 else "borre_acq"]
    c = (kaplan_strong_cfg(g) if name == "g6b" else KAPLAN_CFG) if kind == 1 else BORRE_CFG
    loop = (orc.KaplanLoop if kind == 1 else orc.BorreLoop)(fs, orc.gold_code(7), c, acq[3], int(acq[5]))
    n0 = loop.n
    recs = [loop.step(rf[loop.current_sample:loop.current_sample + loop.n]) for _ in range(epochs)]
    wide, narrow = (loop.sp_wide, loop.sp_narrow) if kind == 1 else (loop.spacing, loop.spacing)
    return fs, rf, recs, wide, narrow, n0


@pytest.mark.parametrize("name,kind", [("g6", 0), ("g6", 1), ("g6b", 1), ("g6c", 0), ("g6c", 1)])
def test_replay_reproduces_the_oracle_loops_bit_for_bit(name, kind):
    epochs = {"g6": 300, "g6b": 600, "g6c": 120}[name]      # (g6b enters NARROW at epoch 447)
    fs, rf, recs, wide, narrow, n0 = _oracle_run(name, kind, epochs)
    cols = tr.columns(recs)
    taps = tr.spacings(cols, kind, wide, narrow)
    if kind == 1:
        assert [list(t) for t in taps] == [r["spacing"] for r in recs]
    expected, scale = tr.replay(cols, rf, fs, orc.gold_code(7), taps)
    assert np.array_equal(expected, cols["corr"])
    assert np.all(tr.tap_ratios(cols["corr"], expected, scale) == 0.0) and np.all(scale > 0)
    assert tr.check_nco(cols, fs, kind, n0=n0) == []
    if name == "g6b":     # the strong stream reaches NARROW: both spacings were replayed
        assert {tuple(t) for t in taps} == {tuple(wide), tuple(narrow)} and tuple(wide) != tuple(narrow)


def test_replay_through_a_ring_shorter_than_the_stream():
    """The 4 MHz stream made periodic with a period of `cap` samples, tracked linearly by the oracle's loop, replayed from a
    ring of `cap` samples addressed modulo its capacity: every epoch bit for bit, the ones that wrap included."""
    g, fs, raw = trajectory_iq(GOLDEN["g6b"])
    rf = orc.iq_to_complex(raw)
    cap = 37 * 4000 + 8
    ring = rf[:cap].copy()
    stream = np.tile(ring, 10)
    fs, _, recs, wide, narrow, n0 = _oracle_run("g6b", 1, 300, rf=stream)
    cols = tr.columns(recs)
    wraps = [k for k in range(len(recs)) if cols["start"][k] % cap + cols["n"][k] > cap]
    assert len(wraps) >= 2
    expected, _ = tr.replay(cols, ring, fs, orc.gold_code(7), tr.spacings(cols, 1, wide, narrow))
    assert np.array_equal(expected, cols["corr"])
    assert tr.check_nco(cols, fs, 1, n0=n0) == []
    assert {c for c in tr.classify(cols, "W512", "ci8", 3, cap, epochs=wraps)} == {"PS"}


def test_replay_sees_one_sample_of_one_tap():
    """The bar is a rounding-error scale: one sample left out of one tap's sum (the size of a one-sample chip error) is
    orders of magnitude above it."""
    fs, rf, recs, wide, narrow, _ = _oracle_run("g6c", 1, 3)
    cols = tr.columns(recs)
    expected, scale = tr.replay(cols, rf, fs, orc.gold_code(7), tr.spacings(cols, 1, wide, narrow))
    got = cols["corr"].copy()
    k, s0, n = 1, int(cols["start"][1]), int(cols["n"][1])
    x = rf[s0 + n - 1]
    ph = -(cols["carrier_hz_in"][k] * 2.0 * np.pi * (n - 1) / fs) + cols["rem_carrier_in"][k]
    chip = orc.pad_code(orc.gold_code(7))[orc.epl_indices(n, cols["rem_code_in"][k], cols["code_step_in"][k], wide[0])[-1]]
    mixed = chip * np.exp(1j * ph) * x
    got[k, 0] -= mixed.real
    got[k, 1] -= mixed.imag
    r = tr.tap_ratios(got, expected, scale)
    assert r[k, 0] > 1e3 * tr.BAR and np.all(np.delete(r.reshape(-1), 3 * k) == 0.0)


def test_nco_check_finds_a_broken_hand_over():
    fs, rf, recs, wide, narrow, n0 = _oracle_run("g6", 1, 20)
    cols = tr.columns(recs)
    for field, k, delta in (("start", 5, 1), ("n", 7, 1), ("rem_code_in", 9, 1e-9), ("rem_carrier_in", 11, 1e-9),
                            ("code_step_in", 13, 1e-12), ("carrier_hz_in", 15, 1e-7)):
        bad = {key: v.copy() for key, v in cols.items()}
        bad[field][k] = bad[field][k] + delta
        assert any(f[0] == field and f[1] == k for f in tr.check_nco(bad, fs, 1, n0=n0)), field
    assert tr.check_nco(cols, fs, 1, n0=n0 + 1)[0][:2] == ("n", 0)


# ------------------------------------------------------------------------------------------------ the core classifier
def _step(fs):
    return orc.CODE_RATE / fs


def _n(fs):
    return orc.required_samples(0.0, _step(fs))


CAP = 10_000_000


def test_thresholds_come_from_the_kernel_headers():
    t = tr.THRESHOLDS
    assert 0 < t["kFastMinCodeStep"] < t["kChipMinCodeStep"] < t["kFastMaxCodeStep"] < t["kChipMaxCodeStep"] < t["kFastMaxCodeStep8"]
    # the rates the GPU matrix puts on the thresholds: nominal code steps that are the thresholds themselves
    assert _step(8.184e6) == t["kFastMaxCodeStep8"] and _step(17.05e6) == t["kFastMaxCodeStep"]
    assert _step(26.4957e6) == t["kChipMinCodeStep"] and _n(32.768e6) == 16 * 2048


@pytest.mark.parametrize("fs,want", [
    (25e6, {"W512": "B16", "C2": "B16", "C4": "B16", "C8": "SG", "D": "CH"}),
    (20e6, {"W512": "B16", "C2": "B16", "C4": "B16", "C8": "SG", "D": "B16"}),
    (24.6e6, {"W512": "B16", "C2": "B16", "C4": "B16", "C8": "SG", "D": "CH"}),
    # (the chip-aligned core is tried from 15.5 to 25.9 samples per chip but runs blocks of CHIP_BLOCK (24) / + 1 only)
    (16.368e6, {"W512": "B8", "C2": "B8", "C4": "B8", "C8": "B8", "D": "B8"}),
    (10e6, {"W512": "B8", "C2": "B8", "C4": "B8", "C8": "B8", "D": "B8"}),
    (4e6, {"W512": "PS", "C2": "PS", "C4": "PS", "C8": "PS", "D": "PS"}),
    (50e6, {"W512": "B16", "C2": "B16", "C4": "B16", "C8": "B16", "D": "B16"}),
])
def test_classifier_known_answers(fs, want):
    for form, core in want.items():
        assert tr.expected_core(form, "ci8", 3, _step(fs), _n(fs), 4096, CAP) == core, form
    # CH is the dense form's ci8 3-tap core only
    if want["D"] == "CH":
        for fmt in ("ci16", "cf32", "cf64"):
            assert tr.expected_core("D", fmt, 3, _step(fs), _n(fs), 4096, CAP) == want["W512"]
        assert tr.expected_core("D", "ci8", 5, _step(fs), _n(fs), 4096, CAP) == want["W512"]


@pytest.mark.parametrize("form", list(tr.FORM_PARTS))
def test_classifier_wrapping_epochs_take_the_per_sample_core(form):
    fs = 25e6
    n = _n(fs)
    cap = 40 * n + 8
    for start in (cap - n + 100, 3 * cap - 5, 2 * cap - n + 1):
        assert tr.expected_core(form, "ci8", 3, _step(fs), n, start, cap) == "PS"


def _up(x):
    return math.nextafter(x, 1.0)


def _down(x):
    return math.nextafter(x, 0.0)


def test_classifier_on_both_sides_of_each_threshold():
    t = tr.THRESHOLDS
    s8, s16, cmin, cmax, smin = (t[k] for k in ("kFastMaxCodeStep8", "kFastMaxCodeStep", "kChipMinCodeStep", "kChipMaxCodeStep",
                                                 "kFastMinCodeStep"))
    n = 20000
    core = lambda form, s, n=n, fmt="ci8", taps=3, pos=4096: tr.expected_core(form, fmt, taps, s, n, pos, CAP)
    # 8.184 MHz: s = 0.125
    for form in ("W512", "C8", "D"):
        assert core(form, s8) == "B8" and core(form, _up(s8)) == "PS"
    # 17.05 MHz: s = 0.06
    assert core("W512", s16) == "B16" and core("W512", _up(s16)) == "B8"
    assert core("C8", s16) == "SG" and core("C8", _up(s16)) == "B8"
    # 26.4957 MHz in the dense form: s = 1/25.9 is where the chip-aligned core is tried, but 25-sample blocks are not the
    # closed loop's (compiled-in 24): B16 on both sides
    assert tr.CHIP_BLOCK == 24
    assert core("D", cmin) == "B16" and core("D", _down(cmin)) == "B16"
    assert core("D", cmax) == "B8" and core("D", _up(cmax)) == "B8"
    # 25.575 / 24.552 MHz in the dense form: s = 1/25 and 1/24 exactly, where the block length M leaves 24 (a code-rate
    # change of 0.1 ppm: a DLL's)
    s25, s24 = _step(25.575e6), _step(24.552e6)
    assert s25 == 1.0 / 25.0 and core("D", s25) == "B16" and core("D", s25 * (1 + 1e-7)) == "CH"
    assert s24 == 1.0 / 24.0 and core("D", s24) == "CH" and core("D", s24 * (1 + 1e-7)) == "B16"
    # 32.768 MHz in C8: n = 16 * 2048 is the longest epoch the single-round core takes
    s = _step(32.768e6)
    assert core("C8", s, n=32768) == "SG" and core("C8", s, n=32769) == "B16"
    assert core("C4", s, n=16384) == "SG" and core("C4", s, n=16385) == "B16"
    # the lower end of the boundary variants
    assert core("W512", smin) == "B16" and core("W512", _down(smin)) == "PS" and core("C8", _down(smin)) == "PS"
    assert tr.expected_core("W512", "ci8", 3, s16, n, 4096, CAP, prefix=False) == "PS"


def test_classifier_at_the_ring_guards():
    """epoch_wraps (a 16-sample group of slack behind the epoch, start rounded down to a multiple of 8), the chip-aligned
    core's 32 samples, the single-round core's whole 16-sample groups."""
    cap = 16 * 9999 + 8                       # a multiple of 8, not of 16
    fs = 25e6
    s, n = _step(fs), _n(fs)                   # 25000 samples: 1563 groups of 16, 25008 samples
    for r in range(8):
        assert (cap - n - 16 - r) % 8 != (cap - n - 16) % 8 or r == 0
    for d, w512, c8, dense in ((-17, "PS", "PS", "PS"), (-1, "PS", "PS", "PS"), (0, "PS", "PS", "PS"), (1, "PS", "PS", "PS"),
                               (8, "PS", "SG", "PS"), (15, "PS", "SG", "PS"), (16, "B16", "SG", "B16"),
                               (31, "B16", "SG", "B16"), (32, "B16", "SG", "CH"), (48, "B16", "SG", "CH")):
        pos = cap - n - d
        assert tr.expected_core("W512", "ci8", 3, s, n, pos, cap) == w512, d
        assert tr.expected_core("C8", "ci8", 3, s, n, pos, cap) == c8, d
        assert tr.expected_core("D", "ci8", 3, s, n, pos, cap) == dense, d
        assert tr.expected_core("D", "ci8", 3, s, n, pos + 5 * cap, cap) == dense, d     # absolute sample index
        assert tr.expected_core("D", "ci16", 3, s, n, pos, cap) == w512, d
    # with the ring a multiple of 8, rounding the start down to a multiple of 8 changes nothing: the guard is the same
    # for every start mod 8
    for r in range(8):
        pos = cap - n - 16 - r
        assert not tr.epoch_wraps(pos, n, cap) and tr.epoch_wraps(pos + r + 1, n, cap)
