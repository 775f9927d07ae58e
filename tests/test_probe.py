"""The NumPy statement of sdr_iq_probe (sydr_amd/signal/probe.py) on its own: its spectrum against scipy.signal.welch, its
integer fields against plain Python integers, the C struct against its ctypes image, and what ProbeResult reads off the raw
fields on hand-made inputs.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import probe_cases as cases
from conftest import REPO
from sydr_amd import _lib
from sydr_amd.signal import probe as pb


def test_spectrum_equals_scipy_welch():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(11)
    fs = 4e6
    worst = 0.0
    for nfft, n in ((64, 64), (64, 1000), (256, 256 * 3 + 77), (1024, 5000), (4096, 4096 * 3 + 2047)):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n) + 30.0 * np.exp(2j * np.pi * 0.17 * np.arange(n)) + (0.5 - 0.25j)
        raw = np.empty(2 * n)
        raw[0::2], raw[1::2] = x.real, x.imag
        got = pb.probe(raw, nfft=nfft, fs=fs)
        _, ref = signal.welch(x, fs, "hann", nfft, nfft // 2, detrend=False, return_onesided=False, scaling="density")
        err = float(np.max(np.abs(got.psd - ref)) / ref.max())
        worst = max(worst, err)
        assert got.n_segments == (n - nfft) // (nfft // 2) + 1
        assert err <= 1e-12, (nfft, n, err)
    print(f"statement against scipy.signal.welch: worst {worst:.3g} of the peak")


@pytest.mark.parametrize("fmt", [0, 1])
def test_integer_fields_equal_plain_python_integers(fmt):
    rng = np.random.default_rng(20 + fmt)
    raw = cases.integer_ring(rng, fmt, 4096)
    info = np.iinfo(raw.dtype)
    for start, n in ((0, 4096), (5, 1), (17, 1001), (4000, 300)):
        win = cases.window(raw, start, n)
        vi, vq = [int(v) for v in win[0::2]], [int(v) for v in win[1::2]]
        for shift in cases.HIST_SHIFTS[fmt]:
            got = pb.probe(win, hist_shift=shift)
            assert got.n_samples == n and got.n_segments == 0 and got.n_nonfinite == 0
            assert got.sum == (float(sum(vi)), float(sum(vq)))
            assert got.sum_sq == (float(sum(v * v for v in vi)), float(sum(v * v for v in vq)))
            assert got.sum_iq == float(sum(a * b for a, b in zip(vi, vq)))
            assert got.min == (float(min(vi)), float(min(vq))) and got.max == (float(max(vi)), float(max(vq)))
            assert got.n_rail == tuple(sum(v in (info.min, info.max) for v in c) for c in (vi, vq))
            for c, vals in enumerate((vi, vq)):
                want = [0] * 256
                for v in vals:
                    want[min(255, max(0, (v >> shift) + 128))] += 1
                assert got.hist[c].tolist() == want
                assert int(got.hist[c].sum()) == n
    # sums beyond 2^53 round once, to nearest even: what float(int) does
    big = np.full(2 * (1 << 20), info.min, dtype=raw.dtype)
    assert pb.probe(big).sum_sq[0] == float((1 << 20) * info.min * info.min)
    with pytest.raises(ValueError):
        pb.probe(raw, hist_shift=9 if fmt else 1)


def test_float_samples_with_nan_and_inf_are_counted_and_left_out():
    raw = np.array([1.0, 2.0, np.nan, 5.0, 3.0, -4.0, 7.0, np.inf, -1.0, 0.5], dtype=np.float32)
    got = pb.probe(raw)
    assert got.n_samples == 5 and got.n_nonfinite == 2 and got.n_rail == (0, 0) and got.hist is None
    assert got.sum == (3.0, -1.5) and got.sum_sq == (11.0, 20.25) and got.sum_iq == 2.0 - 12.0 - 0.5
    assert got.min == (-1.0, -4.0) and got.max == (3.0, 2.0)
    none = pb.probe(np.array([np.nan, 1.0, 2.0, -np.inf]))
    assert none.n_nonfinite == 2 and all(np.isnan(v) for v in none.min + none.max) and none.sum == (0.0, 0.0)
    # a non-finite sample in a used segment: the spectrum is NaN; only in the unused tail: it is not
    x = np.ones(2 * (64 + 32 + 5))
    x[2 * 70] = np.nan
    assert np.isnan(pb.probe(x, nfft=64, fs=1.0).psd).all()
    x = np.ones(2 * (64 + 32 + 5))
    x[2 * 97 + 1] = np.inf
    tail = pb.probe(x, nfft=64, fs=1.0)
    assert np.isfinite(tail.psd).all() and tail.n_segments == 2 and tail.n_nonfinite == 1


def test_c_struct_layout_equals_the_ctypes_image(tmp_path):
    fields = [name for name, _ in _lib.ProbeResultC._fields_]
    src = tmp_path / "probe_sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu", sizeof(sdr_probe_result));\n'
                   + "".join(f'printf(" %zu", offsetof(sdr_probe_result, {f}));\n' for f in fields) + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "probe_sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.ProbeResultC)] + [getattr(_lib.ProbeResultC, f).offset for f in fields]
    assert C.sizeof(_lib.ProbeResultC) == 5 * 8 + 9 * 8
    assert "sdr_iq_probe" in _lib.exported_symbols() and hasattr(_lib.load(), "sdr_iq_probe")


def test_what_a_result_says_about_a_front_end():
    rng = np.random.default_rng(5)
    n, fs = 1 << 16, 4e6
    # a known DC offset on I: mean 3, noise sigma 4 -> mean / rms = 3 / 5
    i, q = 3.0 + 4.0 * rng.standard_normal(n), 4.0 * rng.standard_normal(n)
    raw = np.empty(2 * n)
    raw[0::2], raw[1::2] = i, q
    r = pb.probe(raw)
    assert abs(r.mean[0] - 3.0) < 0.1 and abs(r.mean[1]) < 0.1
    assert abs(r.dc_offset[0] - 0.6) < 0.02 and abs(r.dc_offset[1]) < 0.02
    assert abs(r.iq_correlation) < 0.02
    # a 2:1 I/Q gain: 20 log10(2) dB
    raw[0::2], raw[1::2] = 2.0 * q, q[::-1].copy()
    r = pb.probe(raw)
    assert abs(r.iq_imbalance_db - 20.0 * np.log10(2.0)) < 1e-9
    assert abs(r.rms[0] / r.rms[1] - 2.0) < 1e-12
    # Q a copy of I: correlation 1
    raw[0::2], raw[1::2] = q, q
    assert abs(pb.probe(raw).iq_correlation - 1.0) < 1e-12
    # rails of an int8 stream: a quarter of the I components
    few = np.zeros(2 * 1000, dtype=np.int8)
    few[0:500:2] = 127
    few[1::2] = 3
    r = pb.probe(few)
    assert r.rail_fraction == (0.25, 0.0) and r.n_rail == (250, 0)
    assert r.hist[0][255] == 250 and r.hist[0][128] == 750 and r.hist[1][131] == 1000
    # a tone in noise: `spurs` finds it at its frequency, and nothing else
    f_tone = -37 * fs / 1024
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n) + 10.0 * np.exp(2j * np.pi * f_tone / fs * np.arange(n))
    raw[0::2], raw[1::2] = x.real, x.imag
    r = pb.probe(raw, nfft=1024, fs=fs)
    spurs = r.spurs(15.0)
    assert spurs and spurs[0][0] == f_tone and spurs[0][1] > 30.0
    assert all(abs(f - f_tone) <= 2 * fs / 1024 for f, _ in spurs)      # (the Hann window's main lobe)
    assert r.frequencies()[1024 - 37] == f_tone and r.psd_db.shape == (1024,)
    with pytest.raises(ValueError):
        pb.probe(raw).spurs(10.0)
