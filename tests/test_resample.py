"""Rational-rate resampling in the down-converter (interpolation by L, decimation by M), everything that needs no GPU: the
NumPy statement (sydr_amd/signal/downconvert.py with `interpolation`) against an independent zero-stuff / convolve / decimate
formulation, against itself however the stream is cut, and at L = 1 against a frozen copy of the arithmetic it replaced;
`design_resampler`; the [RFSIGNAL] key; the manager's slab check; the new export's prototype; the shared index arithmetic
(sydr_amd/csrc/resample_tiles.h) run on the host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
import downconvert_cases as dcases
import host_check
import resample_cases as cases

from sydr_amd import _lib
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal.iqsource import RFSignal



# ---------------------------------------------------------------------------------------------- 1. the statement
@pytest.mark.parametrize("fcw_name", ["zero", "odd"])
@pytest.mark.parametrize("in_fmt", dcases.IN_FORMATS, ids=lambda f: dcases.IN_NAMES[f])
@pytest.mark.parametrize("shape", cases.CPU_SHAPES, ids=cases.shape_id)
def test_statement_equals_zero_stuffing_filtering_and_decimating(shape, in_fmt, fcw_name):
    L, M, T = shape
    n = 1201 if L > 8 else 3001
    raw = dcases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, L, M, T, dcases.FCWS[fcw_name], dcases.GOLD)
    v = dc.statement(cfg, [raw])
    want = cases.zero_stuffed(cfg, raw)
    assert v.size == want.size == dc.out_count(0, n, M, L) == -(-n * L // M)
    band = dc.tolerance(cfg, dcases.max_abs(in_fmt, raw))
    err = max(np.max(np.abs(v.real - want.real)), np.max(np.abs(v.imag - want.imag)))
    print(f"max |statement - convolve| = {err:.3e}, tolerance {band:.3e}")
    assert 0.0 < band and err <= band
    assert np.max(np.abs(v)) > 10.0                                          # (it is a signal that was compared)
    if T < L:
        # phases p >= T have no tap: exactly gain * 0.0, in both components, at exactly the outputs the formula names
        empty = (np.arange(v.size) * M) % L >= T
        assert empty.any() and np.all(v[empty] == 0.0) and np.count_nonzero(v[~empty]) > 0.9 * np.count_nonzero(~empty)
        assert not np.signbit(v.real[empty]).any() and not np.signbit(v.imag[empty]).any()


@pytest.mark.parametrize("in_fmt", [dc.IN_R8, dc.IN_CI16], ids=lambda f: dcases.IN_NAMES[f])
@pytest.mark.parametrize("shape", cases.CPU_SHAPES + [(6, 4, 25)], ids=cases.shape_id)
def test_statement_is_bit_identical_however_the_stream_is_cut(shape, in_fmt):
    L, M, T = shape
    n = 12001
    raw = dcases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, L, M, T, dcases.FCWS["odd"], dcases.GOLD)
    whole = cases.reference(in_fmt, L, M, T, cfg.fcw, cfg.gain, n)
    assert whole.size == dc.out_count(0, n, M, L)
    Tp = cfg.phase_taps
    assert Tp == -(-T // L)
    st = dc.Statement(cfg)
    parts, counts = [], 0
    for piece in dcases.cut(raw, in_fmt, cases.push_lengths(Tp)):
        n_in = piece.size // (2 if dc.input_is_complex(in_fmt) else 1)
        want = st.out_count(n_in)
        assert want == dc.out_count(st.n_seen, n_in, M, L)
        parts.append(st.push(piece))
        assert parts[-1].size == want
        counts += want
    assert counts == whole.size                                             # the counts of any cut add up to one push's
    assert st._hist_re.size == Tp - 1                                       # the history: the last ceil(T / L) - 1 raw inputs
    assert np.concatenate(parts).tobytes() == whole.tobytes()               # bit for bit, signs of zeros included
    for lengths in ([5000], [1] * 40, [7, 0, 0, 11, 4999]):
        assert dc.statement(cfg, dcases.cut(raw, in_fmt, lengths)).tobytes() == whole.tobytes()
        at, total = 0, 0
        for k in lengths + [n - sum(lengths)]:
            total += dc.out_count(at, k, M, L)
            at += k
        assert total == whole.size
    st.reset()
    assert st.push(raw).tobytes() == whole.tobytes()


@pytest.mark.parametrize("in_fmt", dcases.IN_FORMATS, ids=lambda f: dcases.IN_NAMES[f])
@pytest.mark.parametrize("T,D", [(1, 1), (2, 1), (33, 2), (17, 3), (512, 16), (3, 64)])
def test_interpolation_one_is_the_converter_as_it_was(in_fmt, T, D):
    n = 9001
    raw = dcases.stream(in_fmt, n)
    taps = dcases.taps_for(T, D)
    cfg = dc.DownConverterConfig(in_fmt, D, taps, dcases.FCWS["odd"], dcases.GOLD, 1)
    assert cfg.phase_taps == T and cfg.group_delay == (T - 1) / 2.0
    frozen = cases.Frozen(in_fmt, D, taps, cfg.fcw, cfg.gain)
    st = dc.Statement(cfg)
    for piece in dcases.cut(raw, in_fmt, dcases.push_lengths(T)):
        n_in = piece.size // (2 if dc.input_is_complex(in_fmt) else 1)
        assert st.out_count(n_in) == dc.out_count(st.n_seen, n_in, D) == dc.out_count(st.n_seen, n_in, D, 1)
        assert st.push(piece).tobytes() == frozen.push(piece).tobytes()
        assert st.n_seen == frozen.n_seen and np.array_equal(st._hist_re, frozen._hist_re) and np.array_equal(st._hist_im, frozen._hist_im)
    # the tolerance at L = 1: the expression as it was
    assert dc.tolerance(cfg, 127.0) == abs(cfg.gain) * (T + 16) * 2.0 ** -53 * float(np.sum(np.abs(cfg.taps))) * 127.0


def test_limits_group_delay_and_tolerance():
    ok = dc.DownConverterConfig
    assert ok(dc.IN_CI8, 1024, np.ones(2048), 0, 1.0, 1024).phase_taps == 2
    assert ok(dc.IN_CI8, 1024, np.ones(512), 0, 1.0, 16).phase_taps == 32          # M = 64 L
    assert ok(dc.IN_CI8, 1, np.ones(32768), 0, 1.0, 64).phase_taps == 512
    for bad in (lambda: ok(dc.IN_CI8, 1, [1.0], 0, 1.0, 0), lambda: ok(dc.IN_CI8, 1, [1.0], 0, 1.0, 1025),
                lambda: ok(dc.IN_CI8, 1025, [1.0], 0, 1.0, 1024), lambda: ok(dc.IN_CI8, 129, [1.0], 0, 1.0, 2),      # M > 64 L
                lambda: ok(dc.IN_CI8, 1, np.ones(32769), 0, 1.0, 1024), lambda: ok(dc.IN_CI8, 1, np.ones(32768), 0, 1.0, 63),   # Tp = 521
                lambda: ok(dc.IN_CI8, 65, [1.0]), lambda: ok(dc.IN_CI8, 1, np.ones(513)),                           # L = 1: today's domain
                lambda: dc.design_resampler(0, 1), lambda: dc.design_resampler(1, 65), lambda: dc.design_resampler(3, 2, 3 * 512 + 1),
                lambda: dc.design_resampler(3, 2, 0), lambda: dc.design_resampler(3, 2, 7, 0.0), lambda: dc.design_resampler(3, 2, 7, 0.6)):
        with pytest.raises(ValueError):
            bad()
    cfg = cases.config(dc.IN_CI8, 250, 341, 5457, 0, 2.0)
    assert cfg.group_delay == 5456 / 500.0 and cfg.phase_taps == 22 and cfg.interpolation == 250 and cfg.decimation == 341
    h_max = max(float(np.sum(np.abs(cfg.taps[p::250]))) for p in range(250))
    assert dc.tolerance(cfg, 180.0) == 2.0 * (22 + 16) * 2.0 ** -53 * h_max * 180.0
    assert dc.out_count(5, 7, 341, 250) == -(-12 * 250 // 341) - -(-5 * 250 // 341)


def test_design_resampler():
    for L, M in ((250, 341), (500, 341), (625, 341), (2, 3), (3, 2), (5, 4), (64, 1)):
        h = dc.design_resampler(L, M)
        big = max(L, M)
        assert h.size == 16 * big + 1 and abs(h.sum() - L) < 1e-12 * L and np.allclose(h, h[::-1], rtol=0, atol=1e-15 * L)
        # every phase has about unit DC gain: the sinc's side lobes alias into a phase's sum below the stop band's level --
        # within 2 % with these defaults (cutoff 0.45 / max(L, M), beta 8)
        sums = np.array([h[p::L].sum() for p in range(L)])
        assert np.all(np.abs(sums - 1.0) < 0.02), (L, M, sums.min(), sums.max())
        # pass band flat, stop band down 60 dB, at the up-sampled rate (as test_tones asks of the low-pass)
        nfft = 1 << int(np.ceil(np.log2(64 * h.size)))
        H = np.abs(np.fft.rfft(h, nfft)) / L
        f = np.arange(H.size) / nfft
        assert H[f <= 0.30 / big].min() > 0.99 and H[f >= 0.70 / big].max() < 1e-3, (L, M)
    assert dc.design_resampler(4, 1, 1).tolist() == [4.0]
    assert dc.design_resampler(3, 2, 7).size == 7 and np.array_equal(dc.design_resampler(3, 2, 49, 0.1), dc.design_resampler(3, 2, 49, 0.1, 8.0))


def test_tones_through_the_resampler():
    """A complex tone at the shift frequency comes out as DC of about gain (every phase's sum is about 1); a tone in the stop band
    of the prototype -- which would alias onto DC at the output rate -- is attenuated by what the taps' own response says."""
    L, M, n, gain, A = 3, 2, 16368, 1.5, 20000.0
    h = dc.design_resampler(L, M)
    k = np.arange(n)
    tone = A * np.exp(2j * np.pi * k / 8)
    raw = np.empty(2 * n, dtype=np.int16)
    raw[0::2], raw[1::2] = np.rint(tone.real), np.rint(tone.imag)
    cfg = dc.DownConverterConfig(dc.IN_CI16, M, h, dc.frequency_word(1.0, 8.0), gain, L)
    v = dc.statement(cfg, [raw])[60:]
    sums = np.array([h[p::L].sum() for p in range(L)])
    assert np.max(np.abs(v - gain * A)) < gain * A * np.max(np.abs(sums - 1.0)) + 2.0 * gain * np.max(sums)
    # a tone at nu = 0.4 of the input rate, no shift: at the up-sampled rate 0.4 / 3 and its images (0.4 + i) / 3 lie in the stop
    # band (cutoff 0.45 / 3 = 0.15, stop from 0.7 / 3); the output holds the tone itself times H(0.4 / 3) plus images below 1e-3
    nu = 0.4
    tone = A * np.exp(2j * np.pi * nu * k)
    raw[0::2], raw[1::2] = np.rint(tone.real), np.rint(tone.imag)
    v = dc.statement(dc.DownConverterConfig(dc.IN_CI16, M, h, 0, gain, L), [raw])[60:]
    H = lambda f: np.sum(h * np.exp(-2j * np.pi * f * np.arange(h.size))) / L
    images = sum(abs(H((nu + i) / L)) for i in range(1, L))
    assert images < 2e-3 and 0.5 < abs(H(nu / L)) < 0.9                       # (0.4 / 3 = 0.133: in the transition band)
    m = 60 + np.arange(v.size)
    want = gain * A * H(nu / L) * np.exp(2j * np.pi * (nu / L) * (m * M))
    assert np.max(np.abs(v - want)) < gain * A * images + 2.0 * gain * np.max(sums)


# ---------------------------------------------------------------------------------------------- 2. RFSignal
def test_rfsignal_interpolation_key(tmp_path):
    path = tmp_path / "rec.bin"
    raw = dcases.stream(dc.IN_CI8, 3 * 16368)
    raw.tofile(path)
    sig = RFSignal(cases.recording_conf(path))
    fe = sig.frontEnd
    assert sig.samplingFrequency == 12e6 and sig.samplesPerMs == 12000 and sig.interFrequency == 0.0
    assert (sig.inputSamplingFrequency, sig.inputSamplesPerMs) == (16.368e6, 16368)
    assert fe.interpolation == 250 and fe.decimation == 341 and fe.outputBits == 8
    cfg = fe.config
    assert cfg.interpolation == 250 and cfg.decimation == 341 and cfg.in_fmt == dc.IN_CI8 and cfg.gain == 2.0 and cfg.fcw == 0
    assert np.array_equal(cfg.taps, dc.design_resampler(250, 341)) and cfg.n_taps == 16 * 341 + 1
    assert fe.groupDelay == cfg.group_delay == 5456 / 500.0                              # input samples: 8 output samples
    assert sig.totalSamples == 3 * 16368 and np.array_equal(sig.getMilliseconds(1), raw[:2 * 16368])
    # the optional keys: taps and a cutoff as a fraction of the UP-SAMPLED rate; the other documented rates
    own = RFSignal(cases.recording_conf(path, filter_taps=1500, filter_cutoff=0.001, baseband_shift=1e3, intermediate_frequency=4e3))
    assert np.array_equal(own.frontEnd.config.taps, dc.design_resampler(250, 341, 1500, 0.001)) and own.interFrequency == 3e3
    assert own.frontEnd.config.fcw == dc.frequency_word(1e3, 16.368e6)
    assert RFSignal(cases.recording_conf(path, interpolation=500)).samplingFrequency == 24e6
    ci16 = RFSignal(cases.recording_conf(path, sampling_frequency=5.456e6, interpolation=625, data_size=16))
    assert ci16.samplingFrequency == 10e6 and ci16.samplesPerMs == 10000 and ci16.frontEnd.config.in_fmt == dc.IN_CI16
    real = RFSignal(dict(filepath="x", sampling_frequency=6.138e6, is_complex="", intermediate_frequency=1.5345e6, data_size=8,
                         decimation=3, interpolation=2))
    assert real.samplingFrequency == 4.092e6 and real.samplesPerMs == 4092 and real.frontEnd.config.in_fmt == dc.IN_R8 and real.frontEnd.config.fcw == 1 << 62
    assert real.frontEnd.config.n_taps == 49 and real.interFrequency == 0.0


def test_rfsignal_interpolation_refusals_and_untouched_defaults():
    conf = cases.recording_conf("x")
    no_decimation = {k: v for k, v in conf.items() if k != "decimation"}
    for bad in (no_decimation,                                                            # only valid beside `decimation`
                dict(conf, decimation=340),                                               # 16368 * 250 / 340: no whole millisecond
                dict(conf, interpolation=7),                                              # 16368 * 7 / 341: neither
                dict(conf, interpolation=0), dict(conf, interpolation=1025), dict(conf, interpolation=-3),
                dict(conf, interpolation=2, decimation=129),                              # M > 64 L
                dict(conf, interpolation=1024, decimation=1025),
                dict(conf, filter_taps=250 * 512 + 1), dict(conf, filter_taps=32769, interpolation=1000, decimation=1000),
                dict(conf, filter_cutoff=0.6), dict(conf, data_size=2), dict(conf, data_size=4)):    # packed input
        with pytest.raises(ValueError):
            RFSignal(bad)
    with pytest.raises(ValueError, match="`interpolation` needs `decimation`"):
        RFSignal(no_decimation)
    # without the key every attribute is what it was: the converter tests' own front end, defaults included
    base = dcases.real_signal_conf("x")
    plain, one = RFSignal(base), RFSignal(dict(base, interpolation=1))
    for sig in (plain, one):
        fe = sig.frontEnd
        assert (sig.samplingFrequency, sig.samplesPerMs, sig.interFrequency, sig.inputSamplesPerMs) == (4.092e6, 4092, 0.0, 8184)
        assert fe.decimation == 2 and fe.interpolation == 1 and fe.groupDelay == 16.0 and fe.config.interpolation == 1
        assert np.array_equal(fe.config.taps, dc.design_lowpass(33, 0.225)) and fe.config.fcw == 1 << 62 and fe.config.gain == 2.0
    with pytest.raises(ValueError, match="not a whole multiple of decimation 5"):
        RFSignal(dict(base, decimation=5))
    with pytest.raises(ValueError, match="decimation 65 outside 1..64"):
        RFSignal(dict(base, decimation=65))


# ---------------------------------------------------------------------------------------------- 3. the manager
def test_manager_advances_the_ring_by_the_resampled_count(tmp_path):
    from fake_engine import OracleEngine
    from sydr_amd.channel.manager import ChannelManager

    class Engine(OracleEngine):
        def ddc_create(self, cfg):
            return dc.Statement(cfg)

        def ddc_push(self, ddc, raw, ring_offset=0):
            v = ddc.push(raw)
            self.iq_upload(dc.quantise(v, self.iq_fmt), ring_offset)
            return v.size

        def ddc_destroy(self, ddc):
            pass

    sig, _, converted = cases.write_recording_and_converted(tmp_path, 3)
    eng = Engine()
    mgr = ChannelManager(sig, engine=eng)
    assert mgr.sharedBuffer.maxSize == 100 * 12000 and mgr.sharedBuffer.fmt == 0          # a ci8 ring at the OUTPUT rate
    with pytest.raises(ValueError, match="times interpolation 250 is not a whole multiple of decimation 341"):
        mgr.addNewRFData(sig.samples(0, 16367))
    mgr.addNewRFData(sig.getMilliseconds(1))
    assert mgr.sharedBuffer.idxWrite == 12000                                              # n_in * L / M
    mgr.addNewRFData(sig.getMilliseconds(1))
    assert mgr.sharedBuffer.idxWrite == 24000
    assert np.array_equal(eng.ring[:2 * 24000], converted[:2 * 24000])
    mgr.close()


# ---------------------------------------------------------------------------------------------- 4. the export's prototype
def test_create_rational_prototype_agrees_with_the_header(tmp_path):
    """The ctypes prototype against include/sydr_amd.h: the C compiler accepts the header's declaration as exactly
    int (sdr_engine*, const sdr_ddc_cfg*, int, sdr_ddc**) -- a mismatch is an error --, and the binding says the same."""
    src = tmp_path / "proto.c"
    src.write_text('#include "sydr_amd.h"\n'
                   "int (*const rational)(sdr_engine*, const sdr_ddc_cfg*, int, sdr_ddc**) = sdr_ddc_create_rational;\n"
                   "int (*const integer)(sdr_engine*, const sdr_ddc_cfg*, sdr_ddc**) = sdr_ddc_create;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(REPO, "include"), "-c", str(src),
                           "-o", str(tmp_path / "proto.o")])
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sydr_amd.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sdr_ddc_create_rational\(sdr_engine\*\s*e,\s*const sdr_ddc_cfg\*\s*cfg,\s*int interpolation,\s*sdr_ddc\*\*\s*out\);", text)
    lib = _lib.load()
    fn = lib.sdr_ddc_create_rational
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.POINTER(_lib.DdcCfg), C.c_int, C.POINTER(C.c_void_p)]
    assert list(fn.argtypes[:2]) + [fn.argtypes[3]] == list(lib.sdr_ddc_create.argtypes)
    assert "sdr_ddc_create_rational" in _lib.exported_symbols()
    # (host checks come before any device call: NULL arguments are refused without a GPU too)
    assert fn(None, None, 3, None) != 0


# ---------------------------------------------------------------------------------------------- 5. the index arithmetic
@host_check.requires_hipcc
def test_tile_phase_history_and_ring_arithmetic_on_the_host():
    """sydr_amd/csrc/resample_tiles.h, the arithmetic the resampler's kernels and its host side share, compiled for the host
    alone and checked exhaustively over small L, M, T, tile, push length, ring offset and capacity
    (tests/csrc/resample_tiles_check.hip)."""
    exe = host_check.build("resample_tiles_check")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 1000000
