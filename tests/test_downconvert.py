"""The down-converter between a recording and the ring, everything that needs no GPU: the NumPy statement
(sydr_amd/signal/downconvert.py) against itself however the stream is cut, against pass-through and against tones; the
[RFSIGNAL] keys; the manager's converting route over the oracle-backed engine (packets equal to those of the statement's
output stored as an ordinary complex recording); the C struct's layout; the shared index arithmetic run on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from oracle import sydr_oracle as orc
from fake_engine import OracleEngine
import downconvert_cases as cases
import host_check
import packed_cases

from sydr_amd import _lib
from sydr_amd.channel.manager import ChannelManager
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal.iqsource import RFSignal
from sydr_amd.utils.enumerations import ChannelMessage



# ---------------------------------------------------------------------------------------------- 1. the statement
@pytest.mark.parametrize("in_fmt", cases.IN_FORMATS, ids=lambda f: cases.IN_NAMES[f])
@pytest.mark.parametrize("T,D", [(1, 1), (2, 1), (33, 2), (17, 3), (512, 16), (3, 64)])
def test_statement_is_bit_identical_however_the_stream_is_cut(in_fmt, T, D):
    n = 12001
    raw = cases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, T, D, cases.FCWS["odd"], cases.GOLD)
    whole = cases.reference(in_fmt, T, D, cfg.fcw, cfg.gain, n)
    assert whole.size == dc.out_count(0, n, D) == -(-n // D)
    lengths = [1, 2, 3, max(T - 2, 0), max(T - 1, 0), T, T + 1, 1000]
    st = dc.Statement(cfg)
    parts = []
    for piece in cases.cut(raw, in_fmt, lengths):
        want = st.out_count(piece.size // (2 if dc.input_is_complex(in_fmt) else 1))
        parts.append(st.push(piece))
        assert parts[-1].size == want
    cutup = np.concatenate(parts)
    assert cutup.tobytes() == whole.tobytes()                  # bit for bit, signs of zeros included
    assert dc.statement(cfg, cases.cut(raw, in_fmt, [5000])).tobytes() == whole.tobytes()
    # `state` carries history and index between calls; reset starts over
    st = dc.Statement(cfg)
    a = dc.statement(cfg, cases.cut(raw, in_fmt, [777])[:1], state=st)
    b = dc.statement(cfg, cases.cut(raw, in_fmt, [777])[1:], state=st)
    assert np.concatenate([a, b]).tobytes() == whole.tobytes()
    st.reset()
    assert st.push(raw).tobytes() == whole.tobytes()


@pytest.mark.parametrize("in_fmt", cases.IN_FORMATS, ids=lambda f: cases.IN_NAMES[f])
def test_pass_through_is_the_identity(in_fmt):
    raw = cases.stream(in_fmt, 5001)
    v = dc.statement(dc.DownConverterConfig(in_fmt), [raw])
    x = raw.astype(np.float64)
    want = x[0::2] + 1j * x[1::2] if dc.input_is_complex(in_fmt) else x + 0j
    assert np.array_equal(v, want)
    ring_fmt = dc.FMT_CI8 if raw.dtype == np.int8 else dc.FMT_CI16
    pair = dc.quantise(v, ring_fmt)
    assert pair.dtype == raw.dtype
    if dc.input_is_complex(in_fmt):
        assert np.array_equal(pair, raw)
    else:
        assert np.array_equal(pair[0::2], raw) and not pair[1::2].any()      # a real recording lands as (r, 0)


def test_frequency_word_and_lowpass():
    assert dc.frequency_word(0.0, 1e6) == 0
    assert dc.frequency_word(2.046e6, 8.184e6) == 1 << 62
    assert dc.frequency_word(-2.046e6, 8.184e6) == 3 << 62                   # mod 2^64
    assert dc.frequency_word(8.184e6, 8.184e6) == 0
    assert dc.frequency_word(1.0, 3.0) == ((1 << 64) + 1) // 3                  # exact rational arithmetic, not a float quotient
    assert 0 <= dc.frequency_word(1234567.891, 8.184e6) < 1 << 64
    for T, cutoff in ((33, 0.225), (17, 0.15), (512, 0.45 / 16), (2, 0.3)):
        h = dc.design_lowpass(T, cutoff)
        assert h.size == T and abs(h.sum() - 1.0) < 1e-15 and np.allclose(h, h[::-1], rtol=0, atol=1e-18)
    assert dc.design_lowpass(1, 0.2).tolist() == [1.0]
    H = np.abs(np.fft.fft(dc.design_lowpass(33, 0.225), 4096))
    assert H[: int(0.15 * 4096)].min() > 0.99 and H[int(0.35 * 4096): 2048].max() < 1e-3   # pass band flat, stop band down 60 dB
    for bad in (lambda: dc.design_lowpass(0, 0.2), lambda: dc.design_lowpass(513, 0.2), lambda: dc.design_lowpass(9, 0.0),
                lambda: dc.design_lowpass(9, 0.6), lambda: dc.DownConverterConfig(dc.IN_R8, 0), lambda: dc.DownConverterConfig(dc.IN_R8, 65),
                lambda: dc.DownConverterConfig(dc.IN_R8, 1, [1.0, float("nan")]), lambda: dc.DownConverterConfig(dc.IN_R8, 1, [1.0], 0, float("inf")),
                lambda: dc.DownConverterConfig(7), lambda: dc.DownConverterConfig(dc.IN_R8, 1, np.ones(513)), lambda: dc.frequency_word(1.0, 0.0)):
        with pytest.raises(ValueError):
            bad()


def test_tones():
    """A complex tone at the shift frequency comes out as DC of size gain * sum(h); the image of a real tone (at minus twice
    the shift after mixing) is attenuated by what the taps' own frequency response says there."""
    fs, n, D, gain, A = 8.184e6, 16368, 2, 1.5, 20000.0
    h = dc.design_lowpass(33, 0.225)
    k = np.arange(n)
    # 1. complex tone at fs / 8 (int16 I,Q), shifted by fs / 8
    tone = A * np.exp(2j * np.pi * k / 8)
    raw = np.empty(2 * n, dtype=np.int16)
    raw[0::2], raw[1::2] = np.rint(tone.real), np.rint(tone.imag)
    cfg = dc.DownConverterConfig(dc.IN_CI16, D, h, dc.frequency_word(fs / 8, fs), gain)
    v = dc.statement(cfg, [raw])[40:]                                       # (past the filter's start-up)
    assert np.max(np.abs(v - gain * h.sum() * A)) < 2.0 * gain              # rounding the tone to int16: < 1 LSB per component
    # 2. real tone at 3 fs / 16 (int16), shifted by as much: DC of half the amplitude plus the image at nu = -3 / 8 of the input
    # rate, which the filter passes with its own response H(nu) = sum_k h_k e^{-2 pi i nu k} -- deep in its stop band
    f, nu = 3.0 / 16.0, -3.0 / 8.0
    real = np.rint(A * np.cos(2 * np.pi * f * k)).astype(np.int16)
    cfg = dc.DownConverterConfig(dc.IN_R16, D, h, dc.frequency_word(f * fs, fs), gain)
    v = dc.statement(cfg, [real])[40:]
    H_image = np.sum(h * np.exp(-2j * np.pi * nu * np.arange(h.size)))
    m = 40 + np.arange(v.size)                                               # the outputs' numbers
    image = gain * (A / 2) * H_image * np.exp(2j * np.pi * nu * (m * D))
    assert abs(H_image) < 1e-3
    assert np.max(np.abs(v - gain * h.sum() * A / 2 - image)) < 2.0 * gain
    assert np.max(np.abs(v - gain * h.sum() * A / 2)) < 2.0 * gain + gain * (A / 2) * abs(H_image)
    # ... and where the response is NOT small (the default cutoff's transition band, nu = -1 / 4) the image is there, as large as
    # the taps say: the statement filters, it does not idealise
    f, nu = 1.0 / 8.0, -1.0 / 4.0
    real = np.rint(A * np.cos(2 * np.pi * f * k)).astype(np.int16)
    v = dc.statement(dc.DownConverterConfig(dc.IN_R16, D, h, dc.frequency_word(f * fs, fs), gain), [real])[40:]
    H_image = np.sum(h * np.exp(-2j * np.pi * nu * np.arange(h.size)))
    image = gain * (A / 2) * H_image * np.exp(2j * np.pi * nu * (m * D))
    assert 0.1 < abs(H_image) < 0.3
    assert np.max(np.abs(v - gain * h.sum() * A / 2 - image)) < 2.0 * gain
    # quantised: ties to even, clipped
    q = dc.quantise(np.array([0.5 + 1.5j, 2.5 - 0.5j, 300.0 - 300.0j, 126.5 + 127.5j]), dc.FMT_CI8)
    assert q.tolist() == [0, 2, 2, 0, 127, -127, 126, 127] and q.dtype == np.int8
    assert dc.quantise(np.array([40000.0 - 40000.0j]), dc.FMT_CI16).tolist() == [32767, -32767]
    assert dc.ambiguous(np.array([0.5 + 1j, 2.25 - 3.5000000000001j]), 1e-9) == 2 and dc.ambiguous(np.array([0.4 + 1j]), 1e-9) == 0


# ---------------------------------------------------------------------------------------------- 2. RFSignal
def test_rfsignal_front_end_keys(tmp_path):
    path = tmp_path / "real.bin"
    raw = cases.real_if_recording(3)
    raw.tofile(path)
    sig = RFSignal(cases.real_signal_conf(path))
    fe = sig.frontEnd
    assert not sig.isComplex and sig.packing is None and sig.fileDataType == np.int8
    assert (sig.samplingFrequency, sig.samplesPerMs, sig.interFrequency) == (4.092e6, 4092, 0.0)     # the ring's
    assert (sig.inputSamplingFrequency, sig.inputSamplesPerMs) == (8.184e6, 8184)
    assert fe.decimation == 2 and fe.outputBits == 8 and fe.groupDelay == 16.0 and fe.shift == 2.046e6
    cfg = fe.config
    assert cfg.in_fmt == dc.IN_R8 and cfg.n_taps == 33 and cfg.fcw == 1 << 62 and cfg.gain == 2.0
    assert np.array_equal(cfg.taps, dc.design_lowpass(33, 0.225))
    # raw input is handed out: a millisecond is 8184 int8, a view of the file
    assert sig.totalSamples == raw.size
    ms = sig.getMilliseconds(1)
    assert ms.dtype == np.int8 and np.array_equal(ms, raw[:8184]) and np.shares_memory(ms, sig._recording()) and sig.position == 8184
    assert np.array_equal(sig.samples(100, 50), raw[100:150])
    assert np.array_equal(sig.getMilliseconds(1, raw=False), raw[8184:2 * 8184].astype(np.float64) + 0j)
    assert np.array_equal(sig.readFile(timeLength=1, raw=True), raw[:8184])
    # the optional keys; a complex wide-band recording
    wide = RFSignal(dict(filepath="x", sampling_frequency=50e6, is_complex="true", intermediate_frequency=1e6, data_size=16, decimation=5,
                         baseband_shift=0.25e6, filter_taps=41, filter_cutoff=0.08, output_gain=0.5, output_bits=8))
    assert wide.samplingFrequency == 10e6 and wide.samplesPerMs == 10000 and wide.interFrequency == 0.75e6 and wide.inputSamplesPerMs == 50000
    assert wide.frontEnd.outputBits == 8 and wide.frontEnd.config.in_fmt == dc.IN_CI16 and wide.frontEnd.config.gain == 0.5
    assert np.array_equal(wide.frontEnd.config.taps, dc.design_lowpass(41, 0.08)) and wide.frontEnd.config.fcw == dc.frequency_word(0.25e6, 50e6)
    assert RFSignal(dict(cases.real_signal_conf("x"), filter_taps=1)).frontEnd.config.taps.tolist() == [1.0]   # no filter
    assert RFSignal(dict(cases.real_signal_conf("x"), data_size=16)).frontEnd.outputBits == 16                 # default: data_size


def test_rfsignal_front_end_refusals():
    conf = cases.real_signal_conf("x")
    for bad in (dict(decimation=0), dict(decimation=65), dict(decimation=5),                 # 8184 is no multiple of 5
                dict(output_bits=12), dict(output_bits=4), dict(data_size=2), dict(data_size=4, is_complex="true"),
                dict(decimation=62, sampling_frequency=62e6),                                 # default filter: 993 taps > 512
                dict(filter_taps=0), dict(filter_taps=513), dict(filter_cutoff=0.0), dict(filter_cutoff=0.7), dict(output_gain="nan")):
        with pytest.raises(ValueError):
            RFSignal(dict(conf, **bad))
    # without the key nothing has changed: a real recording is refused, the other keys alone open nothing
    plain = {k: v for k, v in conf.items() if k != "decimation"}
    with pytest.raises(ValueError, match="real-valued recordings are not supported"):
        RFSignal(plain)
    with pytest.raises(ValueError, match="real-valued recordings are not supported"):
        RFSignal(dict(plain, output_gain=2.0, filter_taps=33, baseband_shift=0.0))
    ordinary = RFSignal(dict(plain, is_complex="true"))
    assert ordinary.frontEnd is None and ordinary.samplingFrequency == 8.184e6 and ordinary.interFrequency == 2.046e6


# ---------------------------------------------------------------------------------------------- 3. the manager
class ConvertingOracleEngine(OracleEngine):
    """The oracle-backed engine with the converter's entry points: the statement, quantised as the ring's format says --
    what the device's kernels are held to (tests/test_gpu_downconvert.py)."""

    def __init__(self):
        super().__init__()
        self.ddc_calls = dict(create=0, push=0, queue=0, destroy=0)

    def ddc_create(self, cfg):
        self.ddc_calls["create"] += 1
        return dc.Statement(cfg)

    def ddc_push(self, ddc, raw, ring_offset=0):
        self.ddc_calls["push"] += 1
        v = ddc.push(raw)
        self.iq_upload(dc.quantise(v, self.iq_fmt), ring_offset)
        return v.size

    def ddc_push_queue(self, ddc, raw, ring_offset=0):
        self.ddc_calls["queue"] += 1
        self.ddc_calls["push"] -= 1
        return self.ddc_push(ddc, raw, ring_offset)

    def ddc_reset(self, ddc):
        ddc.reset()

    def ddc_destroy(self, ddc):
        self.ddc_calls["destroy"] += 1

    def sync(self):
        pass


def test_manager_over_a_real_if_recording_equals_the_converted_recording(tmp_path):
    """Real int8 at 8.184 MHz, IF 2.046 MHz, through the converter (D = 2, 33 taps, gain 2) against the statement's output fed
    as an ordinary complex int8 recording at 4.092 MHz: acquisition, tracking and channel packets equal bit for bit."""
    sig, conv_sig, converted = cases.write_real_and_converted(tmp_path)
    ms = cases.REAL_MS
    assert converted.size == 2 * ms * 4092
    cfg = packed_cases.kaplan_config()
    eng = ConvertingOracleEngine()
    got, mgr = packed_cases.receive(sig, eng, prns=[cases.SATELLITE["prn"]], cfg=cfg, ms=ms, mode="ticks")
    want, want_mgr = packed_cases.receive(conv_sig, ConvertingOracleEngine(), prns=[cases.SATELLITE["prn"]], cfg=cfg, ms=ms, mode="ticks")
    assert mgr.sharedBuffer.fmt == 0 and mgr.sharedBuffer.maxSize == 100 * 4092          # a ci8 ring at the output rate
    assert len(got) == len(want) == ms
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, k
    assert packed_cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 1
    assert packed_cases.count(got) > 40                                                   # ... and tracked
    assert np.array_equal(eng.ring, want_mgr.engine.ring)
    assert eng.ddc_calls == dict(create=1, push=0, queue=ms, destroy=0)
    assert want_mgr.engine.ddc_calls == dict(create=0, push=0, queue=0, destroy=0)        # an ordinary recording never meets it
    mgr.close()
    assert eng.ddc_calls["destroy"] == 1
    # the satellite sits where the filter's group delay puts it: (T - 1) / (2 D) = 8 output samples behind the same satellite
    # synthesised at the output rate, in the same Doppler bin
    fs = 4.092e6
    n = orc.samples_per_code(fs)
    code = orc.gold_code(cases.SATELLITE["prn"])
    rf = orc.iq_to_complex(converted[:2 * n].astype(np.float64)).reshape(1, -1)
    peak, ratio = orc.two_peak_compare(orc.pcps_map(rf, 0.0, fs, orc.code_spectrum(code, fs), 5000.0, 250.0, n), n, round(fs / orc.CODE_RATE))
    direct = orc.iq_to_complex(orc.synth_iq(fs, n, [cases.SATELLITE], 0.0, 1).astype(np.float64)).reshape(1, -1)
    peak0, _ = orc.two_peak_compare(orc.pcps_map(direct, 0.0, fs, orc.code_spectrum(code, fs), 5000.0, 250.0, n), n, round(fs / orc.CODE_RATE))
    assert peak[0] == peak0[0] and abs(peak[1] - (peak0[1] + 8)) <= 1 and ratio > 3.0, (peak, peak0, ratio)


def test_manager_refusals_and_untouched_paths(tmp_path):
    sig, conv_sig, _ = cases.write_real_and_converted(tmp_path, 3)
    mgr = ChannelManager(sig, engine=ConvertingOracleEngine())
    with pytest.raises(ValueError, match="read-ahead"):
        mgr.enableReadAhead(16)
    mgr.enableReadAhead(0)
    with pytest.raises(ValueError, match="multiple of decimation"):
        mgr.addNewRFData(sig.samples(0, 8183))
    mgr.addNewRFData(sig.getMilliseconds(1))
    assert mgr.sharedBuffer.idxWrite == 4092                                              # the count is n_in / D
    with pytest.raises(ValueError, match="one device"):
        ChannelManager(sig, devices=[0, 1])
    with pytest.raises(ValueError, match="one device"):
        ChannelManager(sig, engines=[ConvertingOracleEngine(), ConvertingOracleEngine()])
    # a manager without a front end runs the class's own methods: nothing bound per instance, no converter made
    plain = ChannelManager(conv_sig, engine=ConvertingOracleEngine())
    assert "addNewRFData" not in vars(plain) and "_upload_block" not in vars(plain) and plain._ddc is None
    assert "addNewRFData" in vars(mgr) and "_upload_block" in vars(mgr)


# ---------------------------------------------------------------------------------------------- 4. the C struct
def test_ddc_cfg_layout_agrees_with_the_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(sdr_ddc_cfg),offsetof(sdr_ddc_cfg,in_fmt),offsetof(sdr_ddc_cfg,decimation),offsetof(sdr_ddc_cfg,n_taps),"
                   "offsetof(sdr_ddc_cfg,flags),offsetof(sdr_ddc_cfg,fcw),offsetof(sdr_ddc_cfg,gain),offsetof(sdr_ddc_cfg,taps));return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _lib.DdcCfg
    assert got == [C.sizeof(D), D.in_fmt.offset, D.decimation.offset, D.n_taps.offset, D.flags.offset, D.fcw.offset, D.gain.offset, D.taps.offset]
    assert got == [40, 0, 4, 8, 12, 16, 24, 32]
    assert (_lib.DDC_IN_R8, _lib.DDC_IN_R16, _lib.DDC_IN_CI8, _lib.DDC_IN_CI16) == (dc.IN_R8, dc.IN_R16, dc.IN_CI8, dc.IN_CI16)
    lib = _lib.load()
    for name in ("sdr_ddc_create", "sdr_ddc_destroy", "sdr_ddc_reset", "sdr_ddc_push", "sdr_ddc_push_queue", "sdr_ddc_out_count"):
        assert hasattr(lib, name)
    assert lib.sdr_ddc_out_count(None, 10) == -1                                           # (host arithmetic: refuses without a GPU too)


# ---------------------------------------------------------------------------------------------- 5. the index arithmetic
@host_check.requires_hipcc
def test_tile_history_and_ring_arithmetic_on_the_host():
    """sydr_amd/csrc/ddc_tiles.h, the arithmetic the converter's kernels and its host side share, compiled for the host alone
    and checked exhaustively over small T, D, tile, push length, ring offset and capacity (tests/csrc/ddc_tiles_check.hip)."""
    exe = host_check.build("ddc_tiles_check")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 100000
