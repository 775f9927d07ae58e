"""Shared inputs, seeds and converter settings of the down-converter tests (test_downconvert.py, test_gpu_downconvert.py).

Every stream is seeded; a statement is computed once per (input format, T, D, fcw, gain) and shared (lru_cache, the arrays
read-only).  Taps are never exactly dyadic and the gain is irrational, so that no statement output lies near a rounding
tie -- which every integer-ring test asserts before it demands byte equality -- except in the pass-through case
(T = 1, h = [1], D = 1, fcw = 0, gain = 1), which is exact on both sides."""
from functools import lru_cache

import numpy as np

from sydr_amd.signal import downconvert as dc

SEED = 20260018
N_INPUTS = 70001                       # several tiles of every (T, D), the last one ragged
IN_FORMATS = [dc.IN_R8, dc.IN_R16, dc.IN_CI8, dc.IN_CI16]
IN_NAMES = {dc.IN_R8: "r8", dc.IN_R16: "r16", dc.IN_CI8: "ci8", dc.IN_CI16: "ci16"}
RING_FORMATS = [dc.FMT_CI8, dc.FMT_CI16, dc.FMT_CF32, dc.FMT_CF64]
RING_NAMES = {dc.FMT_CI8: "ci8", dc.FMT_CI16: "ci16", dc.FMT_CF32: "cf32", dc.FMT_CF64: "cf64"}
RING_DTYPE = {dc.FMT_CI8: np.int8, dc.FMT_CI16: np.int16, dc.FMT_CF32: np.float32, dc.FMT_CF64: np.float64}
SHAPES = [(1, 1), (2, 1), (33, 2), (17, 3), (65, 5), (512, 16), (3, 64)]            # (T, D)
FS_IN = 8.184e6
FCWS = {"zero": 0, "quarter": 1 << 62, "odd": dc.frequency_word(1234567.891, FS_IN)}
GOLD = 1.618033988749895
AMPLITUDE = {dc.IN_R8: 127, dc.IN_CI8: 127, dc.IN_R16: 3000, dc.IN_CI16: 3000}


def taps_for(T: int, D: int) -> np.ndarray:
    """Kaiser-windowed sinc at the default cutoff; T = 2 would come out as [0.5, 0.5] (dyadic) and T = 1 is no filter."""
    if T == 1:
        return np.ones(1)
    if T == 2:
        return np.array([0.53, 0.47])
    return dc.design_lowpass(T, 0.45 / D)


def gain_for(in_fmt: int, ring_fmt: int) -> float:
    """Irrational; scaled so that an integer ring of the other width is neither all rails nor all zeros."""
    wide_in = in_fmt in (dc.IN_R16, dc.IN_CI16)
    if ring_fmt == dc.FMT_CI8 and wide_in:
        return GOLD / 24.0
    if ring_fmt == dc.FMT_CI16 and not wide_in:
        return GOLD * 24.0
    return GOLD


@lru_cache(maxsize=None)
def stream(in_fmt: int, n: int = N_INPUTS, seed: int = SEED) -> np.ndarray:
    """n raw inputs of the format (complex ones interleaved), uniformly over +-AMPLITUDE; read-only."""
    rng = np.random.default_rng(seed + 17 * in_fmt)
    a = AMPLITUDE[in_fmt]
    count = 2 * n if dc.input_is_complex(in_fmt) else n
    raw = rng.integers(-a, a + 1, count).astype(dc.input_dtype(in_fmt))
    raw.setflags(write=False)
    return raw


def max_abs(in_fmt: int, raw: np.ndarray) -> float:
    x = raw.astype(np.float64)
    return float(np.max(np.hypot(x[0::2], x[1::2]))) if dc.input_is_complex(in_fmt) else float(np.max(np.abs(x)))


def config(in_fmt: int, T: int, D: int, fcw: int, gain: float) -> dc.DownConverterConfig:
    return dc.DownConverterConfig(in_fmt, D, taps_for(T, D), fcw, gain)


@lru_cache(maxsize=64)
def reference(in_fmt: int, T: int, D: int, fcw: int, gain: float, n: int = N_INPUTS) -> np.ndarray:
    """The statement's outputs of stream(in_fmt, n) in one push, complex128, read-only."""
    v = dc.statement(config(in_fmt, T, D, fcw, gain), [stream(in_fmt, n)])
    v.setflags(write=False)
    return v


def cut(raw: np.ndarray, in_fmt: int, lengths) -> list:
    """The stream cut into pushes of the given lengths (in inputs), then the rest."""
    w = 2 if dc.input_is_complex(in_fmt) else 1
    out, at = [], 0
    for n in lengths:
        out.append(raw[w * at:w * (at + n)])
        at += n
    out.append(raw[w * at:])
    return out


def push_lengths(T: int) -> list:
    return [1, 2, 3, max(T - 2, 0), max(T - 1, 0), T, 0, T + 1, 4097]


# ------------------------------------------------------------------------------------------------ a real IF recording
FS_REAL, IF_REAL, REAL_MS = 8.184e6, 2.046e6, 60
SATELLITE = dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=30.0)


@lru_cache(maxsize=None)
def real_if_recording(ms: int = REAL_MS) -> np.ndarray:
    """One C/A satellite in noise, real int8 at 8.184 MHz with the carrier at IF = fs / 4: r_n = Re((I_n + i Q_n) e^{+i pi n / 2})
    of the oracle's complex baseband stream at that rate (the phasor takes the values 1, i, -1, -i: exact)."""
    from oracle import sydr_oracle as orc
    n = ms * int(FS_REAL * 1e-3)
    raw = orc.synth_iq(FS_REAL, n, [SATELLITE], 10.0, SEED + 60)
    i, q = raw[0::2].astype(np.int64), raw[1::2].astype(np.int64)
    r = np.choose(np.arange(n) % 4, [i, -q, -i, q])
    r = np.clip(r, -127, 127).astype(np.int8)
    r.setflags(write=False)
    return r


def real_signal_conf(path, **more):
    """[RFSIGNAL] of that recording: through the converter with the default filter (33 taps, cutoff 0.225), gain 2."""
    conf = dict(filepath=str(path), sampling_frequency=FS_REAL, is_complex="", intermediate_frequency=IF_REAL, data_size=8,
                decimation=2, output_gain=2.0)
    conf.update(more)
    return conf


def converted_signal_conf(path):
    """[RFSIGNAL] of the statement's output of that recording, stored as an ordinary complex int8 file at 4.092 MHz."""
    return dict(filepath=str(path), sampling_frequency=FS_REAL / 2, is_complex="true", intermediate_frequency=0.0, data_size=8)


def write_real_and_converted(tmp_path, ms: int = REAL_MS):
    """-> (RFSignal over the real file, RFSignal over the statement's output file, the statement's output as int8 I,Q)"""
    from sydr_amd.signal.iqsource import RFSignal
    real_path, conv_path = tmp_path / "real_if.bin", tmp_path / "converted_ci8.bin"
    real_if_recording(ms).tofile(real_path)
    sig = RFSignal(real_signal_conf(real_path))
    converted = dc.statement(sig.frontEnd.config, [real_if_recording(ms)], dc.FMT_CI8)
    converted.tofile(conv_path)
    return sig, RFSignal(converted_signal_conf(conv_path)), converted
