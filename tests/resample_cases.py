"""Shared inputs, settings and references of the rational-resampler tests (test_resample.py, test_gpu_resample.py).

Streams, frequency words and gains are the converter tests' own (downconvert_cases.py): seeded streams, an irrational gain
and taps that are never dyadic, so that no statement output lies near a rounding tie -- which every integer-ring test asserts
before it demands byte equality.  A statement is computed once per (input format, L, M, T, fcw, gain) and shared (lru_cache,
the arrays read-only).  `Frozen` is the parent's Statement, kept word for word: what L = 1 must still compute."""
from functools import lru_cache

import numpy as np

import downconvert_cases as dcases

from sydr_amd.signal import downconvert as dc

SEED = dcases.SEED
N_INPUTS = dcases.N_INPUTS             # 70 001: several tiles of every case, the last one ragged
FCWS = dcases.FCWS
# (L, M, T).  (8,3,5): T < L, phases 5..7 have no tap (K_p = 0: gain * 0.0); (6,4,25): gcd 2
SMALL = [(3, 2, 7), (2, 3, 33), (5, 4, 43), (8, 3, 5), (6, 4, 25), (250, 341, 1500)]
# the ends of the domain: L = 1024 with two taps per phase; M = 64 L; Tp = 512 with the longest prototype
EDGES = [(1024, 1023, 2048), (16, 1024, 512), (64, 1, 32768)]
CPU_SHAPES = [(3, 2, 7), (2, 3, 33), (5, 4, 43), (8, 3, 5), (250, 341, 1500)]


def shape_id(s) -> str:
    return f"L{s[0]}_M{s[1]}_T{s[2]}"


def taps_for(L: int, M: int, T: int) -> np.ndarray:
    """A Kaiser-windowed sinc of T taps at the default cutoff, sum(h) = L."""
    return dc.design_resampler(L, M, T)


def config(in_fmt: int, L: int, M: int, T: int, fcw: int, gain: float) -> dc.DownConverterConfig:
    return dc.DownConverterConfig(in_fmt, M, taps_for(L, M, T), fcw, gain, L)


@lru_cache(maxsize=96)
def reference(in_fmt: int, L: int, M: int, T: int, fcw: int, gain: float, n: int = N_INPUTS) -> np.ndarray:
    """The statement's outputs of dcases.stream(in_fmt, n) in one push, complex128, read-only."""
    v = dc.statement(config(in_fmt, L, M, T, fcw, gain), [dcases.stream(in_fmt, n)])
    v.setflags(write=False)
    return v


def push_lengths(Tp: int) -> list:
    """In inputs; then the rest."""
    return [1, 2, 3, max(Tp - 2, 0), max(Tp - 1, 0), Tp, 0, Tp + 1, 4097]


def zero_stuffed(cfg: dc.DownConverterConfig, raw: np.ndarray) -> np.ndarray:
    """The independent formulation: mix (the statement's phasor, written out again), zero-stuff by L, np.convolve with h, keep
    every M-th sample, times gain."""
    L, M = cfg.interpolation, cfg.decimation
    x = raw.astype(np.float64)
    x = x[0::2] + 1j * x[1::2] if dc.input_is_complex(cfg.in_fmt) else x + 0j
    j = np.arange(x.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        turn = ((j * np.uint64(cfg.fcw)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    z = x * np.exp(-2j * np.pi * turn)
    up = np.zeros(x.size * L, dtype=np.complex128)
    up[::L] = z
    return cfg.gain * np.convolve(up, cfg.taps)[:x.size * L:M]


class Frozen:
    """The converter's statement as it stood before `interpolation` existed (integer decimation D only), its arithmetic kept
    operation for operation: what a configuration with interpolation = 1 must still return, bit for bit."""

    def __init__(self, in_fmt, D, taps, fcw, gain):
        self.in_fmt, self.D, self.taps, self.fcw, self.gain = in_fmt, int(D), np.ascontiguousarray(taps, dtype=np.float64), int(fcw), float(gain)
        self.n_seen = 0
        self._hist_re = np.zeros(self.taps.size - 1)
        self._hist_im = np.zeros(self.taps.size - 1)

    def push(self, raw) -> np.ndarray:
        T, D, N = self.taps.size, self.D, self.n_seen
        raw = np.asarray(raw).reshape(-1)
        if dc.input_is_complex(self.in_fmt):
            xr, xi = raw[0::2].astype(np.float64), raw[1::2].astype(np.float64)
        else:
            xr = raw.astype(np.float64)
            xi = np.zeros(xr.size)
        n_in = xr.size
        xr, xi = np.concatenate([self._hist_re, xr]), np.concatenate([self._hist_im, xi])
        j = (np.arange(-(T - 1), n_in, dtype=np.int64) + np.int64(N)).astype(np.uint64)
        with np.errstate(over="ignore"):
            p = j * np.uint64(self.fcw)
        t = (p >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        ph = 6.283185307179586 * t
        c, s = np.cos(ph), np.sin(ph)
        zr = xr * c + xi * s
        zi = xi * c - xr * s
        m_first = -(-N // D)
        n_out = -(-(N + n_in) // D) - m_first
        at = m_first * D - (N - (T - 1))
        ar, ai = np.zeros(n_out), np.zeros(n_out)
        if n_out:
            for k in range(T):
                h = self.taps[k]
                span = slice(at - k, at - k + (n_out - 1) * D + 1, D)
                ar = ar + h * zr[span]
                ai = ai + h * zi[span]
        ar, ai = ar * self.gain, ai * self.gain
        if T > 1:
            self._hist_re, self._hist_im = xr[-(T - 1):].copy(), xi[-(T - 1):].copy()
        self.n_seen = N + n_in
        v = np.empty(n_out, dtype=np.complex128)
        v.real, v.imag = ar, ai
        return v


# ------------------------------------------------------------------------------------------------ a 16.368 MHz recording
FS_REC, FS_RING, REC_L, REC_M, REC_MS = 16.368e6, 12e6, 250, 341, 60
SATELLITE = dcases.SATELLITE


@lru_cache(maxsize=None)
def recording(ms: int = REC_MS) -> np.ndarray:
    """One C/A satellite in noise, complex int8 at 16.368 MHz (the commodity front-end rate: 16 samples per chip); read-only."""
    from oracle import sydr_oracle as orc
    raw = orc.synth_iq(FS_REC, ms * int(FS_REC * 1e-3), [SATELLITE], 10.0, SEED + 62)
    raw.setflags(write=False)
    return raw


def recording_conf(path, **more):
    """[RFSIGNAL] of that recording: into a 12 MHz ring by 250 / 341 with the default prototype, gain 2."""
    conf = dict(filepath=str(path), sampling_frequency=FS_REC, is_complex="true", intermediate_frequency=0.0, data_size=8,
                decimation=REC_M, interpolation=REC_L, output_gain=2.0)
    conf.update(more)
    return conf


def write_recording_and_converted(tmp_path, ms: int = REC_MS):
    """-> (RFSignal over the 16.368 MHz file, RFSignal over the statement's output stored as an ordinary complex int8 recording at
    12 MHz, that output as int8 I,Q)"""
    from sydr_amd.signal.iqsource import RFSignal
    rec_path, conv_path = tmp_path / "rec_16368.bin", tmp_path / "converted_12000.bin"
    recording(ms).tofile(rec_path)
    sig = RFSignal(recording_conf(rec_path))
    converted = dc.statement(sig.frontEnd.config, [recording(ms)], dc.FMT_CI8)
    converted.tofile(conv_path)
    plain = RFSignal(dict(filepath=str(conv_path), sampling_frequency=FS_RING, is_complex="true", intermediate_frequency=0.0, data_size=8))
    return sig, plain, converted
