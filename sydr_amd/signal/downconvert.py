"""The digital down-converter between a recording and the ring, as NumPy: what the device must leave in the ring.

Mixer, FIR low-pass, decimator -- for real or complex recordings at an intermediate frequency and for wide-band recordings.
The device form is sydr_amd/csrc/ddc.hip (sdr_ddc_* in include/sydr_amd.h, Engine.ddc_*); this file is its only yardstick.

Input samples are counted j = 0, 1, ... from creation or reset, across pushes; x_j is the sample as a complex number
(imaginary part 0 for real recordings), x_j = 0 for j < 0:

    p_j = (j * fcw) mod 2^64                    (uint64 wrap)
    t_j = (p_j >> 11) * 2^-53                   (exact in a double, in [0, 1))
    z_j = x_j * (cos 2 pi t_j - i sin 2 pi t_j)
    v_m = gain * sum_{k < T} h_k * z_{m D - k}  m = 0, 1, ...

A push of n_in inputs whose first has index N yields exactly the outputs m with N <= m D < N + n_in.

With `interpolation` L > 1 the converter resamples by L / M (M = `decimation`): zero-stuffing by L, the prototype filter
h[0..T-1] at the up-sampled rate, every M-th sample kept -- of which only the non-zero products are formed.  The mixer is
unchanged (p_j, t_j, z_j are functions of the INPUT index j alone); for output m = 0, 1, ...:

    u = m * M      q = u div L      p = u mod L      K_p = ceil((T - p) / L)   (0 when p >= T)
    v_m = gain * sum_{k < K_p} h[p + k L] * z_{q - k}                            (k ascending; K_p = 0 gives gain * 0.0)

and a push yields exactly the outputs m with N L <= m M < (N + n_in) L, that is N <= q_m < N + n_in.  The history is the last
ceil(T / L) - 1 raw inputs.  Limits: L in 1..1024, M in 1..1024 with M <= 64 L, T in 1..32768 with ceil(T / L) <= 512; L = 1 is
the converter above, operation for operation.  The device form of L > 1 is sydr_amd/csrc/resample.hip.

Float rings store v
(cf32: rounded to nearest float), integer rings clip(rint(v)), ties to even, clip +-127 (ci8) / +-32767 (ci16).
Every operation below is one IEEE fp64 operation on real arrays in a fixed order (k ascending, product then sum), and the
phasor depends on j alone: the result does not depend on how the stream is cut into pushes, bit for bit.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

IN_R8, IN_R16, IN_CI8, IN_CI16 = 0, 1, 2, 3            # sdr_ddc_input
FMT_CI8, FMT_CI16, FMT_CF32, FMT_CF64 = 0, 1, 2, 3     # sdr_iq_format (the ring's)
MAX_TAPS, MAX_DECIMATION = 512, 64                     # of a converter without interpolation, and of a phase (ceil(T / L))
MAX_INTERPOLATION, MAX_RATIONAL_DECIMATION, MAX_PROTOTYPE_TAPS = 1024, 1024, 32768
_IN_DTYPE = {IN_R8: np.int8, IN_R16: np.int16, IN_CI8: np.int8, IN_CI16: np.int16}
_TWO_PI = 6.283185307179586


def input_is_complex(in_fmt: int) -> bool:
    return in_fmt in (IN_CI8, IN_CI16)


def input_dtype(in_fmt: int):
    return _IN_DTYPE[in_fmt]


def frequency_word(shift_hz, fs_in) -> int:
    """round(shift_hz / fs_in * 2^64) mod 2^64 in exact rational arithmetic (the floats are taken for what they hold)."""
    if not fs_in > 0:
        raise ValueError("fs_in must be positive")
    return int(round(Fraction(shift_hz) / Fraction(fs_in) * (1 << 64))) % (1 << 64)


def design_lowpass(n_taps: int, cutoff: float, beta: float = 8.0) -> np.ndarray:
    """Kaiser-windowed sinc: n_taps taps, cutoff as a fraction of the INPUT rate (0 < cutoff <= 0.5), unit DC gain.
    n_taps = 1 is no filter: [1]."""
    n_taps = int(n_taps)
    if not 1 <= n_taps <= MAX_TAPS:
        raise ValueError(f"{n_taps} taps outside 1..{MAX_TAPS}")
    if not 0.0 < cutoff <= 0.5:
        raise ValueError("cutoff is a fraction of the input rate in (0, 0.5]")
    if n_taps == 1:
        return np.ones(1)
    n = np.arange(n_taps) - (n_taps - 1) / 2.0
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * n) * np.kaiser(n_taps, beta)
    return h / h.sum()


def design_resampler(L: int, M: int, n_taps=None, cutoff=None, beta: float = 8.0) -> np.ndarray:
    """The prototype filter of a resampler by L / M: a Kaiser-windowed sinc at the UP-SAMPLED rate (L times the input's),
    n_taps taps (default 16 max(L, M) + 1), cutoff a fraction of the up-sampled rate (default 0.45 / max(L, M)), scaled to
    sum(h) = L: every phase h[p::L] then has about unit DC gain and `gain` keeps its meaning."""
    L, M = int(L), int(M)
    if not (1 <= L <= MAX_INTERPOLATION and 1 <= M <= MAX_RATIONAL_DECIMATION and M <= MAX_DECIMATION * L):
        raise ValueError(f"interpolation {L} / decimation {M} outside 1..{MAX_INTERPOLATION} / 1..{MAX_RATIONAL_DECIMATION}, "
                         f"M <= {MAX_DECIMATION} L")
    n_taps = 16 * max(L, M) + 1 if n_taps is None else int(n_taps)
    cutoff = 0.45 / max(L, M) if cutoff is None else float(cutoff)
    if not (1 <= n_taps <= MAX_PROTOTYPE_TAPS and -(-n_taps // L) <= MAX_TAPS):
        raise ValueError(f"{n_taps} taps outside 1..{MAX_PROTOTYPE_TAPS} or more than {MAX_TAPS} per phase of {L}")
    if not 0.0 < cutoff <= 0.5:
        raise ValueError("cutoff is a fraction of the up-sampled rate in (0, 0.5]")
    if n_taps == 1:
        return np.full(1, float(L))
    n = np.arange(n_taps) - (n_taps - 1) / 2.0
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * n) * np.kaiser(n_taps, beta)
    return h * (L / h.sum())


@dataclass
class DownConverterConfig:
    in_fmt: int
    decimation: int = 1
    taps: np.ndarray = field(default_factory=lambda: np.ones(1))
    fcw: int = 0
    gain: float = 1.0
    interpolation: int = 1

    def __post_init__(self):
        self.taps = np.ascontiguousarray(self.taps, dtype=np.float64).reshape(-1)
        self.decimation, self.fcw, self.gain = int(self.decimation), int(self.fcw), float(self.gain)
        self.interpolation = int(self.interpolation)
        if self.in_fmt not in _IN_DTYPE:
            raise ValueError(f"unknown input format {self.in_fmt}")
        L = self.interpolation
        if not 1 <= L <= MAX_INTERPOLATION:
            raise ValueError(f"interpolation {L} outside 1..{MAX_INTERPOLATION}")
        if not 1 <= self.decimation <= min(MAX_DECIMATION * L, MAX_RATIONAL_DECIMATION):
            raise ValueError(f"decimation {self.decimation} outside 1..{min(MAX_DECIMATION * L, MAX_RATIONAL_DECIMATION)}")
        if not (1 <= self.taps.size <= MAX_PROTOTYPE_TAPS and self.phase_taps <= MAX_TAPS):
            raise ValueError(f"{self.taps.size} taps outside 1..{min(MAX_TAPS * L, MAX_PROTOTYPE_TAPS)}")
        if not (np.all(np.isfinite(self.taps)) and np.isfinite(self.gain)):
            raise ValueError("taps and gain must be finite")
        if not 0 <= self.fcw < 1 << 64:
            raise ValueError("fcw is an unsigned 64-bit word")

    @property
    def n_taps(self) -> int:
        return int(self.taps.size)

    @property
    def phase_taps(self) -> int:
        """Tp = ceil(T / L): the taps of the longest phase, one more than the history holds."""
        return -(-int(self.taps.size) // self.interpolation)

    @property
    def group_delay(self) -> float:
        """Of a symmetric filter, in INPUT samples."""
        return (self.n_taps - 1) / (2.0 * self.interpolation)


def out_count(n_seen: int, n_in: int, decimation: int, interpolation: int = 1) -> int:
    """Outputs of a push of n_in inputs behind n_seen earlier ones: the m with n_seen L <= m M < (n_seen + n_in) L."""
    return -(-(n_seen + n_in) * interpolation // decimation) - -(-n_seen * interpolation // decimation)


def quantise(v: np.ndarray, ring_fmt: int) -> np.ndarray:
    """Outputs `v` (complex128) as a ring of format ring_fmt holds them: interleaved [re, im, ...] in the ring's type."""
    pair = np.empty(2 * v.size, dtype=np.float64)
    pair[0::2], pair[1::2] = v.real, v.imag
    if ring_fmt == FMT_CF64:
        return pair
    if ring_fmt == FMT_CF32:
        return pair.astype(np.float32)
    lim, dtype = (127.0, np.int8) if ring_fmt == FMT_CI8 else (32767.0, np.int16)
    return np.clip(np.rint(pair), -lim, lim).astype(dtype)


class Statement:
    """The statement with its state: the last ceil(T / L) - 1 raw inputs and the count of inputs, carried from push to push."""

    def __init__(self, cfg: DownConverterConfig):
        self.cfg = cfg
        self.reset()

    def reset(self):
        self.n_seen = 0
        self._hist_re = np.zeros(self.cfg.phase_taps - 1)
        self._hist_im = np.zeros(self.cfg.phase_taps - 1)

    def out_count(self, n_in: int) -> int:
        return out_count(self.n_seen, int(n_in), self.cfg.decimation, self.cfg.interpolation)

    def push(self, raw) -> np.ndarray:
        """`raw`: the inputs as the recording holds them (real: one integer each; complex: interleaved I, Q).  Returns the
        outputs v of this push as complex128."""
        cfg = self.cfg
        T, M, L, N = cfg.n_taps, cfg.decimation, cfg.interpolation, self.n_seen
        Tp = cfg.phase_taps
        raw = np.asarray(raw).reshape(-1)
        if input_is_complex(cfg.in_fmt):
            xr, xi = raw[0::2].astype(np.float64), raw[1::2].astype(np.float64)
        else:
            xr = raw.astype(np.float64)
            xi = np.zeros(xr.size)
        n_in = xr.size
        # inputs N - (Tp-1) .. N + n_in - 1: the history, then the push
        xr, xi = np.concatenate([self._hist_re, xr]), np.concatenate([self._hist_im, xi])
        j = (np.arange(-(Tp - 1), n_in, dtype=np.int64) + np.int64(N)).astype(np.uint64)     # (j < 0 wraps: x = 0 there)
        with np.errstate(over="ignore"):
            p = j * np.uint64(cfg.fcw)
        t = (p >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        ph = _TWO_PI * t
        c, s = np.cos(ph), np.sin(ph)
        zr = xr * c + xi * s
        zi = xi * c - xr * s
        m_first, n_out = -(-N * L // M), out_count(N, n_in, M, L)
        # outputs L' = L / gcd apart share their phase and lie M' = M / gcd inputs apart: one strided pass per phase (L = 1: one)
        g = math.gcd(L, M)
        Lp, Mp = L // g, M // g
        v = np.empty(n_out, dtype=np.complex128)
        for first in range(min(Lp, n_out)):
            q, phase = divmod((m_first + first) * M, L)
            count = len(range(first, n_out, Lp))
            at = q - (N - (Tp - 1))                  # position of input q in the arrays above; this phase's output i: at + i M'
            ar, ai = np.zeros(count), np.zeros(count)
            for k in range(-(-(T - phase) // L) if phase < T else 0):
                h = cfg.taps[phase + k * L]
                span = slice(at - k, at - k + (count - 1) * Mp + 1, Mp)
                ar = ar + h * zr[span]
                ai = ai + h * zi[span]
            ar, ai = ar * cfg.gain, ai * cfg.gain
            v.real[first::Lp], v.imag[first::Lp] = ar, ai
        if Tp > 1:
            self._hist_re, self._hist_im = xr[-(Tp - 1):].copy(), xi[-(Tp - 1):].copy()
        self.n_seen = N + n_in
        return v


def statement(cfg: DownConverterConfig, pushes, ring_fmt=None, state: Statement | None = None):
    """The outputs of a list of pushes (one array of raw inputs each), concatenated; `state` carries history and index from
    an earlier call (default: a fresh converter).  ring_fmt given: as that ring holds them (`quantise`)."""
    st = state if state is not None else Statement(cfg)
    parts = [st.push(raw) for raw in pushes]
    v = np.concatenate(parts) if parts else np.zeros(0, dtype=np.complex128)
    return v if ring_fmt is None else quantise(v, ring_fmt)


def tolerance(cfg: DownConverterConfig, max_abs_x: float) -> float:
    """gain * B, B = (Tp + 16) * 2^-53 * max_p sum_k |h[p + k L]| * max|x|, Tp = ceil(T / L): what any order of a phase's
    fp64 products and sums keeps of an output component, plus a few ulp for the phasor.  (L = 1: T and sum|h|.)"""
    L = cfg.interpolation
    h_sum = max(float(np.sum(np.abs(cfg.taps[p::L]))) for p in range(min(L, cfg.n_taps)))
    return abs(cfg.gain) * (cfg.phase_taps + 16) * 2.0 ** -53 * h_sum * float(max_abs_x)


def ambiguous(v: np.ndarray, band: float) -> int:
    """Components of the outputs v within `band` of a half-integer: where clip(rint(.)) of two computations may differ."""
    pair = np.concatenate([v.real, v.imag])
    return int(np.count_nonzero(np.abs(np.abs(pair - np.floor(pair)) - 0.5) <= band))
