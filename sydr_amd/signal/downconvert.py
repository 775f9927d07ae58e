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

With an INPUT LAYOUT (`InputLayout`, `decode`; sdr_ddc_layout in include/sydr_amd.h) the recording's bytes are described
field by field instead of by one of the four input formats:

  Fields.  A recording is a sequence of fields f = 0, 1, ..., one component each, of one kind: INT8, INT16 (native byte order),
  FLOAT32 (native) or PACKED, a code of `bits` bits (1, 2 or 4).  With F = 8 / bits, packed field f lies in byte f div F at
  position p = f mod F; its code is the `bits` bits from bit bits * p up (least significant field first) or, with msb_first,
  from bit bits * (F - 1 - p) up; the component is levels[code], an int8 -- `packing.unpack`, field for field.  Every
  component is widened to fp64, which is exact for all four kinds.
  Frames.  A frame is `stride` consecutive fields; input j of the stream is frame j: real x_j = field(j stride + lane) + 0i;
  complex a = field(j stride + lane), b = field(j stride + lane + 1), x_j = a + ib, with swap_iq x_j = b + ia.  Frames of a
  packed layout need not be whole bytes (1-bit real, stride 3 is valid).
  Limits.  stride in 1..64; lane >= 0 and lane + (2 if complex else 1) <= stride; bits 1, 2 or 4 exactly when the kind is
  PACKED, else 0; swap_iq only with complex; msb_first only with PACKED.
  Pushes.  n_in counts frames; a push reads n_in * stride * (bytes per field) bytes, packed n_in * stride * bits / 8, which
  must be a whole number (`bytes_for` raises otherwise): every push begins on a byte boundary.

From x_j on everything is the statement above; the history is the last Tp - 1 inputs decoded.  Float inputs are the caller's to
keep finite: a NaN or Inf may change only the outputs whose filter window contains it.  The layouts {INT8 real, 1, 0},
{INT16 real, 1, 0}, {INT8 complex, 2, 0}, {INT16 complex, 2, 0} are IN_R8, IN_R16, IN_CI8, IN_CI16; a packed layout is the INT8
layout on the unpacked bytes; float32 that holds integers within int16 is the INT16 layout on those integers -- bit for bit.

With an ARRAY (`DownConverterConfig.array`, signal/array.py) the K elements of a frame are combined, x_j = w^H s_j, where the frame
is decoded; that file states the combine, the covariance and the weight rules, and from x_j on everything is this statement.

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
FIELD_INT8, FIELD_INT16, FIELD_FLOAT32, FIELD_PACKED = 0, 1, 2, 3    # sdr_ddc_field
LAYOUT_COMPLEX, LAYOUT_SWAP_IQ, LAYOUT_MSB_FIRST = 1, 2, 4           # SDR_DDC_LAYOUT_*
MAX_STRIDE = 64
_FIELD_DTYPE = {FIELD_INT8: np.int8, FIELD_INT16: np.int16, FIELD_FLOAT32: np.float32, FIELD_PACKED: np.uint8}
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


class InputLayout:
    """How a recording's bytes hold the converter's inputs (the definition at the top; sdr_ddc_layout)."""

    def __init__(self, field: int, bits: int = 0, stride=None, lane: int = 0, complex: bool = False, swap_iq: bool = False,
                 msb_first: bool = False, levels=None):
        from .packing import DEFAULT_LEVELS
        self.field, self.bits, self.lane = int(field), int(bits), int(lane)
        self.complex, self.swap_iq, self.msb_first = bool(complex), bool(swap_iq), bool(msb_first)
        self.stride = (2 if self.complex else 1) if stride is None else int(stride)
        if self.field not in _FIELD_DTYPE:
            raise ValueError(f"unknown field kind {field}")
        if self.field == FIELD_PACKED:
            if self.bits not in (1, 2, 4):
                raise ValueError(f"packed fields have 1, 2 or 4 bits, not {bits}")
        elif self.bits != 0:
            raise ValueError("bits is 0 unless the fields are packed")
        if not 1 <= self.stride <= MAX_STRIDE:
            raise ValueError(f"stride {self.stride} outside 1..{MAX_STRIDE}")
        if self.lane < 0 or self.lane + (2 if self.complex else 1) > self.stride:
            raise ValueError(f"lane {self.lane} of a {'complex' if self.complex else 'real'} stream does not fit a frame of {self.stride} fields")
        if self.swap_iq and not self.complex:
            raise ValueError("swap_iq needs a complex stream")
        if self.msb_first and self.field != FIELD_PACKED:
            raise ValueError("msb_first needs packed fields")
        if self.field == FIELD_PACKED:
            levels = DEFAULT_LEVELS[self.bits] if levels is None else tuple(int(v) for v in levels)
            if len(levels) != 1 << self.bits:
                raise ValueError(f"{self.bits}-bit fields need {1 << self.bits} levels, {len(levels)} given")
            if any(not -128 <= v <= 127 for v in levels):
                raise ValueError("levels are int8")
        elif levels is not None:
            raise ValueError("levels need packed fields")
        self.levels = np.array(levels if levels is not None else (), dtype=np.int8)
        self.levels.setflags(write=False)

    @property
    def flags(self) -> int:
        return (LAYOUT_COMPLEX if self.complex else 0) | (LAYOUT_SWAP_IQ if self.swap_iq else 0) | (LAYOUT_MSB_FIRST if self.msb_first else 0)

    @property
    def dtype(self):
        """Of the arrays a push takes: uint8 for packed fields, else the field's own."""
        return _FIELD_DTYPE[self.field]

    @property
    def field_bits(self) -> int:
        return self.bits if self.field == FIELD_PACKED else 8 * np.dtype(self.dtype).itemsize

    @property
    def frame_bits(self) -> int:
        return self.stride * self.field_bits

    @property
    def frame_group(self) -> int:
        """The fewest frames that are whole bytes: 8 / gcd(8, stride * bits) of a packed layout, else 1."""
        return 8 // math.gcd(8, self.frame_bits)

    def bytes_for(self, n_in: int) -> int:
        """Bytes a push of n_in frames reads; ValueError when n_in < 0 or they are not whole."""
        n_in = int(n_in)
        if n_in < 0:
            raise ValueError("negative input count")
        total = n_in * self.frame_bits
        if total % 8:
            raise ValueError(f"{n_in} frames of {self.stride} fields of {self.field_bits} bit(s) are not whole bytes")
        return total // 8

    def frames_in(self, n_bytes: int) -> int:
        """The frames n_bytes hold, which must be whole frames (the inverse of bytes_for)."""
        total = 8 * int(n_bytes)
        if total % self.frame_bits:
            raise ValueError(f"{n_bytes} bytes are not whole frames of {self.stride} fields of {self.field_bits} bit(s)")
        return total // self.frame_bits

    def input_array(self, raw) -> np.ndarray:
        """`raw` as a push takes it: contiguous, 1-D, of `dtype`, whole frames; ValueError otherwise."""
        if not (isinstance(raw, np.ndarray) and raw.ndim == 1 and raw.flags.c_contiguous and raw.dtype == self.dtype):
            raise ValueError(f"a push takes a contiguous 1-D {np.dtype(self.dtype).name} array of the recording's bytes")
        self.frames_in(raw.nbytes)
        return raw

    def __eq__(self, other):
        return (isinstance(other, InputLayout) and (self.field, self.bits, self.stride, self.lane, self.flags) ==
                (other.field, other.bits, other.stride, other.lane, other.flags) and np.array_equal(self.levels, other.levels))

    def __hash__(self):
        return hash((self.field, self.bits, self.stride, self.lane, self.flags, self.levels.tobytes()))

    def __repr__(self):
        return (f"InputLayout(field={self.field}, bits={self.bits}, stride={self.stride}, lane={self.lane}, complex={self.complex}, "
                f"swap_iq={self.swap_iq}, msb_first={self.msb_first}, levels={tuple(int(v) for v in self.levels)})")


def fields(raw, layout: InputLayout) -> np.ndarray:
    """Every field the bytes of `raw` hold, in order, in the component's own type (packed: int8, `packing.unpack` itself)."""
    raw = np.ascontiguousarray(raw).reshape(-1)
    if layout.field != FIELD_PACKED:
        return raw.view(np.uint8).view(layout.dtype) if raw.dtype != layout.dtype else raw
    from .packing import Packing, unpack
    return unpack(raw.view(np.uint8), Packing(layout.bits, layout.levels, layout.msb_first))


def decode(raw, layout: InputLayout):
    """The inputs x_j = xr_j + i xi_j (float64 each) of the frames in `raw`, the recording's bytes of one push."""
    raw = np.ascontiguousarray(raw).reshape(-1)
    n_in = layout.frames_in(raw.nbytes)
    f = fields(raw, layout)
    at = np.arange(n_in, dtype=np.int64) * layout.stride + layout.lane
    a = f[at].astype(np.float64)
    if not layout.complex:
        return a, np.zeros(n_in)
    b = f[at + 1].astype(np.float64)
    return (b, a) if layout.swap_iq else (a, b)


@dataclass
class DownConverterConfig:
    in_fmt: int
    decimation: int = 1
    taps: np.ndarray = field(default_factory=lambda: np.ones(1))
    fcw: int = 0
    gain: float = 1.0
    interpolation: int = 1
    layout: InputLayout | None = None      # an input layout: in_fmt is then not consulted
    array: object | None = None            # signal.array.ArrayGeometry: the K elements of a frame combined (needs a layout)

    def __post_init__(self):
        self.taps = np.ascontiguousarray(self.taps, dtype=np.float64).reshape(-1)
        self.decimation, self.fcw, self.gain = int(self.decimation), int(self.fcw), float(self.gain)
        self.interpolation = int(self.interpolation)
        if self.layout is not None:
            if not isinstance(self.layout, InputLayout):
                raise ValueError("layout is an InputLayout")
        elif self.in_fmt not in _IN_DTYPE:
            raise ValueError(f"unknown input format {self.in_fmt}")
        if self.array is not None:
            from .array import ArrayGeometry
            if not isinstance(self.array, ArrayGeometry):
                raise ValueError("array is an ArrayGeometry")
            if self.layout is None:
                raise ValueError("an array needs an input layout")
            self.array.check(self.layout)
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
        """`raw`: the inputs as the recording holds them (real: one integer each; complex: interleaved I, Q; with a layout:
        the bytes of whole frames, `decode`d).  Returns the outputs v of this push as complex128."""
        cfg = self.cfg
        T, M, L, N = cfg.n_taps, cfg.decimation, cfg.interpolation, self.n_seen
        Tp = cfg.phase_taps
        raw = np.asarray(raw).reshape(-1)
        if cfg.layout is not None:
            xr, xi = decode(raw, cfg.layout)
        elif input_is_complex(cfg.in_fmt):
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
