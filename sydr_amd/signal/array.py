"""Antenna arrays in the down-converter, as NumPy: what the device must leave in the ring, and in the covariance.

A multi-antenna front end writes a recording that interleaves its K elements frame by frame; with weights w the converter
forms x = w^H s where it decodes the frame and a broadband jammer -- no time structure for the blanker, no spectral line for
the excisor -- falls into a spatial null.  The device form is sydr_amd/csrc/ddc_array.h (the decode and the combine, in
ddc_kernel / resample_kernel) and ddc_array.hip (the covariance pass); sdr_ddc_create_array in include/sydr_amd.h,
Engine.ddc_create with `cfg.array`.  This file is its only yardstick.

An ARRAY is a layout (`downconvert.InputLayout`) plus K elements, K in 2..8, element a at lane lanes[a] of the frame: distinct
lanes, lanes[a] + (2 if complex else 1) <= stride, in any order, adjacent or not; the layout's own lane is not read.  Element
a of frame j is decoded exactly as the layout decodes a stream at that lane (`downconvert.decode`):

    s_{a,j} = sr + i si                         (si = 0 for a real layout; swap_iq honoured)

Weights are w_a = wr_a + i wi_a, finite doubles.  The converter's input is x_j = sum_a conj(w_a) s_{a,j}, formed in fp64 in
this order and no other, every product rounded, every sum rounded, no contraction (`combine`):

    re = 0.0; im = 0.0
    for a = 0 .. K-1:
        re = re + wr_a*sr_a;  re = re + wi_a*si_a
        im = im + wr_a*si_a;  im = im - wi_a*sr_a

From x_j on everything is the converter's statement (downconvert.py): p_j, t_j, z_j, v_m, the resampler's form, the ring's
formats -- `Statement` here IS downconvert.Statement fed the combined inputs.  Weights belong to input indices: a change
(`Statement.set_weights`) takes effect with the first input of the next push, earlier inputs keep the x_j they had, those in
the filter's history included -- the history holds the last Tp - 1 COMBINED inputs.  With the changes at the same input
indices the ring does not depend on how the stream was cut into pushes, bit for bit.

Covariance (opt-in, `measure`; SDR_DDC_ARRAY_MEASURE).  Over the inputs j pushed since creation, reset or the last clearing
read:

    R[a][b] = sum_j s_{a,j} conj(s_{b,j}):   re = sum(sr_a sr_b + si_a si_b)   im = sum(si_a sr_b - sr_a si_b)   n = their number

For INT8, INT16 and PACKED fields the sums are exact int64 integers, each converted to double once at the read (np.int64 sums,
then astype(float64)): device and statement are equal.  For FLOAT32 fields the device adds in fp64 in an order of its own and
may differ by at most 2 n 2^-52 sum_j (|sr_a sr_b| + |si_a si_b|) per component (`covariance_bound`; n terms of two products
in any order), correspondingly for the imaginary part.

Weight rules (host only; K <= 8, numpy.linalg.solve -- the C-ABI takes weights and does not solve for them), with
Rl = R/n + loading * trace(R/n)/K * I:

    power_inversion:  w = Rl^-1 e_ref / (e_ref^H Rl^-1 e_ref)       (unit response of the reference element, least output power)
    mvdr:             w = Rl^-1 a / (a^H Rl^-1 a)                   (unit response towards the steering vector a)

BEAMS (sdr_ddc_beam_attach).  A converter with beams forms several weight sets over one push, beam b >= 1 into the ring of an
engine of its own.  There is no second formulation: beam b's ring holds what `statement` gives a converter of the same
configuration with the weights w_b, the same pushes and the same weight changes at the same input indices --
`beams_statement` is `statement` once per weight set.  `element_weights` are the K unit vectors (the element streams side by
side) and `wiener_weights` the weights R^-1 p of a signal whose per-element prompts p were measured behind them.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import downconvert as dc

MIN_ELEMENTS, MAX_ELEMENTS = 2, 8
ARRAY_MEASURE = 1                       # SDR_DDC_ARRAY_MEASURE
DEFAULT_LOADING = 1e-3


class ArrayGeometry:
    """The lanes and weights of the K elements a converter combines (sdr_ddc_array); `measure` asks for the covariance."""

    def __init__(self, lanes, weights=None, measure: bool = False):
        self.lanes = tuple(int(v) for v in lanes)
        K = len(self.lanes)
        if not MIN_ELEMENTS <= K <= MAX_ELEMENTS:
            raise ValueError(f"{K} elements outside {MIN_ELEMENTS}..{MAX_ELEMENTS}")
        if len(set(self.lanes)) != K:
            raise ValueError("the lanes of an array are distinct")
        if min(self.lanes) < 0:
            raise ValueError("a lane is negative")
        self.measure = bool(measure)
        self.weights = unit_weights(K, 0) if weights is None else weights

    @property
    def n_elements(self) -> int:
        return len(self.lanes)

    @property
    def flags(self) -> int:
        return ARRAY_MEASURE if self.measure else 0

    @property
    def weights(self) -> np.ndarray:
        return self._weights

    @weights.setter
    def weights(self, w):
        self._weights = as_weights(w, len(self.lanes))

    def check(self, layout: dc.InputLayout):
        """ValueError unless every element lies inside a frame of `layout`."""
        width = 2 if layout.complex else 1
        for lane in self.lanes:
            if lane + width > layout.stride:
                raise ValueError(f"lane {lane} of a {'complex' if layout.complex else 'real'} element does not fit a frame of {layout.stride} fields")

    def __eq__(self, other):
        return (isinstance(other, ArrayGeometry) and self.lanes == other.lanes and self.measure == other.measure and
                np.array_equal(self.weights, other.weights))

    def __hash__(self):
        return hash((self.lanes, self.measure, self.weights.tobytes()))

    def __repr__(self):
        return f"ArrayGeometry(lanes={self.lanes}, weights={self.weights.tolist()}, measure={self.measure})"


def as_weights(w, K: int) -> np.ndarray:
    """K finite complex weights, read-only complex128; `w` complex [K] or real [K][2]."""
    w = np.asarray(w)
    if w.ndim == 2 and w.shape == (K, 2) and not np.iscomplexobj(w):
        w = w[:, 0] + 1j * w[:, 1]
    w = np.array(w, dtype=np.complex128).reshape(-1)
    if w.size != K:
        raise ValueError(f"{w.size} weights for {K} elements")
    if not np.all(np.isfinite(w.real) & np.isfinite(w.imag)):
        raise ValueError("weights must be finite")
    w.setflags(write=False)
    return w


def unit_weights(K: int, a: int) -> np.ndarray:
    """e_a: 1 at element a, 0 elsewhere."""
    if not 0 <= a < K:
        raise ValueError(f"element {a} outside 0..{K - 1}")
    w = np.zeros(K, dtype=np.complex128)
    w[a] = 1.0
    return w


def element_layout(layout: dc.InputLayout, lane: int) -> dc.InputLayout:
    """`layout` with its lane replaced: the stream of one element."""
    return dc.InputLayout(layout.field, layout.bits, layout.stride, lane, layout.complex, layout.swap_iq, layout.msb_first,
                          layout.levels if layout.field == dc.FIELD_PACKED else None)


def elements(raw, layout: dc.InputLayout, lanes):
    """The K elements of the frames in `raw`: (sr, si), float64 [K][n_in] each."""
    parts = [dc.decode(raw, element_layout(layout, lane)) for lane in lanes]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def combine(sr: np.ndarray, si: np.ndarray, weights):
    """x = sum_a conj(w_a) s_a in the statement's order -> (re, im), float64 [n_in] each.  Every line is one IEEE operation per
    element of the arrays."""
    w = as_weights(weights, sr.shape[0])
    re, im = np.zeros(sr.shape[1]), np.zeros(sr.shape[1])
    for a in range(sr.shape[0]):
        wr, wi = float(w[a].real), float(w[a].imag)
        re = re + wr * sr[a]
        re = re + wi * si[a]
        im = im + wr * si[a]
        im = im - wi * sr[a]
    return re, im


def covariance(raw, layout: dc.InputLayout, lanes):
    """R [K][K] complex128 of the frames in `raw` and their number n: int64 sums converted once for integer fields, fp64 sums
    in NumPy's order for float32 fields."""
    sr, si = elements(raw, layout, lanes)
    n = sr.shape[1]
    if layout.field != dc.FIELD_FLOAT32:
        sr, si = sr.astype(np.int64), si.astype(np.int64)
        re, im = sr @ sr.T + si @ si.T, si @ sr.T - sr @ si.T              # (int64 throughout: exact)
    else:
        K = sr.shape[0]
        re = np.array([[np.sum(sr[a] * sr[b] + si[a] * si[b]) for b in range(K)] for a in range(K)])
        im = np.array([[np.sum(si[a] * sr[b] - sr[a] * si[b]) for b in range(K)] for a in range(K)])
    return re.astype(np.float64) + 1j * im.astype(np.float64), n


def covariance_bound(raw, layout: dc.InputLayout, lanes):
    """What a component of a float32 array's R may differ by between two orders of fp64 addition: (for re, for im), [K][K]
    each -- 2 n 2^-52 sum_j (|sr_a sr_b| + |si_a si_b|) and 2 n 2^-52 sum_j (|si_a sr_b| + |sr_a si_b|)."""
    sr, si = elements(raw, layout, lanes)
    n = sr.shape[1]
    ar, ai = np.abs(sr), np.abs(si)
    scale = 2.0 * n * 2.0 ** -52
    return scale * (ar @ ar.T + ai @ ai.T), scale * (ai @ ar.T + ar @ ai.T)


def _loaded(R, n, loading: float) -> np.ndarray:
    R = np.asarray(R, dtype=np.complex128)
    K = R.shape[0]
    if R.shape != (K, K) or not MIN_ELEMENTS <= K <= MAX_ELEMENTS:
        raise ValueError("R is K x K, K in 2..8")
    if not n > 0:
        raise ValueError("the covariance holds no input")
    if not loading >= 0.0:
        raise ValueError("loading is not negative")
    Rn = R / float(n)
    return Rn + loading * (np.trace(Rn).real / K) * np.eye(K)


def power_inversion(R, n, reference: int = 0, loading: float = DEFAULT_LOADING) -> np.ndarray:
    """w = Rl^-1 e_ref / (e_ref^H Rl^-1 e_ref), Rl = R/n + loading trace(R/n)/K I: the reference element passes with unit
    weight, every direction stronger than the noise is nulled."""
    Rl = _loaded(R, n, loading)
    return mvdr_loaded(Rl, unit_weights(Rl.shape[0], int(reference)))


def mvdr(R, n, steering, loading: float = DEFAULT_LOADING) -> np.ndarray:
    """w = Rl^-1 a / (a^H Rl^-1 a): unit response w^H a = 1 towards the steering vector a, least output power."""
    Rl = _loaded(R, n, loading)
    return mvdr_loaded(Rl, as_weights(steering, Rl.shape[0]))


def mvdr_loaded(Rl: np.ndarray, a: np.ndarray) -> np.ndarray:
    u = np.linalg.solve(Rl, a)
    den = np.vdot(a, u)                     # a^H Rl^-1 a, real and positive for a Hermitian positive-definite Rl
    if not (np.isfinite(den.real) and den.real > 0.0):
        raise ValueError("the loaded covariance is singular")
    return u / den.real


class Statement(dc.Statement):
    """downconvert.Statement over the combined inputs of an array: `cfg.layout` and `cfg.array` say how a push's bytes hold the
    elements.  The base class keeps the last Tp - 1 inputs it was given -- here the COMBINED ones -- so a weight change never
    reaches them.  With `measure` the covariance accumulates over the pushes."""

    def __init__(self, cfg: dc.DownConverterConfig):
        if cfg.layout is None or cfg.array is None:
            raise ValueError("an array statement needs a layout and an array")
        cfg.array.check(cfg.layout)
        self.weights = cfg.array.weights
        self._plain = dc.DownConverterConfig(dc.IN_CI16, cfg.decimation, cfg.taps, cfg.fcw, cfg.gain, cfg.interpolation)
        super().__init__(cfg)

    def reset(self):
        """History and covariance zero, j = 0; the weights stay."""
        super().reset()
        K = self.cfg.array.n_elements
        self.R, self.n = np.zeros((K, K), dtype=np.complex128), 0

    def set_weights(self, weights):
        """From the first input of the next push on."""
        self.weights = as_weights(weights, self.cfg.array.n_elements)

    def read_covariance(self, clear: bool = False):
        R, n = self.R.copy(), self.n
        if clear:
            self.R, self.n = np.zeros_like(self.R), 0
        return R, n

    def combined(self, raw):
        """The inputs x_j of the frames in `raw` under the current weights -> (re, im)."""
        sr, si = elements(raw, self.cfg.layout, self.cfg.array.lanes)
        return combine(sr, si, self.weights)

    def push(self, raw) -> np.ndarray:
        raw = np.ascontiguousarray(raw).reshape(-1)
        re, im = self.combined(raw)
        if self.cfg.array.measure:
            R, n = covariance(raw, self.cfg.layout, self.cfg.array.lanes)
            # (integer fields: sums of integers below 2^53 stay exact in this addition as well)
            self.R, self.n = self.R + R, self.n + n
        return self._push_inputs(re, im)

    def _push_inputs(self, xr, xi) -> np.ndarray:
        """downconvert.Statement.push from x_j on: the base class, told that its raw inputs are these complex doubles."""
        pair = np.empty(2 * xr.size)
        pair[0::2], pair[1::2] = xr, xi
        cfg, self.cfg = self.cfg, self._plain               # (IN_CI16's branch: raw[0::2], raw[1::2] as float64 -- the doubles themselves)
        try:
            return super().push(pair)
        finally:
            self.cfg = cfg


def statement(cfg: dc.DownConverterConfig, pushes, ring_fmt=None, state: Statement | None = None, weights_at=None):
    """The outputs of a list of pushes (one array of the recording's bytes each), concatenated; weights_at: {push index: weights}
    set before that push.  ring_fmt given: as that ring holds them (`downconvert.quantise`)."""
    st = state if state is not None else Statement(cfg)
    parts = []
    for k, raw in enumerate(pushes):
        if weights_at and k in weights_at:
            st.set_weights(weights_at[k])
        parts.append(st.push(raw))
    v = np.concatenate(parts) if parts else np.zeros(0, dtype=np.complex128)
    return v if ring_fmt is None else dc.quantise(v, ring_fmt)


def with_weights(cfg: dc.DownConverterConfig, weights) -> dc.DownConverterConfig:
    """`cfg` with its array's weights replaced: the configuration of the independent converter a beam is defined by."""
    return dataclasses.replace(cfg, array=ArrayGeometry(cfg.array.lanes, weights, cfg.array.measure))


def beams_statement(cfg: dc.DownConverterConfig, weight_sets, pushes, ring_fmts=None, weights_at=None, _statement=None, _with=None):
    """What every beam's ring holds: `statement` per weight set, in its own words -> a list, beam 0 first.  weight_sets[b]: beam
    b's weights at creation / attachment; ring_fmts (optional): one ring format per beam; weights_at: {push index: {beam:
    weights}} set before that push."""
    one, replaced = _statement or statement, _with or with_weights
    out = []
    for b, w in enumerate(weight_sets):
        changes = {k: per_beam[b] for k, per_beam in (weights_at or {}).items() if b in per_beam}
        out.append(one(replaced(cfg, w), pushes, None if ring_fmts is None else ring_fmts[b], weights_at=changes))
    return out


def element_weights(K: int) -> np.ndarray:
    """The K unit vectors [K][K]: beam a of them is element a's own stream."""
    return np.stack([unit_weights(K, a) for a in range(K)])


def wiener_weights(R, p, loading: float = DEFAULT_LOADING) -> np.ndarray:
    """w = (R + loading tr(R)/K I)^-1 p: R the covariance of the elements (any common scale), p the per-element prompts of a
    tracked signal, p_a = sum_j s_a[j] conj(replica[j]) -- the cross-correlation of the elements with the wanted signal.  The
    beam w^H s then has the largest ratio of signal to interference plus noise a linear combination of the elements can have."""
    R = np.asarray(R, dtype=np.complex128)
    K = R.shape[0]
    if R.shape != (K, K) or not MIN_ELEMENTS <= K <= MAX_ELEMENTS:
        raise ValueError("R is K x K, K in 2..8")
    if not loading >= 0.0:
        raise ValueError("loading is not negative")
    return np.linalg.solve(R + loading * (np.trace(R).real / K) * np.eye(K), as_weights(p, K))
