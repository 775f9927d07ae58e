"""Space-time adaptive weights (STAP) in the array down-converter, as NumPy: what the device must leave in the ring, and in the
lag covariance.

`array.py` combines the K elements of a frame with one weight each: at most K - 1 nulls, each the same at every frequency.
Here every element has a short FIR, K x T weights: the time taps give nulls that depend on frequency, so two elements remove
several partial-band jammers from different directions, and they absorb the elements' differing channel responses.  The device
form is sydr_amd/csrc/ddc_stap.h (the combine and the raw tail, in ddc_kernel / resample_kernel) and ddc_stap.hip (the lag
covariance); sdr_ddc_create_stap in include/sydr_amd.h, Engine.ddc_create with a `SpaceTimeGeometry` as `cfg.array`.  This file
is its only yardstick.

A SPACE-TIME ARRAY is an array (layout, K lanes, as `array.ArrayGeometry`) plus T taps, T in 1..8.  Weights are
w[t][a] = wr + i wi, t = 0..T-1, a = 0..K-1, finite doubles.  s_a[i] is element a of frame i, decoded exactly as the array
converter decodes it (`array.elements`), and 0 before the first input since creation or reset.  The converter's input is

    x_j = sum_t sum_a conj(w[t][a]) s_a[j - t]

formed in fp64 with one running pair that starts at +0.0, t ascending and inside each t a ascending, the array converter's four
operations per (t, a), every product rounded, every sum rounded, no contraction (`combine`):

    re = 0.0; im = 0.0
    for t = 0 .. T-1:
        for a = 0 .. K-1:                       (sr, si) = s_a[j - t]
            re = re + wr*sr;  re = re + wi*si
            im = im + wr*si;  im = im - wi*sr

From x_j on everything is `downconvert.Statement`, as `array.Statement` already is.  Weights belong to input indices: a change
(`Statement.set_weights`) takes effect with the first input of the next push, for all T taps of that input; earlier x_j, those
in the filter's history included, keep their values, and the raw elements of the last T - 1 frames are carried across pushes.
With the changes at the same input indices the ring does not depend on how the stream was cut into pushes, bit for bit.

Lag covariance (opt-in, `measure`; SDR_DDC_ARRAY_MEASURE).  For tau = 0..T-1, over the inputs j pushed since creation, reset or
the last clearing read, n their number:

    C[tau][a][b] = sum_j s_a[j] conj(s_b[j - tau]):   re = sum(sr_a sr_b' + si_a si_b')   im = sum(si_a sr_b' - sr_a si_b')

with (sr_b', si_b') = s_b[j - tau], the real earlier input when one has been pushed since creation or reset -- before a
clearing read too -- and zero otherwise.  For INT8, INT16 and PACKED fields the sums are exact int64 integers, each converted to
double once at the read: device and statement are equal.  For FLOAT32 fields the device adds in fp64 in an order of its own and
may differ by at most 2 n 2^-52 sum_j (|sr_a sr_b'| + |si_a si_b'|) per component (`lag_covariance_bound`: `array.py`'s
derivation, n terms of two products in any order, applied per lag), correspondingly for the imaginary part.

Weight rules (host only; K T <= 64, numpy.linalg.solve -- the C-ABI takes weights and does not solve for them).  The stacked
vector of input j is y_j[t K + a] = s_a[j - t]; `space_time_covariance` builds its K T x K T covariance R = E[y y^H] from the
lags, block-Toeplitz: the entry at ((t, a), (u, b)) is C[u - t][a][b] / n for u >= t and conj(C[t - u][b][a]) / n otherwise.
With Rl = R + loading * trace(R)/(K T) * I -- `array.py`'s loading rule on the larger matrix --

    power_inversion:  w = Rl^-1 e / (e^H Rl^-1 e),   e = 1 at (reference_tap, reference)      (reference_tap = (T - 1) // 2)
    mvdr:             w = Rl^-1 c / (c^H Rl^-1 c),   c = the steering vector at reference_tap, zero elsewhere

The output is then the reference element (the steered beam) delayed by reference_tap input samples; sdr_ddc_delay does not know
of it, the host layer adds it.

BEAMS (sdr_ddc_beam_attach): as in `array.py` -- beam b's ring is `statement` of the same configuration with the weights w_b
[T][K]; `beams_statement` is that, once per weight set.  The raw tail holds elements and is the same for every beam.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import array as ar
from . import downconvert as dc

MIN_TAPS, MAX_TAPS = 1, 8
DEFAULT_LOADING = ar.DEFAULT_LOADING


def default_reference_tap(T: int) -> int:
    return (int(T) - 1) // 2


def as_weights(w, T: int, K: int) -> np.ndarray:
    """T x K finite complex weights, read-only complex128 [T][K]; `w` complex [T][K] (or flat) or real [T][K][2]."""
    w = np.asarray(w)
    if w.ndim == 3 and w.shape == (T, K, 2) and not np.iscomplexobj(w):
        w = w[..., 0] + 1j * w[..., 1]
    w = np.array(w, dtype=np.complex128)
    if w.size != T * K:
        raise ValueError(f"{w.size} weights for {T} taps of {K} elements")
    w = w.reshape(T, K)
    if not np.all(np.isfinite(w.real) & np.isfinite(w.imag)):
        raise ValueError("weights must be finite")
    w.setflags(write=False)
    return w


def unit_weights(T: int, K: int, a: int, t0: int = 0) -> np.ndarray:
    """1 at element a of tap t0, 0 elsewhere."""
    if not (0 <= a < K and 0 <= t0 < T):
        raise ValueError(f"element {a} of tap {t0} outside {K} elements of {T} taps")
    w = np.zeros((T, K), dtype=np.complex128)
    w[t0, a] = 1.0
    return w


class SpaceTimeGeometry(ar.ArrayGeometry):
    """An `array.ArrayGeometry` with `taps` weights per element (sdr_ddc_create_stap): `weights` is [T][K]."""

    def __init__(self, lanes, taps: int = 1, weights=None, measure: bool = False):
        self.taps = int(taps)
        if not MIN_TAPS <= self.taps <= MAX_TAPS:
            raise ValueError(f"{self.taps} taps outside {MIN_TAPS}..{MAX_TAPS}")
        K = len(tuple(lanes))
        if weights is None and ar.MIN_ELEMENTS <= K <= ar.MAX_ELEMENTS:
            weights = unit_weights(self.taps, K, 0, 0)
        super().__init__(lanes, weights, measure)

    @property
    def weights(self) -> np.ndarray:
        return self._weights

    @weights.setter
    def weights(self, w):
        self._weights = as_weights(w, self.taps, len(self.lanes))

    def __eq__(self, other):
        return (isinstance(other, SpaceTimeGeometry) and self.lanes == other.lanes and self.taps == other.taps and
                self.measure == other.measure and np.array_equal(self.weights, other.weights))

    def __hash__(self):
        return hash((self.lanes, self.taps, self.measure, self.weights.tobytes()))

    def __repr__(self):
        return f"SpaceTimeGeometry(lanes={self.lanes}, taps={self.taps}, weights={self.weights.tolist()}, measure={self.measure})"


def combine(sr: np.ndarray, si: np.ndarray, weights, T: int):
    """x_j for j = T - 1 .. of the elements sr, si [K][T - 1 + n] (the first T - 1 columns the frames before the push), in the
    statement's order -> (re, im), float64 [n] each.  Every line is one IEEE operation per element of the arrays."""
    K, n = sr.shape[0], sr.shape[1] - (T - 1)
    w = as_weights(weights, T, K)
    re, im = np.zeros(n), np.zeros(n)
    for t in range(T):
        lo = T - 1 - t
        for a in range(K):
            wr, wi = float(w[t, a].real), float(w[t, a].imag)
            r, i = sr[a, lo:lo + n], si[a, lo:lo + n]
            re = re + wr * r
            re = re + wi * i
            im = im + wr * i
            im = im - wi * r
    return re, im


def lag_covariance(sr: np.ndarray, si: np.ndarray, T: int, integer: bool):
    """C [T][K][K] complex128 of the elements sr, si [K][T - 1 + n], j over the last n columns: int64 sums converted once for
    integer fields, fp64 sums in NumPy's order otherwise."""
    K, n = sr.shape[0], sr.shape[1] - (T - 1)
    C = np.zeros((T, K, K), dtype=np.complex128)
    if integer:
        sr, si = sr.astype(np.int64), si.astype(np.int64)
    for tau in range(T):
        ar_, ai_ = sr[:, T - 1:], si[:, T - 1:]
        br, bi = sr[:, T - 1 - tau:T - 1 - tau + n], si[:, T - 1 - tau:T - 1 - tau + n]
        if integer:
            re, im = ar_ @ br.T + ai_ @ bi.T, ai_ @ br.T - ar_ @ bi.T            # (int64 throughout: exact)
        else:
            re = np.array([[np.sum(ar_[a] * br[b] + ai_[a] * bi[b]) for b in range(K)] for a in range(K)])
            im = np.array([[np.sum(ai_[a] * br[b] - ar_[a] * bi[b]) for b in range(K)] for a in range(K)])
        C[tau] = re.astype(np.float64) + 1j * im.astype(np.float64)
    return C


def lag_covariance_bound(sr: np.ndarray, si: np.ndarray, T: int):
    """What a component of a float32 array's C may differ by between two orders of fp64 addition: (for re, for im), [T][K][K]
    each -- 2 n 2^-52 sum_j (|sr_a sr_b'| + |si_a si_b'|) and 2 n 2^-52 sum_j (|si_a sr_b'| + |sr_a si_b'|)."""
    K, n = sr.shape[0], sr.shape[1] - (T - 1)
    scale = 2.0 * n * 2.0 ** -52
    re, im = np.zeros((T, K, K)), np.zeros((T, K, K))
    for tau in range(T):
        ar_, ai_ = np.abs(sr[:, T - 1:]), np.abs(si[:, T - 1:])
        br, bi = np.abs(sr[:, T - 1 - tau:T - 1 - tau + n]), np.abs(si[:, T - 1 - tau:T - 1 - tau + n])
        re[tau], im[tau] = scale * (ar_ @ br.T + ai_ @ bi.T), scale * (ai_ @ br.T + ar_ @ bi.T)
    return re, im


def space_time_covariance(C, n) -> np.ndarray:
    """The K T x K T block-Toeplitz covariance of the stacked vector y[t K + a] = s_a[j - t] from the lags C [T][K][K] of n
    inputs: C[u - t][a][b] / n at ((t, a), (u, b)) for u >= t, conj(C[t - u][b][a]) / n otherwise."""
    C = np.asarray(C, dtype=np.complex128)
    if C.ndim != 3 or C.shape[1] != C.shape[2] or not MIN_TAPS <= C.shape[0] <= MAX_TAPS:
        raise ValueError("C is T x K x K, T in 1..8")
    if not n > 0:
        raise ValueError("the covariance holds no input")
    T, K = C.shape[0], C.shape[1]
    R = np.empty((T * K, T * K), dtype=np.complex128)
    for t in range(T):
        for u in range(T):
            R[t * K:(t + 1) * K, u * K:(u + 1) * K] = C[u - t] if u >= t else C[t - u].conj().T
    return R / float(n)


def _loaded(C, n, loading: float) -> np.ndarray:
    if not loading >= 0.0:
        raise ValueError("loading is not negative")
    R = space_time_covariance(C, n)
    return R + loading * (np.trace(R).real / R.shape[0]) * np.eye(R.shape[0])


def _reference_tap(T: int, reference_tap) -> int:
    t0 = default_reference_tap(T) if reference_tap is None else int(reference_tap)
    if not 0 <= t0 < T:
        raise ValueError(f"reference tap {t0} outside 0..{T - 1}")
    return t0


def power_inversion(C, n, reference: int = 0, reference_tap=None, loading: float = DEFAULT_LOADING) -> np.ndarray:
    """w [T][K] = Rl^-1 e / (e^H Rl^-1 e), e = 1 at (reference_tap, reference): the reference element passes with unit weight,
    delayed by reference_tap inputs, and the output power is least."""
    C = np.asarray(C)
    T, K = C.shape[0], C.shape[1]
    Rl = _loaded(C, n, loading)
    e = unit_weights(T, K, int(reference), _reference_tap(T, reference_tap)).reshape(-1)
    return ar.mvdr_loaded(Rl, e).reshape(T, K)


def mvdr(C, n, steering, reference_tap=None, loading: float = DEFAULT_LOADING) -> np.ndarray:
    """w [T][K] = Rl^-1 c / (c^H Rl^-1 c), c the steering vector at reference_tap and zero elsewhere."""
    C = np.asarray(C)
    T, K = C.shape[0], C.shape[1]
    Rl = _loaded(C, n, loading)
    c = np.zeros((T, K), dtype=np.complex128)
    c[_reference_tap(T, reference_tap)] = ar.as_weights(steering, K)
    return ar.mvdr_loaded(Rl, c.reshape(-1)).reshape(T, K)


class Statement(ar.Statement):
    """`array.Statement` with T taps per element: the combined inputs come from the push's frames and the raw tail of the
    T - 1 frames before it; the covariance is the lag covariance C [T][K][K]."""

    def __init__(self, cfg: dc.DownConverterConfig):
        if not isinstance(cfg.array, SpaceTimeGeometry):
            raise ValueError("a space-time statement needs a SpaceTimeGeometry")
        self.taps = cfg.array.taps
        super().__init__(cfg)
        self.weights = cfg.array.weights

    def reset(self):
        """Both histories and the covariance zero, j = 0; the weights stay."""
        dc.Statement.reset(self)
        K, T = self.cfg.array.n_elements, self.cfg.array.taps
        self.tail_r, self.tail_i = np.zeros((K, T - 1)), np.zeros((K, T - 1))
        self.C, self.n = np.zeros((T, K, K), dtype=np.complex128), 0

    def set_weights(self, weights):
        """From the first input of the next push on, for all T taps of that input."""
        self.weights = as_weights(weights, self.taps, self.cfg.array.n_elements)

    def read_covariance(self, clear: bool = False):
        C, n = self.C.copy(), self.n
        if clear:
            self.C, self.n = np.zeros_like(self.C), 0
        return C, n

    def _with_tail(self, raw):
        sr, si = ar.elements(raw, self.cfg.layout, self.cfg.array.lanes)
        return np.concatenate([self.tail_r, sr], axis=1), np.concatenate([self.tail_i, si], axis=1)

    def combined(self, raw):
        sr, si = self._with_tail(raw)
        return combine(sr, si, self.weights, self.taps)

    def push(self, raw) -> np.ndarray:
        raw = np.ascontiguousarray(raw).reshape(-1)
        T = self.taps
        sr, si = self._with_tail(raw)
        re, im = combine(sr, si, self.weights, T)
        if self.cfg.array.measure:
            # (integer fields: sums of integers below 2^53 stay exact in this addition as well)
            self.C = self.C + lag_covariance(sr, si, T, self.cfg.layout.field != dc.FIELD_FLOAT32)
            self.n += sr.shape[1] - (T - 1)
        self.tail_r, self.tail_i = sr[:, sr.shape[1] - (T - 1):].copy(), si[:, si.shape[1] - (T - 1):].copy()
        return self._push_inputs(re, im)


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
    """`cfg` with its space-time weights replaced: the configuration of the independent converter a beam is defined by."""
    return dataclasses.replace(cfg, array=SpaceTimeGeometry(cfg.array.lanes, cfg.array.taps, weights, cfg.array.measure))


def beams_statement(cfg: dc.DownConverterConfig, weight_sets, pushes, ring_fmts=None, weights_at=None):
    """`array.beams_statement` with this file's `statement`: one list entry per weight set [T][K], beam 0 first."""
    return ar.beams_statement(cfg, weight_sets, pushes, ring_fmts, weights_at, _statement=statement, _with=with_weights)


def element_weights(T: int, K: int, t0: int = 0) -> np.ndarray:
    """The K unit vectors at tap t0, [K][T][K]: beam a of them is element a's own stream, delayed by t0 inputs."""
    return np.stack([unit_weights(T, K, a, t0) for a in range(K)])


def wiener_weights(C, n, p, reference_tap=None, loading: float = DEFAULT_LOADING) -> np.ndarray:
    """w [T][K] = Rl^-1 c, Rl the loaded space-time covariance of the lags C of n inputs and c the per-element prompts p of a
    tracked signal at reference_tap, zero elsewhere (`array.wiener_weights` on the stacked vector)."""
    C = np.asarray(C)
    T, K = C.shape[0], C.shape[1]
    c = np.zeros((T, K), dtype=np.complex128)
    c[_reference_tap(T, reference_tap)] = ar.as_weights(p, K)
    return np.linalg.solve(_loaded(C, n, loading), c.reshape(-1)).reshape(T, K)
