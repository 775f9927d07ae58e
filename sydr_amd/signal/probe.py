"""What a window of I,Q samples holds -- level statistics, a histogram per component, a Welch power spectral density: the
statement of `sdr_iq_probe` (include/sydr_amd.h) in NumPy, and `ProbeResult`, what either of them returns.

`probe(raw)` is what the engine's call (`Engine.iq_probe`, on the device, over the ring) is tested against; it is also the
way to look at samples that are on the host anyway.  The raw fields are the C struct's; the properties are what people read
off them: mean and RMS per component, the DC offset relative to the RMS, the I/Q gain imbalance, the I/Q correlation
coefficient, the fraction of components on the rails, the spectrum in dB and the bins that stand out of it.
"""
from __future__ import annotations

import numpy as np

HIST_BINS = 256
NFFT_MIN, NFFT_MAX = 64, 4096
_RAILS = {np.dtype(np.int8): (-128, 127), np.dtype(np.int16): (-32768, 32767)}


class ProbeResult:
    """Raw fields (sdr_probe_result): n_samples, n_segments, n_nonfinite, n_rail[2], min[2], max[2], sum[2], sum_sq[2],
    sum_iq; hist (int64[2, 256] or None), psd (float64[nfft] in FFT order, or None), fs (of the psd, or None)."""

    FIELDS = ("n_samples", "n_segments", "n_nonfinite", "n_rail", "min", "max", "sum", "sum_sq", "sum_iq")

    def __init__(self, n_samples, n_segments, n_nonfinite, n_rail, min, max, sum, sum_sq, sum_iq, hist=None, psd=None, fs=None):
        self.n_samples, self.n_segments, self.n_nonfinite = int(n_samples), int(n_segments), int(n_nonfinite)
        self.n_rail = (int(n_rail[0]), int(n_rail[1]))
        self.min, self.max = (float(min[0]), float(min[1])), (float(max[0]), float(max[1]))
        self.sum, self.sum_sq = (float(sum[0]), float(sum[1])), (float(sum_sq[0]), float(sum_sq[1]))
        self.sum_iq = float(sum_iq)
        self.hist, self.psd, self.fs = hist, psd, fs

    def raw(self) -> dict:
        """The C struct's fields as plain data (what two results are compared by)."""
        return {name: getattr(self, name) for name in self.FIELDS}

    def __repr__(self):
        return "ProbeResult(" + ", ".join(f"{k}={v}" for k, v in self.raw().items()) + ")"

    # ------------------------------------------------------------------ read off the moments
    @property
    def n_finite(self) -> int:
        return self.n_samples - self.n_nonfinite

    @property
    def mean(self):
        n = self.n_finite
        return tuple(s / n if n else float("nan") for s in self.sum)

    @property
    def rms(self):
        n = self.n_finite
        return tuple(float(np.sqrt(q / n)) if n else float("nan") for q in self.sum_sq)

    @property
    def dc_offset(self):
        """Mean over RMS, per component (0 = none; +-1 = nothing but an offset)."""
        return tuple(m / r if r > 0 else float("nan") for m, r in zip(self.mean, self.rms))

    @property
    def iq_imbalance_db(self) -> float:
        """Gain of I over Q: 20 * log10(rms I / rms Q)."""
        qi, qq = self.sum_sq
        return float(10.0 * np.log10(qi / qq)) if qi > 0 and qq > 0 else float("nan")

    @property
    def iq_correlation(self) -> float:
        """Correlation coefficient of I and Q (0 for a clean quadrature front end)."""
        n = self.n_finite
        if not n:
            return float("nan")
        mi, mq = self.mean
        vi, vq = self.sum_sq[0] / n - mi * mi, self.sum_sq[1] / n - mq * mq
        return float((self.sum_iq / n - mi * mq) / np.sqrt(vi * vq)) if vi > 0 and vq > 0 else float("nan")

    @property
    def rail_fraction(self):
        """Fraction of the components at the type's minimum or maximum (integer samples), per component."""
        return tuple(r / self.n_samples for r in self.n_rail)

    # ------------------------------------------------------------------ read off the spectrum
    def frequencies(self, fs=None) -> np.ndarray:
        """Frequency of every psd bin [Hz], FFT order: k*fs/nfft below nfft/2, (k - nfft)*fs/nfft from there on."""
        fs = self.fs if fs is None else fs
        if self.psd is None or fs is None:
            raise ValueError("no spectrum in this result (probe with nfft and fs)")
        nfft = len(self.psd)
        k = np.arange(nfft)
        return np.where(k < nfft // 2, k, k - nfft) * float(fs) / nfft

    @property
    def psd_db(self) -> np.ndarray:
        if self.psd is None:
            raise ValueError("no spectrum in this result (probe with nfft and fs)")
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(self.psd)

    def spurs(self, threshold_db: float = 10.0, fs=None):
        """The bins more than `threshold_db` above the median bin: [(frequency [Hz], dB over the median), ...], strongest
        first -- a carrier-wave interferer shows as one or two bins tens of dB above a flat floor."""
        db = self.psd_db
        over = db - np.median(db)
        f = self.frequencies(fs)
        idx = np.flatnonzero(over > threshold_db)
        idx = idx[np.argsort(-over[idx], kind="stable")]
        return [(float(f[k]), float(over[k])) for k in idx]


def hann_periodic(nfft: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)


def segments(n_samples: int, nfft: int) -> int:
    """Welch segments of nfft samples, hop nfft // 2, inside n_samples."""
    return (n_samples - nfft) // (nfft // 2) + 1 if n_samples >= nfft else 0


def welch(x: np.ndarray, nfft: int, fs: float) -> np.ndarray:
    """psd[k] = sum_s |FFT(w * x_s)[k]|^2 / (S * fs * sum w^2): two-sided, FFT order, periodic Hann, hop nfft // 2, no
    detrending.  All NaN when a used segment holds a non-finite sample."""
    nfft = int(nfft)
    if nfft < NFFT_MIN or nfft > NFFT_MAX or nfft & (nfft - 1):
        raise ValueError(f"nfft {nfft} is not a power of two in {NFFT_MIN}..{NFFT_MAX}")
    if not (fs is not None and np.isfinite(fs) and fs > 0):
        raise ValueError("a spectrum needs a positive sampling frequency")
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    S, hop = segments(x.size, nfft), nfft // 2
    if S < 1:
        raise ValueError(f"{x.size} samples hold no segment of {nfft}")
    used = x[:(S - 1) * hop + nfft]
    if not (np.isfinite(used.real).all() and np.isfinite(used.imag).all()):
        return np.full(nfft, np.nan)
    w = hann_periodic(nfft)
    acc = np.zeros(nfft)
    view = np.lib.stride_tricks.as_strided(used, (S, nfft), (hop * used.itemsize, used.itemsize), writeable=False)
    for s0 in range(0, S, 4096):                       # (segment after segment, a few thousand at a time)
        X = np.fft.fft(view[s0:s0 + 4096] * w, axis=1)
        acc += (X.real * X.real + X.imag * X.imag).sum(axis=0)
    return acc / (S * float(fs) * float((w * w).sum()))


def probe(raw_interleaved, hist_shift: int = 0, nfft: int = 0, fs=None) -> ProbeResult:
    """`raw_interleaved`: [I0, Q0, I1, Q1, ...] as int8, int16, float32 or float64 (complex arrays are taken as float64
    pairs).  Integer samples: exact sums, rails and a histogram with bin min(255, max(0, (v >> hist_shift) + 128)); float
    samples: those with a NaN / Inf component are counted and left out, no histogram.  nfft > 0: the Welch spectrum too."""
    raw = np.asarray(raw_interleaved)
    if np.iscomplexobj(raw):
        raw = np.ascontiguousarray(raw, dtype=np.complex128).view(np.float64)
    raw = raw.reshape(-1)
    if raw.size < 2 or raw.size % 2:
        raise ValueError("interleaved IQ needs an even, positive number of elements")
    n = raw.size // 2
    comp = (raw[0::2], raw[1::2])
    hist = psd = None
    if raw.dtype in _RAILS:
        lo, hi = _RAILS[raw.dtype]
        if hist_shift < 0 or hist_shift > (0 if raw.dtype == np.int8 else 8):
            raise ValueError(f"hist_shift {hist_shift} does not fit {raw.dtype} samples")
        wide = [c.astype(np.int64) for c in comp]
        sums = [int(c.sum()) for c in wide]
        sq = [int((c * c).sum()) for c in wide]
        iq = int((wide[0] * wide[1]).sum())
        n_rail = [int(np.count_nonzero((c == lo) | (c == hi))) for c in wide]
        hist = np.stack([np.bincount(np.clip((c >> hist_shift) + 128, 0, 255), minlength=HIST_BINS) for c in wide]).astype(np.int64)
        res = ProbeResult(n, 0, 0, n_rail, [float(c.min()) for c in wide], [float(c.max()) for c in wide],
                          [float(v) for v in sums], [float(v) for v in sq], float(iq), hist=hist)
        x = None
    elif raw.dtype in (np.dtype(np.float32), np.dtype(np.float64)):
        i64, q64 = comp[0].astype(np.float64), comp[1].astype(np.float64)
        ok = np.isfinite(i64) & np.isfinite(q64)
        fi, fq = i64[ok], q64[ok]
        nan = float("nan")
        res = ProbeResult(n, 0, n - int(ok.sum()), (0, 0),
                          [float(fi.min()) if fi.size else nan, float(fq.min()) if fq.size else nan],
                          [float(fi.max()) if fi.size else nan, float(fq.max()) if fq.size else nan],
                          [float(fi.sum()), float(fq.sum())], [float((fi * fi).sum()), float((fq * fq).sum())], float((fi * fq).sum()))
        x = np.empty(n, dtype=np.complex128)
        x.real, x.imag = i64, q64
    else:
        raise ValueError(f"samples are int8, int16, float32 or float64, not {raw.dtype}")
    if nfft:
        if x is None:
            x = np.empty(n, dtype=np.complex128)
            x.real, x.imag = comp[0], comp[1]
        res.psd = welch(x, nfft, fs)
        res.fs = float(fs)
        res.n_segments = segments(n, int(nfft))
    return res


__all__ = ["HIST_BINS", "ProbeResult", "hann_periodic", "probe", "segments", "welch"]
