"""Pulse blanking and narrow-band excision between the down-converter's output and the ring, as NumPy: what the device
must leave in the ring when a mitigator is attached to a converter.

The device form is sydr_amd/csrc/mitigate.hip (sdr_ddc_mitigate in include/sydr_amd.h, Engine.ddc_mitigate); this file is its
only yardstick.  The input is the converter's v_m (complex128, downconvert.Statement.push), m = 0, 1, ... counted from creation
or reset across pushes, v_m = 0 for m < 0.

Blanker (blank_level > 0; blank_lead, blank_hold in 0..1024 samples):

    p_m = re*re + im*im                         (two products, one sum, each rounded; no FMA)
    t_m = p_m > blank_level * blank_level       (the square formed once)
    b_m = any t_j, m - blank_hold <= j <= m + blank_lead
    u_m = 0 where b_m, else v_m

Excisor (nfft = N, a power of two in 64..4096; limit[k], k < N in FFT order), hop H = N / 2, periodic Hann window
w[j] = 0.5 - 0.5 cos(2 pi j / N) (w[j] + w[j + H] = 1), segment s >= -1 = u[s H .. s H + N):

    A_s = FFT(w * u_s),  P = re^2 + im^2 of A_s[k],  G[k] = 0 where P > limit[k] else 1,  B_s = IFFT(G * A_s)
    y_m = B_{q-1}[m - (q-1) H] + B_q[m - q H],  q = floor(m / H)

(y = u without the excisor).  The delay is L = (N with the excisor) + blank_lead: output i of the stream is format(y_{i-L}) and
format(0) for i < L; a push of k values of v yields exactly k outputs.  Every segment's transform is a function of its N
inputs alone and the state is the last K values of v,

    K = 2 N - 1 + blank_lead + blank_hold   (blank_lead + blank_hold without the excisor)

(output i = n needs y_{n-L}, whose older segment begins at (floor((n-L)/H) - 1) H >= n - L - N + 1, whose first u needs v from
blank_hold earlier): what comes out does not depend on how the stream was cut into pushes, bit for bit.  The tail of a stream
comes out when the caller pushes L more zeros.

Counters, all functions of the number n of outputs delivered alone:

    n_outputs = n,  n_triggers = #{0 <= j < n - L : t_j},  n_blanked = #{0 <= m < n - L : b_m},
    n_segments = #{s >= -1 : s H + N <= n - L},  bins[k] = #{finished segments with G[k] = 0},  n_bins_excised = sum bins
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MIN_NFFT, MAX_NFFT, MAX_REACH = 64, 4096, 1024


@dataclass
class MitigationConfig:
    blank_level: float = 0.0          # an amplitude in v's units; 0 = no blanker
    blank_lead: int = 0
    blank_hold: int = 0
    nfft: int = 0                     # 0 = no excisor
    limit: np.ndarray | None = None   # [nfft] powers |A[k]|^2, FFT order; +inf allowed

    def __post_init__(self):
        self.blank_level, self.blank_lead, self.blank_hold = float(self.blank_level), int(self.blank_lead), int(self.blank_hold)
        self.nfft = int(self.nfft)
        if not self.blank_level >= 0.0:
            raise ValueError("blank_level is a non-negative amplitude")
        for name, reach in (("blank_lead", self.blank_lead), ("blank_hold", self.blank_hold)):
            if not 0 <= reach <= MAX_REACH:
                raise ValueError(f"{name} {reach} outside 0..{MAX_REACH}")
        if self.nfft:
            if not MIN_NFFT <= self.nfft <= MAX_NFFT or self.nfft & (self.nfft - 1):
                raise ValueError(f"nfft {self.nfft} is not a power of two in {MIN_NFFT}..{MAX_NFFT}")
            if self.limit is None:
                raise ValueError("an excisor needs its limits")
            self.limit = np.ascontiguousarray(self.limit, dtype=np.float64).reshape(-1)
            if self.limit.size != self.nfft:
                raise ValueError(f"{self.limit.size} limits for nfft {self.nfft}")
            if not np.all(self.limit >= 0.0):                      # (NaN fails the comparison too)
                raise ValueError("limits are non-negative powers")
        else:
            self.limit = None
        if not self.blanking and not self.nfft:
            raise ValueError("neither a blanker nor an excisor")

    @property
    def blanking(self) -> bool:
        return self.blank_level > 0.0

    @property
    def lead(self) -> int:
        return self.blank_lead if self.blanking else 0

    @property
    def hold(self) -> int:
        return self.blank_hold if self.blanking else 0

    @property
    def delay(self) -> int:
        """L, in ring samples (lead and hold count only with a blanker)."""
        return self.nfft + self.lead

    @property
    def state_length(self) -> int:
        """K: the values of v a push needs from before it."""
        return (2 * self.nfft - 1 if self.nfft else 0) + self.lead + self.hold


def hann(nfft: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nfft) / nfft)


@dataclass
class Stats:
    n_outputs: int
    n_triggers: int
    n_blanked: int
    n_segments: int
    n_bins_excised: int
    bins: np.ndarray

    def __eq__(self, other):
        return (self.n_outputs, self.n_triggers, self.n_blanked, self.n_segments, self.n_bins_excised) == \
            (other.n_outputs, other.n_triggers, other.n_blanked, other.n_segments, other.n_bins_excised) and \
            np.array_equal(self.bins, other.bins)


def segments_finished(n: int, delay: int, nfft: int) -> int:
    """#{s >= -1 : s H + N <= n - L}"""
    if not nfft:
        return 0
    H = nfft // 2
    return 0 if n - delay < H else (n - delay - nfft) // H + 2


class Statement:
    """The statement with its state: the last K values of v and the number of outputs delivered."""

    def __init__(self, cfg: MitigationConfig):
        self.cfg = cfg
        self._win = hann(cfg.nfft) if cfg.nfft else None
        self._level2 = cfg.blank_level * cfg.blank_level
        self.reset()

    def reset(self):
        self.n = 0
        self._state = np.zeros(self.cfg.state_length, dtype=np.complex128)
        self._triggers = self._blanked = 0
        self._bins = np.zeros(self.cfg.nfft, dtype=np.int64)

    @property
    def delay(self) -> int:
        return self.cfg.delay

    @property
    def stats(self) -> Stats:
        return Stats(self.n, self._triggers, self._blanked, segments_finished(self.n, self.cfg.delay, self.cfg.nfft),
                     int(self._bins.sum()), self._bins.copy())

    def _segment(self, u: np.ndarray):
        """-> (B, G == 0) of one segment: a function of its N inputs alone (one 1-D transform each way)."""
        a = np.empty(u.size, dtype=np.complex128)
        a.real, a.imag = self._win * u.real, self._win * u.imag
        A = np.fft.fft(a)
        cut = A.real * A.real + A.imag * A.imag > self.cfg.limit
        A[cut] = 0.0
        return np.fft.ifft(A), cut

    def push(self, v) -> np.ndarray:
        """`v`: the converter's outputs of a push (complex128).  Returns as many outputs of the stream: y_{i-L}, 0 for i < L."""
        cfg = self.cfg
        N, H, lead, hold, K, L = cfg.nfft, cfg.nfft // 2, cfg.lead, cfg.hold, cfg.state_length, cfg.delay
        v = np.asarray(v, dtype=np.complex128).reshape(-1)
        k, n = v.size, self.n
        if k == 0:
            return np.zeros(0, dtype=np.complex128)
        W = np.concatenate([self._state, v])                 # W[x] = v_{n - K + x}
        j_lo, n_u = n - K + hold, K + k - hold - lead        # U[x] = u_{j_lo + x}
        lo, hi = max(0, n - L) - j_lo, n + k - L - j_lo      # the u that this push delivers (counted once, here)
        if cfg.blanking:
            re, im = W.real, W.imag
            t = re * re + im * im > self._level2
            c = np.concatenate([[0], np.cumsum(t)])
            x = np.arange(n_u)
            b = c[x + hold + lead + 1] - c[x] > 0
            U = np.where(b, 0.0, W[hold:hold + n_u])
            if hi > lo:
                self._triggers += int(np.count_nonzero(t[hold + lo:hold + hi]))
                self._blanked += int(np.count_nonzero(b[lo:hi]))
        else:
            U = W
        m = n - L + np.arange(k)
        if N:
            s_lo, s_hi = (n - L) // H - 1, (n + k - 1 - L) // H
            B = np.zeros((s_hi - s_lo + 1, N), dtype=np.complex128)
            for s in range(max(s_lo, -1), s_hi + 1):         # (segments before -1 hold zeros and feed only m < 0)
                at = s * H - j_lo
                B[s - s_lo], cut = self._segment(U[at:at + N])
                if n - L < s * H + N <= n + k - L:           # finishes in this push
                    self._bins += cut
            q = m // H
            y = B[q - 1 - s_lo, m - (q - 1) * H] + B[q - s_lo, m - q * H]
        else:
            y = U[:k].copy()
        y[m < 0] = 0.0
        self._state = W[k:].copy()
        self.n = n + k
        return y


def statement(cfg: MitigationConfig, pushes, state: Statement | None = None) -> np.ndarray:
    """The outputs of a list of pushes (arrays of v), concatenated."""
    st = state if state is not None else Statement(cfg)
    parts = [st.push(v) for v in pushes]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.complex128)


def tolerance(cfg: MitigationConfig, max_abs_v: float) -> float:
    """B_mit = 16 log2(N) N 2^-53 max|u| per component: what two implementations of the segment's two transforms may differ
    by (each transform of log2 N butterfly stages is off by at most 4 log2(N) 2^-53 N max|u|).  0 without the excisor: the
    blanker passes or zeroes v."""
    if not cfg.nfft:
        return 0.0
    return 16.0 * np.log2(cfg.nfft) * cfg.nfft * 2.0 ** -53 * float(max_abs_v)


def ambiguous_gates(cfg: MitigationConfig, v, bin_band: float = 1e-9, level_band: float = 1e-12):
    """Where two computations of the gates may differ on the stream v (one push from reset): -> (bins whose |A_s[k]|^2 lies
    within a relative bin_band of its limit, samples whose p_m lies within a relative level_band of the squared level,
    the smallest relative bin margin, the smallest relative level margin)."""
    st = Statement(cfg)
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    near_level, level_margin = 0, np.inf
    u = v
    if cfg.blanking:
        p = v.real * v.real + v.imag * v.imag
        rel = np.abs(p - st._level2) / st._level2
        near_level, level_margin = int(np.count_nonzero(rel <= level_band)), float(rel.min()) if rel.size else np.inf
        u = statement(MitigationConfig(cfg.blank_level, cfg.blank_lead, cfg.blank_hold), [np.concatenate([v, np.zeros(cfg.lead)])])[cfg.lead:]
    near_bin, bin_margin = 0, np.inf
    if cfg.nfft:
        N, H = cfg.nfft, cfg.nfft // 2
        pad = np.concatenate([np.zeros(H, dtype=np.complex128), u])
        finite = np.isfinite(cfg.limit) & (cfg.limit > 0.0)
        for at in range(0, pad.size - N + 1, H):
            seg = pad[at:at + N]
            a = np.empty(N, dtype=np.complex128)
            a.real, a.imag = st._win * seg.real, st._win * seg.imag
            A = np.fft.fft(a)
            P = A.real * A.real + A.imag * A.imag
            rel = np.abs(P[finite] - cfg.limit[finite]) / cfg.limit[finite]
            if rel.size:
                near_bin += int(np.count_nonzero(rel <= bin_band))
                bin_margin = min(bin_margin, float(rel.min()))
            near_bin += int(np.count_nonzero((cfg.limit == 0.0) & (P <= bin_band)))
    return near_bin, near_level, bin_margin, level_margin


def excision_limits(v, nfft: int, margin_db: float = 10.0) -> np.ndarray:
    """10^(margin_db / 10) times the median over k of the mean over the whole segments of v of |FFT(w v_s)[k]|^2, the same
    value for every bin: the median bin is the noise floor's whatever narrow-band interferer stands in a few others."""
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    nfft = int(nfft)
    H = nfft // 2
    n_seg = 0 if v.size < nfft else (v.size - nfft) // H + 1
    if n_seg < 1:
        raise ValueError(f"{v.size} samples hold no segment of {nfft}")
    w, acc = hann(nfft), np.zeros(nfft)
    for s in range(n_seg):
        A = np.fft.fft(w * v[s * H:s * H + nfft])
        acc += A.real * A.real + A.imag * A.imag
    return np.full(nfft, 10.0 ** (margin_db / 10.0) * float(np.median(acc / n_seg)))


def blanking_level(v, factor: float) -> float:
    """factor * sqrt(median(|v|^2) / ln 2): |v|^2 of complex Gaussian noise is exponential, its median ln 2 times its mean --
    factor times the noise's RMS amplitude, estimated where pulses cannot reach."""
    v = np.asarray(v, dtype=np.complex128).reshape(-1)
    return float(factor) * float(np.sqrt(np.median(v.real * v.real + v.imag * v.imag) / np.log(2.0)))
