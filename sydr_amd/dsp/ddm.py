"""A delay-Doppler map around a known code phase and carrier: the statement of `sdr_ddm` (include/sydr_amd.h) in NumPy,
and its function-level entry.

A receiver that already has a code phase and a carrier -- from a channel that lost its signal a moment ago, from another
channel, an earlier track or an almanac -- searches a few chips and a few hundred hertz around them instead of the whole
code period and every Doppler bin.  The same map verifies that a tracking channel sits on the main peak, and is the data
product of reflectometry.

`ddm_statement` is the definition the device is held against (`Engine.ddm`, tests/test_gpu_ddm.py).  An item is an
`sdr_epl_item` read as a prediction: start_sample = s0, n_samples = W (the whole window), carrier_hz = f0, and
rem_carrier, rem_code, code_step = the NCO state at s0.  With B blocks of S segments, Q = B*S, T taps:

    a_q, b_q   = (q*W)//Q, ((q+1)*W)//Q                                  segment q covers window samples [a_q, b_q)
    s_j        = first_chips + j*step_chips
    z[q][j]    = EPL(ring[s0+a_q .. s0+b_q-1], f0, rem_carrier_q, rem_code_q, code_step, [s_j])      (tracking.py:92-116)
    rem_carrier_q = (rem_carrier + (-(f0*2.0*pi*a_q/fs))) % (2*pi)
    rem_code_q    = rem_code + a_q*code_step
    tau_q      = (a_q + b_q - 1) / 2.0 / fs
    d_k        = (k - (K-1)//2) * step_hz,   K = 2*floor(span_hz/step_hz) + 1
    Z[b][k][j] = sum_{s<S} z[b*S+s][j] * exp(-2j*pi*d_k*tau_{b*S+s})
    map[k][j]  = sum_{b<B} |Z[b][k][j]|^2

The peak is the first maximum of the map in row-major (k, j) order; the true code phase at s0 is rem_code + s_peak, the
true carrier f0 + d_peak.  second_value and noise_mean are the maximum and the mean of the entries whose tap lies a chip
or more from the peak's (any k), 0.0 when there is none.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .._lib import SDR_CORR_MAX_TAPS

MAX_SEGMENTS, MAX_ALL_SEGMENTS, MAX_BINS = 64, 4096, 4096

# result: dict(peak_bin, peak_tap, peak_hz, peak_chips, peak_value, second_value, noise_mean); map: float64[K][T];
# z: complex128[Q][T]; tau: float64[Q]
DdmResult = namedtuple("DdmResult", "result map z tau")


def ddm_bins(span_hz, step_hz):
    """K = 2*floor(span_hz/step_hz) + 1; 0 for a bad grid (sdr_ddm_bins)."""
    if not (step_hz > 0.0) or not (span_hz >= 0.0) or not np.isfinite(span_hz) or not np.isfinite(step_hz):
        return 0
    half = np.floor(span_hz / step_hz)
    return 2 * int(half) + 1 if half < 1e9 else 0


def _epl_tap(x, code, fs, carrier_hz, rem_carrier, rem_code, code_step, spacing):
    """One tap of the reference's EPL on samples x, the chips indexed modulo the code length (padded index p = chip
    (p - 1) mod L for any p)."""
    n = len(x)
    t = np.arange(0.0, n) / fs
    mixed = np.exp(1j * (-(carrier_hz * 2.0 * np.pi * t) + rem_carrier)) * x
    shift = rem_code + spacing
    idx = np.ceil(np.linspace(shift, code_step * n + shift, n, endpoint=False)).astype(np.int64)
    chips = code[(idx - 1) % len(code)]
    return np.sum(chips * mixed.real) + 1j * np.sum(chips * mixed.imag)


def ddm_statement(ring, code, fs, item, n_blocks, n_segments, first_chips, step_chips, n_taps, span_hz, step_hz):
    """ring: complex128[capacity], the ring's samples (widened), indexed modulo its length; code: the +-1 chips staged in
    the item's slot; item: (start_sample, n_samples, carrier_hz, rem_carrier, rem_code, code_step).
    -> DdmResult.  ValueError for what the call refuses."""
    ring = np.asarray(ring, dtype=np.complex128)
    code = np.asarray(code, dtype=np.float64)
    s0, W, f0, rem_carrier, rem_code, code_step = item
    s0, W, B, S, T = int(s0), int(W), int(n_blocks), int(n_segments), int(n_taps)
    K = ddm_bins(span_hz, step_hz)
    if not 1 <= T <= SDR_CORR_MAX_TAPS or K <= 0 or B < 1 or not 1 <= S <= MAX_SEGMENTS or (S == 1 and K > 1):
        raise ValueError("bad tap grid, frequency grid, blocks or segments")
    Q = B * S
    if K > MAX_BINS or Q > MAX_ALL_SEGMENTS or Q > W:
        raise ValueError("too many frequencies or segments")
    if W > len(ring) or s0 < 0:
        raise ValueError("window outside the ring")
    z = np.zeros((Q, T), dtype=np.complex128)
    tau = np.zeros(Q)
    for q in range(Q):
        a, b = (q * W) // Q, ((q + 1) * W) // Q
        x = ring[(s0 + np.arange(a, b)) % len(ring)]
        rem_carrier_q = (rem_carrier + (-(f0 * 2.0 * np.pi * a / fs))) % (2 * np.pi)
        rem_code_q = rem_code + float(a) * code_step
        for j in range(T):
            s_j = first_chips + j * step_chips
            z[q, j] = _epl_tap(x, code, fs, f0, rem_carrier_q, rem_code_q, code_step, s_j)
        tau[q] = (a + b - 1) / 2.0 / fs
    d = (np.arange(K) - (K - 1) // 2) * step_hz
    cmap = np.zeros((K, T))
    for b in range(B):
        Z = np.zeros((K, T), dtype=np.complex128)
        for s in range(S):
            q = b * S + s
            Z = Z + z[q][None, :] * np.exp(-2j * np.pi * d * tau[q])[:, None]
        cmap = cmap + np.abs(Z) ** 2
    return DdmResult(peak_of_map(cmap, f0, first_chips, step_chips, step_hz), cmap, z, tau)


def peak_of_map(cmap, f0, first_chips, step_chips, step_hz):
    """The result record of one item's map[K][T] (the text of the module's docstring)."""
    K, T = cmap.shape
    s = first_chips + np.arange(T) * step_chips
    if not np.isfinite(cmap).all():       # a window that held NaN / Inf: reported, not searched
        return dict(peak_bin=(K - 1) // 2, peak_tap=0, peak_hz=float(f0), peak_chips=float(first_chips),
                    peak_value=np.nan, second_value=np.nan, noise_mean=np.nan)
    k, j = np.unravel_index(int(np.argmax(cmap)), cmap.shape)   # the first maximum in row-major order
    away = np.abs(s - s[j]) >= 1.0
    rest = cmap[:, away]
    return dict(peak_bin=int(k), peak_tap=int(j), peak_hz=float(f0 + (k - (K - 1) // 2) * step_hz), peak_chips=float(s[j]),
                peak_value=float(cmap[k, j]), second_value=float(rest.max()) if rest.size else 0.0,
                noise_mean=float(rest.mean()) if rest.size else 0.0)


def segments_for(n_samples, n_blocks, period_samples, fraction=0.25):
    """S such that a segment of a window of n_samples in n_blocks blocks is `fraction` of a code period (of
    period_samples) or shorter -- a quarter period: the phasor of a 500 Hz offset turns by 45 degrees over a C/A segment --
    within the call's 2 <= S <= 64 (two: one segment per block carries no frequency information)."""
    return int(min(MAX_SEGMENTS, max(2, np.ceil(n_samples / max(1, n_blocks) / (fraction * period_samples)))))


def DelayDopplerMap(rfData, code, samplingFrequency, carrierFrequency, remainingCarrier=0.0, remainingCode=0.0,
                    codeStep=None, nbBlocks=1, nbSegments=8, firstChips=-4.0, stepChips=0.25, nbTaps=33,
                    frequencySpan=500.0, frequencyStep=25.0, codeFrequency=1.023e6):
    """The delay-Doppler map of `rfData` around a predicted code phase and carrier, on the GPU (sdr_ddm; no counterpart
    in the reference).  `code`: the +-1 chips of one period (not padded); `remainingCode` the predicted code phase in
    chips at rfData[0], `carrierFrequency` the predicted carrier (IF included), `codeStep` chips per sample (None:
    codeFrequency / samplingFrequency).
    -> (codePhase = remainingCode + peak_chips, carrier = peak_hz, map[K][nbTaps], result record)."""
    from ..engine import FMT_CF64, make_items
    from ..runtime import get_engine
    rf = np.squeeze(np.asarray(rfData, dtype=np.complex128))
    chips = np.asarray(code)
    step = float(codeFrequency) / float(samplingFrequency) if codeStep is None else float(codeStep)
    eng = get_engine()
    if getattr(eng, "n_slots", 0) < 4:
        eng.code_slots(4, 4092)
    eng.set_code(3, chips.astype(np.int8))
    cap = (rf.size + 7) // 8 * 8
    if eng.iq_fmt != FMT_CF64 or eng.iq_capacity < cap:
        eng.iq_alloc(cap, FMT_CF64)
    eng.iq_upload(rf, 0)
    items = make_items(3, rf.size, 0, float(carrierFrequency), float(remainingCarrier), float(remainingCode), step)
    res, cmap, _ = eng.ddm(items, samplingFrequency, nbBlocks, nbSegments, firstChips, stepChips, nbTaps, frequencySpan,
                           frequencyStep)
    return float(remainingCode) + float(res["peak_chips"][0]), float(res["peak_hz"][0]), cmap[0], res[0]


__all__ = ["ddm_statement", "DelayDopplerMap", "ddm_bins", "peak_of_map", "segments_for", "DdmResult"]
