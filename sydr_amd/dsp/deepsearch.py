"""Deep acquisition (sdr_acq_deep, include/sydr_amd.h): its NumPy statement, written as plainly as the oracle's
`pcps_map`, and the function-level drop-in that computes the same map on the GPU.

The reference's PCPS(coherentIntegration, nonCoherentIntegration) sums a coherent block across data-bit edges and adds
the maps of successive blocks at a fixed code index; on weak signals both cost the peak.  The deep search folds each
coherent block in front of ONE transform, adds the blocks into `groups` interleaved sets (with two sets and blocks of
half a bit, one set holds no edge) and moves every block's map back by the code's drift at the bin's Doppler."""
from __future__ import annotations

import numpy as np

from ..engine import FMT_CF64
from ..runtime import get_engine
from ..utils.constants import GPS_L1CA_CODE_FREQ


def doppler_bins(dopplerRange, dopplerStep):
    """The search grid of acquisition.py:30."""
    return np.arange(-dopplerRange, dopplerRange + 1, dopplerStep)


def deep_shift(dopplerRange, dopplerStep, samplesPerCode, coherentIntegration, carrierFrequencyRF, bin_idx, block):
    """q[b][i] = nearbyint(d_b * float(i*C*N) / carrier_rf_hz): samples the code has drifted by at the start of block i
    on Doppler bin b (fp64 in this order, half-even; 0 without compensation) -- sdr_acq_deep_shift."""
    if not carrierFrequencyRF > 0.0:
        return 0
    d = float(doppler_bins(dopplerRange, dopplerStep)[bin_idx])
    return int(np.rint(d * float(int(block) * int(coherentIntegration) * int(samplesPerCode)) / float(carrierFrequencyRF)))


def deep_map(rfData, interFrequency, samplingFrequency, codeFFT, dopplerRange, dopplerStep, samplesPerCode,
             coherentIntegration=1, nonCoherentIntegration=1, groups=1, carrierFrequencyRF=0.0):
    """The statement: M[g][b][n] of sdr_acq_deep for one PRN, float64[groups][bins][samplesPerCode]."""
    rf = np.squeeze(np.asarray(rfData, dtype=np.complex128))
    N, C, K, G = int(samplesPerCode), int(coherentIntegration), int(nonCoherentIntegration), int(groups)
    bins = doppler_bins(dopplerRange, dopplerStep)
    phi = np.array(range(C * N)) * 2 * np.pi / samplingFrequency
    out = np.zeros((G, len(bins), N))
    for b, d in enumerate(bins):
        carrier = np.exp(-1j * (interFrequency - d) * phi)
        for i in range(K):
            block = rf[i * C * N:(i + 1) * C * N] * carrier
            folded = block.reshape(C, N).sum(axis=0) if C > 1 else block
            r = np.abs(np.fft.ifft(np.fft.fft(folded) * codeFFT))
            q = deep_shift(dopplerRange, dopplerStep, N, C, carrierFrequencyRF, b, i)
            out[i % G, b] += r[(np.arange(N) + q) % N]
    return out


def deep_code_end(peak_bin, peak_code, dopplerRange, dopplerStep, samplesPerCode, coherentIntegration,
                  nonCoherentIntegration, carrierFrequencyRF):
    """peak_code_end: the code start referred to the window's end."""
    return (int(peak_code) + deep_shift(dopplerRange, dopplerStep, samplesPerCode, coherentIntegration, carrierFrequencyRF,
                                        peak_bin, nonCoherentIntegration)) % int(samplesPerCode)


def deep_detect(M, n_peaks, excl_code, excl_bins):
    """The statement of sdr_acq_deep_detect's figures for one PRN's map M[G][B][N] (include/sydr_amd.h):
    -> (peaks, noise).  peaks: n_peaks dicts(group, bin, code, value, z) -- peak k is the first maximum, in row-major
    (g, b, n) order, outside the zones |b - b_j| <= excl_bins, dist(n, n_j) <= excl_code (every g) of the peaks j < k;
    group = -1, value = 0.0 where no cell is left.  noise: dict(n_cells, mean, variance) of the cells whose code column lies
    further than excl_code (circularly) from every reported peak's, in all bins and groups: two passes, population variance.
    z = (value - mean) / sqrt(variance) in fp64, in this order."""
    M = np.asarray(M, dtype=np.float64)
    if M.ndim != 3:
        raise ValueError("deep_detect takes one PRN's map [groups][bins][samplesPerCode]")
    G, B, N = M.shape
    n_peaks, excl_code, excl_bins = int(n_peaks), int(excl_code), int(excl_bins)
    if not 1 <= n_peaks <= 8:
        raise ValueError(f"n_peaks = {n_peaks} outside 1..8")
    if excl_code < 0 or excl_bins < 0:
        raise ValueError("negative exclusion window")
    if n_peaks * (2 * excl_code + 1) >= N:
        raise ValueError(f"{n_peaks} peaks x (2 x {excl_code} + 1) excluded columns leave no noise cell of {N}")
    n = np.arange(N)
    b = np.arange(B)
    free = np.ones((B, N), dtype=bool)          # outside every zone so far (the same for every group)
    columns = np.ones(N, dtype=bool)            # code columns clear of every reported peak
    peaks = []
    for _ in range(n_peaks):
        if not free.any():
            peaks.append(dict(group=-1, bin=0, code=0, value=0.0))
            continue
        masked = np.where(free[None, :, :], M, -np.inf)
        g_k, b_k, n_k = (int(v) for v in np.unravel_index(np.argmax(masked), M.shape))
        peaks.append(dict(group=g_k, bin=b_k, code=n_k, value=float(M[g_k, b_k, n_k])))
        d = np.abs(n - n_k)
        near = np.minimum(d, N - d) <= excl_code
        free &= ~((np.abs(b - b_k) <= excl_bins)[:, None] & near[None, :])
        columns &= ~near
    cells = M[:, :, columns].ravel()
    n_cells = int(cells.size)
    mean = float(np.sum(cells)) / n_cells
    dev = cells - mean
    variance = float(np.sum(dev * dev)) / n_cells
    for p in peaks:
        with np.errstate(divide="ignore", invalid="ignore"):
            p["z"] = float((np.float64(p["value"]) - mean) / np.sqrt(np.float64(variance)))
    return peaks, dict(n_cells=n_cells, mean=mean, variance=variance)


def _chips_of_spectrum(codeFFT, samplingFrequency):
    """The chips behind codeFFT = conj(fft(UpsampleCode(code))) (gnsssignal.py:53: sample k holds chip trunc(k*ts/tc))."""
    up = np.rint(np.real(np.fft.ifft(np.conj(np.asarray(codeFFT, dtype=np.complex128)))))
    idx = np.trunc((1.0 / samplingFrequency) * np.arange(len(up)) / (1.0 / GPS_L1CA_CODE_FREQ)).astype(int)
    first = np.unique(idx, return_index=True)[1]
    return up[first].astype(np.int8)


def _stage(rfData, samplingFrequency, code, samplesPerCode, coherentIntegration, nonCoherentIntegration, who):
    """The window in a cf64 ring from sample 0 and the chips in slot 3 of the process's engine."""
    rf = np.squeeze(np.asarray(rfData, dtype=np.complex128))
    need = int(samplesPerCode) * int(coherentIntegration) * int(nonCoherentIntegration)
    if rf.size < need:
        raise ValueError(f"{who} needs {need} samples, got {rf.size}")
    code = np.asarray(code)
    chips = _chips_of_spectrum(code, samplingFrequency) if np.iscomplexobj(code) else code.astype(np.int8)
    eng = get_engine()
    if getattr(eng, "n_slots", 0) < 4:
        eng.code_slots(4, 4092)
    eng.set_code(3, chips)
    cap = (need + 7) // 8 * 8
    if eng.iq_fmt != FMT_CF64 or eng.iq_capacity < cap:
        eng.iq_alloc(cap, FMT_CF64)
    eng.iq_upload(rf[:need], 0)
    return eng


def DeepSearch(rfData, interFrequency, samplingFrequency, code, dopplerRange, dopplerStep, samplesPerCode,
               coherentIntegration=1, nonCoherentIntegration=1, groups=1, carrierFrequencyRF=0.0):
    """Correlation map [groups][bins][samplesPerCode] of the statement above, on the GPU.  `code`: the chips (+-1), or
    codeFFT = conj(fft(UpsampleCode(code))) of length samplesPerCode as PCPS takes it (the chips are read back from it)."""
    eng = _stage(rfData, samplingFrequency, code, samplesPerCode, coherentIntegration, nonCoherentIntegration, "DeepSearch")
    _, cmap = eng.acq_deep([3], 0, samplingFrequency, interFrequency, dopplerRange, dopplerStep, coherentIntegration,
                           nonCoherentIntegration, groups, carrierFrequencyRF, want_map=True)
    return cmap[0]


def DeepDetect(rfData, interFrequency, samplingFrequency, code, dopplerRange, dopplerStep, samplesPerCode,
               coherentIntegration=1, nonCoherentIntegration=1, groups=1, carrierFrequencyRF=0.0, n_peaks=1, excl_code=0,
               excl_bins=0, want_map=False):
    """`deep_detect`'s (peaks, noise) of DeepSearch's map, made on the GPU where the map lies (sdr_acq_deep_detect); the
    peaks carry `code_end` too.  With want_map -> (peaks, noise, map [groups][bins][samplesPerCode])."""
    eng = _stage(rfData, samplingFrequency, code, samplesPerCode, coherentIntegration, nonCoherentIntegration, "DeepDetect")
    _, peaks, noise, cmap = eng.acq_deep_detect([3], 0, samplingFrequency, interFrequency, dopplerRange, dopplerStep,
                                                coherentIntegration, nonCoherentIntegration, groups, carrierFrequencyRF,
                                                n_peaks, excl_code, excl_bins, want_map=want_map)
    out = ([dict(group=int(p["group"]), bin=int(p["bin"]), code=int(p["code"]), code_end=int(p["code_end"]),
                 value=float(p["value"]), z=float(p["z"])) for p in peaks[0]],
           dict(n_cells=int(noise[0]["n_cells"]), mean=float(noise[0]["mean"]), variance=float(noise[0]["variance"])))
    return out + (cmap[0],) if want_map else out
