"""Acquisition of any staged code: chip rate, code period and the zero-padded search (sdr_pcps_signal, include/sydr_amd.h).

`pcps_signal_statement` is the definition in NumPy -- host arithmetic, the yardstick of the tests, no part of the search --
and `PCPSSignal` the function-level call in the shape of dsp.acquisition.PCPS, computed by the HIP library.

A signal whose symbol lasts one code period (E1-B/C, L5, L1C, B1C, what sdr_iq_synth writes for any code that is not 1023
chips long) flips sign at a code boundary, and that boundary lies inside almost every search window: the circular
correlation over one period then splits its peak over the neighbouring Doppler bins.  pad = 1 correlates two periods of
signal with one period of code followed by zeros -- a linear correlation, whose lags below one period each see one whole,
unbroken code period -- and keeps those lags alone.  A BOC(1,1) signal is searched as its half-chip code (`boc_doubled`) at
twice the chip rate, with `excl_samples` covering the side peaks.

Behind that search, `SecondarySync` (sdr_acq_secondary) finds where the secondary (overlay) code of such a signal stands and
its carrier to a fine grid's step; NH10 and NH20 are the two Neuman-Hofman codes (L5-I, L5-Q), the only secondary tables here."""
from __future__ import annotations

import numpy as np


def _bits(text):
    """'0' -> +1, '1' -> -1."""
    return np.array([1 if b == "0" else -1 for b in text], dtype=np.int8)


NH10 = _bits("0000110101")
NH20 = _bits("00000100110101001110")


def boc_doubled(code):
    """The half-chip code of a BOC(1,1) signal: every chip c becomes (c, -c); searched and tracked at twice the chip rate."""
    code = np.asarray(code)
    return np.stack([code, -code], axis=1).reshape(-1)


def samples_per_code(fs, n_chips, chip_rate_hz) -> int:
    """N = nearbyint(fs * L / chip_rate_hz), halves to the even neighbour."""
    return int(np.rint(float(fs) * int(n_chips) / float(chip_rate_hz)))


def replica(code, fs, chip_rate_hz, n=None):
    """r[k] = c[min(trunc((ts * k) / tc), L - 1)], k < N: the reference's UpsampleCode with the chip rate a parameter."""
    code = np.asarray(code)
    if n is None:
        n = samples_per_code(fs, len(code), chip_rate_hz)
    ts = 1 / fs
    tc = 1 / chip_rate_hz
    idx = np.trunc(ts * np.array(range(n)) / tc).astype(int)
    return code[np.minimum(idx, len(code) - 1)]


def two_peak_compare(cmap, n_code, samples_per_chip):
    """([bin, code], ratio) of sdr_two_peak_compare (the reference's TwoCorrelationPeakComparison, its window quirks kept)."""
    top = np.unravel_index(cmap.argmax(), cmap.shape)
    top = [int(top[0]), int(top[1])]
    p1 = cmap[top[0], top[1]]
    lo = int(top[1] - samples_per_chip)
    hi = int(top[1] + samples_per_chip)
    if lo < 1:
        cols = list(range(hi, n_code - 1))
    elif hi >= n_code:
        cols = list(range(0, lo))
    else:
        cols = list(range(0, lo)) + list(range(hi, n_code - 1))
    p2 = np.amax(cmap[top[0], cols])
    return top, p1 / p2


def pcps_signal_statement(x, codes, fs, if_hz, doppler_range, doppler_step, chip_rate_hz, pad=0, excl_samples=0, coh=1,
                          noncoh=1, start_sample=0):
    """sdr_pcps_signal in NumPy.  x: the ring's samples (complex, flat; the window wraps at its end), codes: [n_prn][L].
    -> (peak_bin[n_prn], peak_code[n_prn], peak_ratio[n_prn], map[n_prn][bins][N])."""
    x = np.squeeze(np.asarray(x, dtype=np.complex128))
    codes = np.atleast_2d(np.asarray(codes))
    if pad not in (0, 1) or (pad == 1 and coh != 1):
        raise ValueError("pad is 0 or 1, and 1 takes coh = 1")
    n_code = samples_per_code(fs, codes.shape[1], chip_rate_hz)
    t_len = n_code * (1 + pad)
    span = t_len if pad else coh * n_code              # samples one block reads
    hop = n_code if pad else coh * n_code              # samples between two blocks
    bins = np.arange(-doppler_range, doppler_range + 1, doppler_step)
    spc = int(excl_samples) if excl_samples else int(np.rint(fs / chip_rate_hz))
    phase_points = np.array(range(span)) * 2 * np.pi / fs
    blocks = [x[(start_sample + k * hop + np.arange(span)) % x.size] for k in range(noncoh)]
    n_prn = codes.shape[0]
    cmap = np.zeros((n_prn, len(bins), n_code))
    code_fft = [np.conj(np.fft.fft(np.r_[replica(c, fs, chip_rate_hz, n_code), np.zeros(t_len - n_code)])) for c in codes]
    for row, b in enumerate(bins):
        freq = if_hz - b
        carrier = np.exp(-1j * freq * phase_points)
        spectra = [[np.fft.fft(np.multiply(carrier, blk)[c * t_len:(c + 1) * t_len]) for c in range(span // t_len)]
                   for blk in blocks]
        for p in range(n_prn):
            noncoh_sum = np.zeros((1, t_len))
            for k in range(noncoh):
                coh_sum = noncoh_sum * 0.0
                for spec in spectra[k]:
                    coh_sum = coh_sum + np.fft.ifft(np.multiply(spec, code_fft[p]))
                noncoh_sum = noncoh_sum + abs(coh_sum)
            cmap[p, row, :] = abs(noncoh_sum)[0, :n_code]
    peak_bin = np.empty(n_prn, dtype=np.int64)
    peak_code = np.empty(n_prn, dtype=np.int64)
    ratio = np.empty(n_prn, dtype=np.float64)
    for p in range(n_prn):
        top, ratio[p] = two_peak_compare(cmap[p], n_code, spc)
        peak_bin[p], peak_code[p] = top
    return peak_bin, peak_code, ratio, cmap


def PCPSSignal(rfData, interFrequency, samplingFrequency, code, chipRate, dopplerRange, dopplerStep, pad=0, exclSamples=0,
               coherentIntegration=1, nonCoherentIntegration=1):
    """Correlation map [bins][N] of one code (its chips, at `chipRate`) over `rfData`, on the GPU, in the shape of
    dsp.acquisition.PCPS: pad = 1 searches zero-padded over two code periods.  -> (map, [bin, code], peak ratio)."""
    from ..engine import FMT_CF64           # (the statement above needs no library)
    from ..runtime import get_engine
    rf = np.squeeze(np.asarray(rfData, dtype=np.complex128))
    chips = np.asarray(code)
    n_code = samples_per_code(samplingFrequency, len(chips), chipRate)
    blocks = int(nonCoherentIntegration) + 1 if pad else int(coherentIntegration) * int(nonCoherentIntegration)
    need = n_code * blocks
    if rf.size < need:
        raise ValueError(f"PCPSSignal needs {need} samples, got {rf.size}")
    eng = get_engine()
    if getattr(eng, "n_slots", 0) < 4 or getattr(eng, "max_chips", 0) < len(chips):
        eng.code_slots(4, max(4092, len(chips)))
    eng.set_code(3, chips.astype(np.int8))
    cap = (need + 7) // 8 * 8
    if eng.iq_fmt != FMT_CF64 or eng.iq_capacity < cap:
        eng.iq_alloc(cap, FMT_CF64)
    eng.iq_upload(rf[:need], 0)
    pb, pc, pr, cmap = eng.pcps_signal([3], 0, samplingFrequency, interFrequency, dopplerRange, dopplerStep, chipRate, pad=pad,
                                       excl_samples=exclSamples, coh=coherentIntegration, noncoh=nonCoherentIntegration,
                                       want_map=True, n_chips=len(chips))
    return np.squeeze(np.squeeze(cmap[0])), [int(pb[0]), int(pc[0])], float(pr[0])


def SecondarySync(rfData, samplingFrequency, code, chipRate, secondary, coarseFrequency, nbPeriods, nbSegments=4,
                  frequencySpan=125.0, frequencyStep=5.0, mode=0):
    """Secondary-code phase and fine carrier frequency behind an acquisition (the definition is sdr_acq_secondary's in
    include/sydr_amd.h), on the GPU, in the shape of dsp.acquisition.FineFrequencySearch.  `rfData` starts where a period of
    the primary `code` (its chips, at `chipRate`) begins and holds `nbPeriods` periods; `secondary` = the +-1 chips of the
    overlay code, one per primary period; `coarseFrequency` = the carrier the search found (IF included); mode 0: a pilot,
    1: a data symbol as long as the secondary period.
    -> (fineFrequency, secPhase, powerRatio, P[len(secondary)][K]): secPhase = the secondary chip the first period carries,
    powerRatio = the best cell over the best cell of any other phase."""
    from ..engine import FMT_CF64, make_secondary_items
    from ..runtime import get_engine
    rf = np.squeeze(np.asarray(rfData, dtype=np.complex128))
    chips = np.asarray(code)
    need = samples_per_code(samplingFrequency, len(chips), chipRate) * int(nbPeriods)
    if rf.size < need:
        raise ValueError(f"SecondarySync needs {need} samples, got {rf.size}")
    eng = get_engine()
    if getattr(eng, "n_slots", 0) < 4 or getattr(eng, "max_chips", 0) < len(chips):
        eng.code_slots(4, max(4092, len(chips)))
    eng.set_code(3, chips.astype(np.int8))
    cap = (need + 7) // 8 * 8
    if eng.iq_fmt != FMT_CF64 or eng.iq_capacity < cap:
        eng.iq_alloc(cap, FMT_CF64)
    eng.iq_upload(rf[:need], 0)
    res, power, _ = eng.acq_secondary(make_secondary_items(3, 0, 0, coarseFrequency, chipRate), np.asarray(secondary),
                                      samplingFrequency, nbPeriods, nbSegments, frequencySpan, frequencyStep, mode, want_tables=True)
    return float(res["fine_hz"][0]), int(res["sec_phase"][0]), float(res["power"][0] / res["power_other"][0]), power[0]
