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
its carrier to a fine grid's step; NH10 and NH20 are the two Neuman-Hofman codes (L5-I, L5-Q), the only secondary tables here.

`CoherentSearch` (sdr_pcps_coherent, statement `pcps_coherent_statement`) is both steps at once for a weak signal: the padded
search's per-period correlations added coherently under every overlay phase and every frequency of a fine grid."""
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


def fine_grid(span_hz, step_hz):
    """d_k = (k - (K-1)/2) * step_hz, K = 2*floor(span_hz/step_hz) + 1 (sdr_acq_refine_bins)."""
    k = 2 * int(np.floor(span_hz / step_hz)) + 1
    return (np.arange(k) - (k - 1) // 2) * step_hz


def _coh_rotation(freq, m, n_code, fs):
    """g = exp(-2j*pi*freq*(m*N)/fs), from the phase in cycles less its nearest whole number."""
    ph = freq * ((m * n_code) / fs)
    return np.exp(-1j * (2 * np.pi * (ph - np.rint(ph))))


def coherent_cell(col, sec, freqs, n_code, fs, mode=0):
    """P[Ls][K] and X[Ls][K] of one cell from its M per-period correlations `col`, m ascending (mode 1: X = 0)."""
    sec = np.asarray(sec, dtype=np.float64)
    n_per, n_sec = len(col), len(sec)
    power = np.zeros((n_sec, len(freqs)))
    prompt = np.zeros((n_sec, len(freqs)), complex)
    for k, f in enumerate(freqs):
        z = [col[m] * _coh_rotation(f, m, n_code, fs) for m in range(n_per)]
        for h in range(n_sec):
            acc, groups = 0j, 0.0
            for m in range(n_per):
                acc = acc + sec[(h + m) % n_sec] * z[m]
                if mode == 1 and (h + m) % n_sec == n_sec - 1:
                    groups, acc = groups + abs(acc) ** 2, 0j
            power[h, k] = groups + abs(acc) ** 2
            prompt[h, k] = acc if mode == 0 else 0j
    return power, prompt


def pcps_coherent_statement(x, codes, sec_codes, sec_rows, fs, if_hz, doppler_range, doppler_step, chip_rate_hz, n_periods,
                            span_hz=125.0, step_hz=25.0, mode=0, excl_samples=0, start_sample=0):
    """sdr_pcps_coherent in NumPy.  x: the ring's samples (complex, flat; the window wraps at its end), codes: [n_prn][L],
    sec_codes: [n_sec][Ls] of +-1, sec_rows: the row of every PRN.
    -> (results: COH_RESULT_DTYPE records, R[n_prn][bins][N], P[n_prn][Ls][K] at each PRN's peak cell)."""
    from .._lib import COH_RESULT_DTYPE     # (a record layout: no library is loaded)
    x = np.squeeze(np.asarray(x, dtype=np.complex128))
    codes = np.atleast_2d(np.asarray(codes))
    sec_codes = np.atleast_2d(np.asarray(sec_codes))
    n_prn = codes.shape[0]
    sec_rows = np.broadcast_to(np.asarray(sec_rows, dtype=int), (n_prn,))
    n_per, n_sec = int(n_periods), sec_codes.shape[1]
    n_code = samples_per_code(fs, codes.shape[1], chip_rate_hz)
    t_len = 2 * n_code
    bins = np.arange(-doppler_range, doppler_range + 1, doppler_step)
    fine = fine_grid(span_hz, step_hz)
    spc = int(excl_samples) if excl_samples else int(np.rint(fs / chip_rate_hz))
    phase_points = np.array(range(t_len)) * 2 * np.pi / fs
    blocks = [x[(start_sample + m * n_code + np.arange(t_len)) % x.size] for m in range(n_per)]
    code_fft = [np.conj(np.fft.fft(np.r_[replica(c, fs, chip_rate_hz, n_code), np.zeros(n_code)])) for c in codes]
    spectra = [[np.fft.fft(np.exp(-1j * (if_hz - b) * phase_points) * blk) for blk in blocks] for b in bins]
    results = np.zeros(n_prn, dtype=COH_RESULT_DTYPE)
    rmap = np.zeros((n_prn, len(bins), n_code))
    tables = np.zeros((n_prn, n_sec, len(fine)))
    for p in range(n_prn):
        sec = sec_codes[sec_rows[p]].astype(np.float64)
        idx = (np.arange(n_sec)[:, None] + np.arange(n_per)[None, :])          # h + m
        signs = sec[idx % n_sec]                                                # w_h(m)
        corr = []
        for row, b in enumerate(bins):
            c = np.array([np.fft.ifft(spec * code_fft[p])[:n_code] for spec in spectra[row]])      # C_m[tau]
            corr.append(c)
            best = np.zeros(n_code)
            for d in fine:
                z = c * _coh_rotation((if_hz - b) + d, np.arange(n_per), n_code, fs)[:, None]
                if mode == 0:
                    pw = np.abs(signs @ z) ** 2
                else:
                    pw = np.zeros((n_sec, n_code))
                    for h in range(n_sec):
                        grp = idx[h] // n_sec
                        for gg in np.unique(grp):
                            pw[h] += np.abs(signs[h, grp == gg] @ z[grp == gg]) ** 2
                best = np.fmax(best, np.fmax.reduce(pw, axis=0))                # (a NaN never wins)
            rmap[p, row] = np.sqrt(best)
        top, ratio = two_peak_compare(rmap[p], n_code, spc)
        b_top = bins[top[0]]
        power, prompt = coherent_cell(corr[top[0]][:, top[1]], sec, [(if_hz - b_top) + d for d in fine], n_code, fs, mode)
        h, k = np.unravel_index(power.argmax(), power.shape)                    # first maximum in row-major order
        tables[p] = power
        r = results[p]
        r["carrier_hz"] = (if_hz - b_top) + fine[k]
        r["peak"], r["peak_ratio"] = rmap[p, top[0], top[1]], ratio
        r["power"], r["power_other"] = power[h, k], np.delete(power, h, axis=0).max()
        r["prompt_re"], r["prompt_im"] = prompt[h, k].real, prompt[h, k].imag
        r["peak_code"], r["peak_bin"], r["fine_idx"], r["sec_phase"] = top[1], top[0], k, h
    return results, rmap, tables


def CoherentSearch(rfData, interFrequency, samplingFrequency, code, chipRate, secondary, dopplerRange, dopplerStep, nbPeriods,
                   frequencySpan=125.0, frequencyStep=25.0, mode=0, exclSamples=0):
    """Coherent search of one code (its chips, at `chipRate`) under its `secondary` (overlay) code over `rfData`, on the GPU, in
    the shape of PCPSSignal / SecondarySync (the definition is sdr_pcps_coherent's in include/sydr_amd.h): `nbPeriods` code
    periods are added coherently under every overlay phase and every frequency of the fine grid; `rfData` holds
    `nbPeriods` + 1 periods.  mode 0: a pilot, 1: a data symbol as long as the overlay code.
    -> (map R[bins][N], [bin, code], peak ratio, carrierFrequency, secPhase, powerRatio)."""
    from ..engine import FMT_CF64
    from ..runtime import get_engine
    rf = np.squeeze(np.asarray(rfData, dtype=np.complex128))
    chips = np.asarray(code)
    need = samples_per_code(samplingFrequency, len(chips), chipRate) * (int(nbPeriods) + 1)
    if rf.size < need:
        raise ValueError(f"CoherentSearch needs {need} samples, got {rf.size}")
    eng = get_engine()
    if getattr(eng, "n_slots", 0) < 4 or getattr(eng, "max_chips", 0) < len(chips):
        eng.code_slots(4, max(4092, len(chips)))
    eng.set_code(3, chips.astype(np.int8))
    cap = (need + 7) // 8 * 8
    if eng.iq_fmt != FMT_CF64 or eng.iq_capacity < cap:
        eng.iq_alloc(cap, FMT_CF64)
    eng.iq_upload(rf[:need], 0)
    res, cmap, _ = eng.pcps_coherent([3], 0, np.asarray(secondary), 0, samplingFrequency, interFrequency, dopplerRange, dopplerStep,
                                     chipRate, nbPeriods, frequencySpan, frequencyStep, mode, exclSamples, want_map=True,
                                     n_chips=len(chips))
    r = res[0]
    return (cmap[0], [int(r["peak_bin"]), int(r["peak_code"])], float(r["peak_ratio"]), float(r["carrier_hz"]),
            int(r["sec_phase"]), float(r["power"] / r["power_other"]))
