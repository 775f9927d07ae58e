"""What tests/test_detect.py (CPU) and tests/test_gpu_detect.py (MI355X) share: a brute-force restatement of
sdr_acq_deep_detect's peaks and noise cells (plain loops, no NumPy masks), the exactly rounded sums the device's figures are
held to, the weak-signal and two-replica streams of the issue's tables, and the shapes of the GPU cases.  The statement
itself is the product's NumPy text (sydr_amd/dsp/deepsearch.py: deep_detect)."""
import functools
import math

import numpy as np

from oracle import sydr_oracle as orc
from sydr_amd.dsp.deepsearch import deep_detect, deep_map  # noqa: F401  (re-exported)


# ------------------------------------------------------------------------------------------------ brute force
def circular(n, m, N):
    return min((n - m) % N, (m - n) % N)


def brute_detect(M, n_peaks, excl_code, excl_bins):
    """-> (peaks [(group, bin, code, value)], the (g, b, n) of the noise cells in row-major order): every cell visited in a
    plain loop, the first maximum kept with a strict comparison, zones and columns tested with Python's own modulo."""
    G, B, N = M.shape
    peaks = []
    for _ in range(n_peaks):
        best = None
        for g in range(G):
            for b in range(B):
                for n in range(N):
                    if any(p[0] >= 0 and abs(b - p[1]) <= excl_bins and circular(n, p[2], N) <= excl_code for p in peaks):
                        continue
                    if best is None or M[g, b, n] > best[3]:
                        best = (g, b, n, float(M[g, b, n]))
        peaks.append(best if best is not None else (-1, 0, 0, 0.0))
    cells = [(g, b, n) for g in range(G) for b in range(B) for n in range(N)
             if all(circular(n, p[2], N) > excl_code for p in peaks if p[0] >= 0)]
    return peaks, cells


def noise_columns(peaks, N, excl_code):
    """The code columns clear of every reported peak (peaks: dicts or records with group / code)."""
    keep = np.ones(N, dtype=bool)
    n = np.arange(N)
    for p in peaks:
        if int(p["group"]) >= 0:
            d = np.abs(n - int(p["code"]))
            keep &= np.minimum(d, N - d) > excl_code
    return keep


def exact_moments(M, columns, mean):
    """(n_cells, math.fsum of the noise cells, math.fsum of their squared deviations from `mean` -- each deviation and each
    square rounded to fp64 as the statement rounds them, the sum exact)."""
    cells = np.ascontiguousarray(M[:, :, columns]).ravel()
    dev = cells - np.float64(mean)
    return int(cells.size), math.fsum(cells.tolist()), math.fsum((dev * dev).tolist())


def moment_bound(n_cells):
    """Fixed-order fp64 sums of n non-negative terms lie within n * 2^-53 (relative) of the exact sum; the division by
    n_cells and the reference's own rounding take the rest of (n_cells + 4) * 2^-53."""
    return (n_cells + 4) * 2.0 ** -53


def host_z(value, mean, variance):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((np.float64(value) - np.float64(mean)) / np.sqrt(np.float64(variance)))


# ------------------------------------------------------------------------------------------------ the issue's streams
WEAK = dict(fs=4e6, N=4000, C=5, K=40, R=500.0, S=100.0, G=1, rf=0.0, prn=7, absent=12, doppler=200.0, chips=300.0,
            cn0_dbhz=27.0, excl_code=4, excl_bins=1, n_peaks=3, cell=(3, 2827))
REPLICA = dict(cn0_dbhz=33.0, seed=100, amp=0.8, doppler=-300.0, chips=650.0, cells=((3, 2827), (8, 1458)), n_peaks=4)


def replica(prn, n, fs, doppler, chips0, amp=1.0, first=0):
    t = np.arange(first, first + n, dtype=np.float64)
    chip = (chips0 + t * 1.023e6 / fs) % 1023
    code = orc.gold_code(prn).astype(np.float64)
    return amp * code[np.floor(chip).astype(np.int64)] * np.exp(2j * np.pi * doppler * t / fs)


@functools.lru_cache(maxsize=None)
def weak_stream(seed, two_replicas=False):
    """The issue's stream: PRN 7, amplitude 1, +200 Hz, 300.0 chips at sample 0, no data bits, in complex white noise of
    sigma = sqrt(fs / (2 * 10^(C/N0 / 10))) per axis -- 27 dB-Hz, or 33 dB-Hz with a second copy at 0.8, -300 Hz, 650.0 chips."""
    w = WEAK
    n = w["C"] * w["K"] * w["N"]
    x = replica(w["prn"], n, w["fs"], w["doppler"], w["chips"])
    cn0 = REPLICA["cn0_dbhz"] if two_replicas else w["cn0_dbhz"]
    if two_replicas:
        x = x + replica(w["prn"], n, w["fs"], REPLICA["doppler"], REPLICA["chips"], REPLICA["amp"])
    sigma = np.sqrt(w["fs"] / (2 * 10 ** (cn0 / 10)))
    rng = np.random.default_rng(seed)
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x.setflags(write=False)
    return x


def weak_tail(seed, ms, two_replicas=False):
    """`ms` more milliseconds of `weak_stream` (the signals continue; noise of a generator of its own, so the stream's
    figures stand) -- what a channel tracks on behind its search window."""
    w = WEAK
    first, n = w["C"] * w["K"] * w["N"], ms * w["N"]
    x = replica(w["prn"], n, w["fs"], w["doppler"], w["chips"], first=first)
    cn0 = REPLICA["cn0_dbhz"] if two_replicas else w["cn0_dbhz"]
    if two_replicas:
        x = x + replica(w["prn"], n, w["fs"], REPLICA["doppler"], REPLICA["chips"], REPLICA["amp"], first=first)
    sigma = np.sqrt(w["fs"] / (2 * 10 ** (cn0 / 10)))
    rng = np.random.default_rng(1000000 + seed)
    return x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def quantised(x, scale=16.0):
    """complex int16, scaled and rounded: (interleaved int16 image, the values as complex128)."""
    raw = np.empty(2 * x.size, dtype=np.int16)
    raw[0::2] = np.rint(x.real * scale)
    raw[1::2] = np.rint(x.imag * scale)
    return raw, raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)


def weak_map(x, prn):
    w = WEAK
    return deep_map(x, 0.0, w["fs"], orc.code_spectrum(orc.gold_code(prn), w["fs"]), w["R"], w["S"], w["N"], w["C"], w["K"],
                    w["G"], w["rf"])


def two_peak_ratio(M, fs):
    """The reference's two-peak ratio on the winning row's map, as sdr_acq_deep reports it."""
    g = int(np.unravel_index(int(np.argmax(M)), M.shape)[0])
    return float(orc.two_peak_compare(M[g], M.shape[2], round(fs / orc.CODE_RATE))[1])


# ------------------------------------------------------------------------------------------------ the GPU cases
# name -> sampling rate (N = 4000; the chirp-z length 4006 = 2 mod 4, whose rows all start on a 16-byte boundary; the odd
# length 4001 with 3 rows per PRN, where every other row does not and PRN 1's rows have the opposite parity of PRN 0's), ring
# format (3 = cf64, 0 = ci8), satellites (prn, doppler, code sample the peak falls on), the search (R, S, C, K, G) and the
# detector (n_peaks, excl_code, excl_bins).
def _gpu(fs=4e6, fmt=3, sats=((7, 500.0, 1), (21, -1000.0, -2)), prns=(7, 21), R=1000.0, S=250.0, C=2, K=4, G=2, n_peaks=8,
         excl_code=4, excl_bins=1):
    return dict(fs=fs, fmt=fmt, sats=sats, prns=prns, R=R, S=S, C=C, K=K, G=G, rf=0.0, if_hz=0.0, n_peaks=n_peaks,
                excl_code=excl_code, excl_bins=excl_bins)


# 9 bins: -1000..1000 by 250.  Doppler +1000 peaks on bin 0, -1000 on the last bin; code samples 1 and N - 2 wrap the zones.
GPU_CASES = {
    "cf64_two_prns_8_peaks": _gpu(),
    "ci8_two_prns_8_peaks": _gpu(fmt=0),
    "cf64_edges_wrap_and_clip": _gpu(sats=((7, 1000.0, 1), (21, -1000.0, -2))),
    "ci8_edges_wrap_and_clip": _gpu(fmt=0, sats=((7, 1000.0, 1), (21, -1000.0, -2))),
    "cf64_no_windows": _gpu(excl_code=0, excl_bins=0),
    "ci8_no_windows": _gpu(fmt=0, excl_code=0, excl_bins=0),
    "cf64_one_peak": _gpu(n_peaks=1),
    "ci8_one_peak": _gpu(fmt=0, n_peaks=1),
    "cf64_one_row": _gpu(sats=((7, 0.0, 300),), prns=(7,), R=0.0, G=1, K=2),
    "ci8_one_row": _gpu(fmt=0, sats=((7, 0.0, 300),), prns=(7,), R=0.0, G=1, K=2),
    "cf64_chirpz_4006": _gpu(fs=4.006e6, sats=((9, 250.0, 40),), prns=(9, 21), R=500.0, G=1, K=2),
    "ci8_chirpz_4006": _gpu(fs=4.006e6, fmt=0, sats=((9, 250.0, 40),), prns=(9, 21), R=500.0, G=1, K=2),
    "cf64_odd_4001": _gpu(fs=4.001e6, sats=((9, 250.0, 4000), (21, -250.0, 0)), prns=(9, 21), R=250.0, G=1, K=2),
    "ci8_odd_4001": _gpu(fs=4.001e6, fmt=0, sats=((9, 250.0, 4000), (21, -250.0, 0)), prns=(9, 21), R=250.0, G=1, K=2),
}


@functools.lru_cache(maxsize=None)
def gpu_input(name):
    """-> (case, ring image in the ring's format, ring capacity)."""
    c = GPU_CASES[name]
    fs, N = c["fs"], orc.samples_per_code(c["fs"])
    n = c["C"] * c["K"] * N
    t = np.arange(n)
    rng = np.random.default_rng(20261000 + sorted(GPU_CASES).index(name))
    x = 4.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for prn, dop, n0 in c["sats"]:
        up = orc.upsample_code(orc.gold_code(prn), fs)
        x += 3.0 * up[(t - n0) % N] * np.exp(2j * np.pi * (dop / fs * t + 0.1))
    cap = (n + 7) // 8 * 8
    if c["fmt"] == 0:
        image = np.zeros(2 * cap, dtype=np.int8)
        image[0:2 * n:2] = np.clip(np.rint(x.real), -127, 127)
        image[1:2 * n:2] = np.clip(np.rint(x.imag), -127, 127)
    else:
        image = np.zeros(cap, dtype=np.complex128)
        image[:n] = x * 0.123456789
    image.setflags(write=False)
    return c, image, cap
