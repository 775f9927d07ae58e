"""Shared by tests/test_probe.py (the NumPy statement, no GPU) and tests/test_gpu_probe.py (sdr_iq_probe on the device): the
window and spectrum case lists, sample makers, and the comparison of two ProbeResults."""
import numpy as np

CAP = 1 << 16                                   # ring samples of the GPU tests unless said otherwise
NP_OF_FMT = {0: np.int8, 1: np.int16, 2: np.float32, 3: np.float64}
FMT_NAMES = {0: "ci8", 1: "ci16", 2: "cf32", 3: "cf64"}
HIST_SHIFTS = {0: (0,), 1: (0, 4, 8)}


def moment_windows(rng, cap=CAP):
    """About 40 windows (start_sample, n): n in {1, 7, 8, 9, 63, 64, 65, random, the whole ring}, odd offsets, every third
    across the ring's end, one with start_sample = offset + 5 * capacity."""
    out = []
    sizes = [1, 7, 8, 9, 63, 64, 65, None, cap]
    for k in range(41):
        n = sizes[k % len(sizes)]
        if n is None:
            n = int(rng.integers(66, cap))
        off = int(rng.integers(0, cap // 2)) * 2 + 1                 # odd
        if k % 3 == 2 and n > 1:
            off = cap - int(rng.integers(1, n))                      # 1 .. n - 1 samples in front of the ring's end
        if k == 13:
            off += 5 * cap
        out.append((off, n))
    return out


def window(ring_raw, start, n, cap=None):
    """Interleaved samples start .. start + n - 1 (modulo the capacity) of a ring given as interleaved I,Q."""
    cap = ring_raw.size // 2 if cap is None else cap
    idx = (start + np.arange(n)) % cap
    return np.stack([ring_raw[2 * idx], ring_raw[2 * idx + 1]], axis=1).reshape(-1)


def integer_ring(rng, fmt, cap=CAP):
    """Random integers over the whole range of the type, both rails among them."""
    dt = NP_OF_FMT[fmt]
    info = np.iinfo(dt)
    raw = rng.integers(info.min, info.max + 1, 2 * cap).astype(dt)
    rails = rng.integers(0, 2 * cap, 600)
    raw[rails[:300]] = info.min
    raw[rails[300:]] = info.max
    return raw


def psd_cases():
    """(nfft, S, ragged tail): nfft in {64, 256, 1024, 4096} with S in {1, 2, 5}; S in {257, 1000} with nfft 64 only (the
    windows stay inside a 2^16 ring); tails of 0, 1 and nfft / 2 - 1 samples."""
    out = []
    for nfft in (64, 256, 1024, 4096):
        for S in (1, 2, 5) + ((257, 1000) if nfft == 64 else ()):
            for tail in (0, 1, nfft // 2 - 1):
                out.append((nfft, S, tail))
    return out


def noise_and_tone(rng, fmt, cap=CAP, fs=4e6, tone_hz=612.5e3):
    """Noise plus a strong tone in the ring's format (interleaved)."""
    n = np.arange(cap)
    scale = {0: 1.0, 1: 150.0, 2: 1e-3, 3: 7.5}[fmt]
    x = scale * (12.0 * (rng.standard_normal(cap) + 1j * rng.standard_normal(cap)) + 70.0 * np.exp(2j * np.pi * tone_hz / fs * n + 0.3j))
    raw = np.empty(2 * cap)
    raw[0::2], raw[1::2] = x.real + 0.25 * scale, x.imag
    dt = NP_OF_FMT[fmt]
    if fmt in (0, 1):
        info = np.iinfo(dt)
        return np.clip(np.rint(raw), info.min, info.max).astype(dt)
    return raw.astype(dt)


def same_raw_fields(got, want):
    """Every field of the C struct equal, doubles by ==; NaN equal to NaN (the min / max of a window with no finite sample)."""
    g, w = got.raw(), want.raw()
    for name in g:
        a, b = np.atleast_1d(np.array(g[name], dtype=np.float64)), np.atleast_1d(np.array(w[name], dtype=np.float64))
        if not np.array_equal(a, b, equal_nan=True):
            return False
    return True
