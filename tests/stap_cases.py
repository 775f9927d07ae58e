"""Shared weights, cuts and the end-to-end recording of the space-time (STAP) tests (test_stap.py, test_gpu_stap.py).

Streams, geometries, converter shapes, frequency words and gains are array_cases' (a few thousand frames: several tiles of
every shape used here).  What is added: [T][K] weights, cuts whose pushes are shorter than the tap span, and a two-element
recording with two partial-band jammers that spatial weights cannot remove and five taps per element can."""
from functools import lru_cache

import numpy as np

import array_cases as acases

from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import stap

SEED = 20260021


def general_weights(T: int, K: int, seed: int = 0) -> np.ndarray:
    """[T][K] complex weights of about unit size over all, whose products with the samples are inexact."""
    rng = np.random.default_rng(SEED + 101 * K + 13 * T + seed)
    return (rng.uniform(-1.0, 1.0, (T, K)) + 1j * rng.uniform(-1.0, 1.0, (T, K))) / np.sqrt(K * T)


def geometry(lanes, T: int, weights=None, measure: bool = False) -> stap.SpaceTimeGeometry:
    return stap.SpaceTimeGeometry(lanes, T, weights, measure)


def delayed(raw, layout: dc.InputLayout, t0: int, n: int) -> np.ndarray:
    """The first n frames of the stream with t0 zero frames prepended (INT8 / INT16 / FLOAT32 fields: a zero field is the number 0)."""
    assert layout.field != dc.FIELD_PACKED
    out = np.concatenate([np.zeros(t0 * layout.stride, dtype=raw.dtype), raw])[:n * layout.stride]
    return np.ascontiguousarray(out)


def x_max(cfg, raw) -> float:
    """max |x_j| of the combined inputs of one push of the whole stream."""
    re, im = stap.Statement(cfg).combined(raw)
    return float(np.max(np.hypot(re, im)))


# ------------------------------------------------------------------------------------------------ two partial-band jammers, two elements
E2E_FS, E2E_MS, E2E_PRN = acases.E2E_FS, acases.E2E_MS, acases.E2E_PRN
E2E_SAT = acases.E2E_SAT
E2E_SIGNAL_AMP, E2E_NOISE, E2E_JAMMER = acases.E2E_SIGNAL_AMP, acases.E2E_NOISE, acases.E2E_JAMMER
E2E_SIGNAL_U = -0.1
E2E_JAMMERS = ((-0.9e6, 0.5e6, 0.6), (0.7e6, 0.5e6, -0.5))          # (centre [Hz], width [Hz], u): element phase exp(i pi a u)
E2E_LAYOUT = dc.InputLayout(dc.FIELD_INT16, 0, 4, 0, True)
E2E_LANES = (0, 2)
E2E_TRAIN_MS = 2
E2E_TAPS = 5
E2E_SEARCH_MS = 3                                                    # the oracle searches the fourth millisecond


def band_noise(rng, n: int, fs: float, centre: float, width: float, sigma: float) -> np.ndarray:
    """Complex Gaussian noise confined to centre +- width / 2 (a brick wall over the FFT of the whole record), of power sigma^2."""
    white = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    f = np.fft.fftfreq(n, 1.0 / fs)
    x = np.fft.ifft(np.where(np.abs(f - centre) <= 0.5 * width, white, 0.0))
    return x * (sigma / np.sqrt(np.mean(np.abs(x) ** 2)))


@lru_cache(maxsize=None)
def two_jammers(ms: int = E2E_MS) -> np.ndarray:
    """A 2-element int16 recording at 4 MHz, array_cases.jammed_recording's recipe cut to two elements: one GPS PRN from
    u = E2E_SIGNAL_U, independent noise per element, and the two band-limited Gaussian jammers of E2E_JAMMERS, each 20 dB above
    the per-element noise.  Frames of 4 int16 fields: I, Q of element 0, of element 1; read-only."""
    from oracle import sydr_oracle as orc
    n = ms * int(E2E_FS * 1e-3)
    clean = orc.iq_to_complex(orc.synth_iq(E2E_FS, n, [dict(E2E_SAT, amp=1000.0)], 0.0, SEED + 70, dtype=np.int16).astype(np.float64)) / 1000.0
    rng = np.random.default_rng(SEED + 71)
    jams = [band_noise(rng, n, E2E_FS, centre, width, E2E_JAMMER) for centre, width, _ in E2E_JAMMERS]
    out = np.empty((n, 4), dtype=np.int16)
    for a in range(2):
        noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (E2E_NOISE / np.sqrt(2.0))
        s = E2E_SIGNAL_AMP * np.exp(1j * np.pi * a * E2E_SIGNAL_U) * clean + noise
        for jam, (_, _, u) in zip(jams, E2E_JAMMERS):
            s = s + np.exp(1j * np.pi * a * u) * jam
        out[:, 2 * a], out[:, 2 * a + 1] = np.clip(np.rint(s.real), -32767, 32767), np.clip(np.rint(s.imag), -32767, 32767)
    out = out.reshape(-1)
    out.setflags(write=False)
    return out


def e2e_config(T: int, weights=None, measure: bool = False) -> dc.DownConverterConfig:
    """The converter of e2e_conf: no mixer, no filter, gain 1 / 8; T taps per element."""
    return dc.DownConverterConfig(dc.IN_R8, 1, np.ones(1), 0, 1.0 / 8.0, 1, E2E_LAYOUT, geometry(E2E_LANES, T, weights, measure))


def e2e_training(T: int):
    """(C, n) of the first E2E_TRAIN_MS of the recording, by the statement."""
    st = stap.Statement(e2e_config(T, None, True))
    st.push(acases.piece(two_jammers(), E2E_LAYOUT, 0, E2E_TRAIN_MS * int(E2E_FS * 1e-3)))
    return st.read_covariance()


def e2e_search(x):
    """The oracle's PCPS and two_peak_compare on the fourth millisecond of the complex stream x -> ([bin, sample], ratio)."""
    from oracle import sydr_oracle as orc
    n = orc.samples_per_code(E2E_FS)
    spectrum = orc.code_spectrum(orc.gold_code(E2E_PRN), E2E_FS)
    cmap = orc.pcps_map(x[E2E_SEARCH_MS * n:(E2E_SEARCH_MS + 1) * n].reshape(1, -1), 0.0, E2E_FS, spectrum, 5000.0, 250.0, n)
    return orc.two_peak_compare(cmap, n, round(E2E_FS / orc.CODE_RATE))


def e2e_conf(path, **more):
    """[RFSIGNAL] of that recording: no mixer, no filter (decimation 1, one tap), gain 1 / 8 into a ci16 ring; element 0 alone
    unless `more` says otherwise (None removes a key)."""
    conf = dict(filepath=str(path), sampling_frequency=E2E_FS, is_complex="true", intermediate_frequency=0.0, data_size=16,
                decimation=1, filter_taps=1, output_gain=1.0 / 8.0, sample_format="int", frame_fields=4, array_lanes="0, 2")
    conf.update(more)
    return {k: v for k, v in conf.items() if v is not None}
