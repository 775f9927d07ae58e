"""Shared cases of the beam tests (test_beams.py, test_gpu_beams.py): several weight sets of an array or space-time converter
over one push, each into its own ring (sdr_ddc_beam_attach).

Streams, geometries, converter shapes, frequency words and gains are array_cases' and stap_cases' (about 3000 frames: several
tiles of every shape used here).  What is added: weight sets per beam -- random complex ones and the unit vectors, alternating --,
ring formats mixed across the beams of one converter, and the sweep of test 1.  The yardstick of a beam is the parent's path: an
independent converter with that beam's weights on an engine of its own; every comparison demands equal ring bytes."""
import numpy as np

import array_cases as acases
import downconvert_cases as dcases
import stap_cases as scases

from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import stap

SEED = 20260022
N_FRAMES = acases.N_FRAMES
RINGS = dcases.RING_FORMATS
RATIONAL = (3, 4, 96)                       # (L, M, T): rational 3/4 with a 96-tap prototype, Tp = 32
FLOAT_LAYOUT = dc.InputLayout(dc.FIELD_FLOAT32, 0, 6, 0, True)          # (ddc_layout_cases.stream: float32 holding integers)
K4_INT8 = (dc.InputLayout(dc.FIELD_INT8, 0, 9, 0, True), (6, 0, 4, 2))

# name -> (layout, lanes, converter shape, taps per element (0: an array converter), beams R)
# K in {2, 3, 4, 8}; INT8, INT16, 2-bit PACKED complex, 1-bit PACKED with K = 3 (frames of 6 bits), FLOAT32 holding integers;
# (T, D) in {(1, 1), (33, 2)} and the rational 3/4; space-time T in {1, 3}; R in {2, 4, 16}
SWEEP = {
    "K2_int8_real_T1D1_R2": (*acases.GEOMETRIES["K2_int8_real"], (1, 1), 0, 2),
    "K3_int16_T33D2_R4": (*acases.GEOMETRIES["K3_int16_complex_swapped"], (33, 2), 0, 4),
    "K4_2bit_T33D2_R16": (acases.packed_layout("K4_2bit_complex", False), acases.PACKED["K4_2bit_complex"][3], (33, 2), 0, 16),
    "K3_1bit_rational_R4": (acases.packed_layout("K3_1bit_complex_6bit_frame", True), acases.PACKED["K3_1bit_complex_6bit_frame"][3], RATIONAL, 0, 4),
    "K8_int8_rational_R2": (*acases.GEOMETRIES["K8_int8_complex"], RATIONAL, 0, 2),
    "K8_int8_real_T33D2_R16": (*acases.GEOMETRIES["K8_int8_real"], (33, 2), 0, 16),
    "K3_float32_T1D1_R4": (FLOAT_LAYOUT, (4, 0, 2), (1, 1), 0, 4),
    "K4_int8_T33D2_R4": (*K4_INT8, (33, 2), 0, 4),
    "stap1_K2_int8_T33D2_R4": (*acases.GEOMETRIES["K2_int8_real"], (33, 2), 1, 4),
    "stap3_K3_int16_T1D1_R2": (*acases.GEOMETRIES["K3_int16_complex_swapped"], (1, 1), 3, 2),
    "stap3_K4_2bit_rational_R16": (acases.packed_layout("K4_2bit_complex", False), acases.PACKED["K4_2bit_complex"][3], RATIONAL, 3, 16),
    "stap3_K8_int8_T33D2_R4": (*acases.GEOMETRIES["K8_int8_complex"], (33, 2), 3, 4),
}


def is_stap(cfg) -> bool:
    return isinstance(cfg.array, stap.SpaceTimeGeometry)


def with_weights(cfg, w):
    return stap.with_weights(cfg, w) if is_stap(cfg) else ar.with_weights(cfg, w)


def beams_statement(cfg, weight_sets, pushes, ring_fmts=None, weights_at=None):
    return (stap if is_stap(cfg) else ar).beams_statement(cfg, weight_sets, pushes, ring_fmts, weights_at)


def general(K: int, T: int, seed: int) -> np.ndarray:
    """Random complex weights in the converter's shape, [K] or (T > 0) [T][K]."""
    return scases.general_weights(T, K, seed) if T else acases.general_weights(K, seed)


def unit(K: int, T: int, a: int) -> np.ndarray:
    return stap.unit_weights(T, K, a, 0) if T else ar.unit_weights(K, a)


def weight_sets(K: int, T: int, R: int, seed: int = 0):
    """R weight sets: random complex ones at the even beams, the unit vectors e_0, e_1, ... at the odd ones.
    -> (the sets, {beam: element} of the unit vectors)"""
    sets, units = [], {}
    for b in range(R):
        if b & 1:
            units[b] = (b >> 1) % K
            sets.append(unit(K, T, units[b]))
        else:
            sets.append(general(K, T, seed + b))
    return sets, units


def ring_formats(R: int, turn: int = 0):
    """All four ring formats, mixed across the beams of one converter."""
    return [RINGS[(b + turn) % len(RINGS)] for b in range(R)]


def config(name: str, fcw: int):
    """-> (cfg with beam 0's weights left at the geometry's default, the stream, K, T)"""
    layout, lanes, shape, T, _ = SWEEP[name]
    K = len(lanes)
    n = acases.frames(N_FRAMES, layout)
    raw = acases.stream(layout, n)
    geometry = scases.geometry(lanes, T) if T else ar.ArrayGeometry(lanes)
    # one gain for every beam (the same constructor arguments): the ci8 ring's, under which the wider rings still hold signal
    gain = dcases.GOLD * 4.0 if layout.field == dc.FIELD_PACKED else acases.gain_for(layout, dc.FMT_CI8, K)
    return acases.config(shape, fcw, gain, layout, geometry), raw, K, T


def fill(ring_fmt: int, capacity: int, seed: int = 0) -> np.ndarray:
    """A pattern for a whole ring of the format: small non-zero numbers, the same for the same (format, capacity, seed)."""
    rng = np.random.default_rng(SEED + 7 * ring_fmt + seed)
    return rng.integers(1, 100, 2 * capacity).astype({dc.FMT_CI8: np.int8, dc.FMT_CI16: np.int16, dc.FMT_CF32: np.float32, dc.FMT_CF64: np.float64}[ring_fmt])


def pieces(raw, layout, cut):
    """[(first frame, frames)] -> the pushes' byte arrays."""
    return [acases.piece(raw, layout, first, count) for first, count in cut]


def placed(ring_fmt: int, capacity: int, out: np.ndarray, offset: int, seed: int = 0) -> np.ndarray:
    """The whole ring a run leaves: `fill` with the quantised outputs `out` written from `offset` on, wrapping at the ring's end."""
    ring = fill(ring_fmt, capacity, seed)
    at = (2 * offset + np.arange(out.size)) % (2 * capacity)
    ring[at] = out
    return ring


# ------------------------------------------------------------------------------------------------ why the feature exists
E2E_CFG = dict(in_fmt=dc.IN_R8, decimation=1, taps=np.ones(1), fcw=0, gain=1.0 / 8.0, interpolation=1, layout=acases.E2E_LAYOUT)


def e2e_config(weights=None) -> dc.DownConverterConfig:
    """The converter of array_cases.e2e_conf: no mixer, no filter, gain 1 / 8 (into ci16 rings)."""
    return dc.DownConverterConfig(**E2E_CFG, array=ar.ArrayGeometry(acases.E2E_LANES, weights))


def jammed(seed: int = 0) -> np.ndarray:
    """array_cases.jammed_recording's recipe with the jammer's and the elements' noise drawn from another seed (0: that recording)."""
    if seed == 0:
        return acases.jammed_recording()
    from oracle import sydr_oracle as orc
    n = acases.E2E_MS * int(acases.E2E_FS * 1e-3)
    clean = orc.iq_to_complex(orc.synth_iq(acases.E2E_FS, n, [dict(acases.E2E_SAT, amp=1000.0)], 0.0, acases.SEED + 70, dtype=np.int16).astype(np.float64)) / 1000.0
    rng = np.random.default_rng(acases.SEED + 71 + 1000 * seed)
    jam = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (acases.E2E_JAMMER / np.sqrt(2.0))
    out = np.empty((n, 8), dtype=np.int16)
    for a in range(4):
        noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (acases.E2E_NOISE / np.sqrt(2.0))
        s = acases.E2E_SIGNAL_AMP * acases.E2E_SIGNAL_DIRECTION[a] * clean + acases.E2E_JAMMER_DIRECTION[a] * jam + noise
        out[:, 2 * a], out[:, 2 * a + 1] = np.clip(np.rint(s.real), -32767, 32767), np.clip(np.rint(s.imag), -32767, 32767)
    return out.reshape(-1)


def search(ring, ms: int = 0):
    """The oracle's PCPS and two_peak_compare on millisecond `ms` of an int16 ring -> ([bin, sample], ratio)"""
    from oracle import sydr_oracle as orc
    fs = acases.E2E_FS
    n = orc.samples_per_code(fs)
    x = orc.iq_to_complex(np.asarray(ring)[2 * ms * n:2 * (ms + 1) * n].astype(np.float64))
    cmap = orc.pcps_map(x.reshape(1, -1), 0.0, fs, orc.code_spectrum(orc.gold_code(acases.E2E_PRN), fs), 5000.0, 250.0, n)
    return orc.two_peak_compare(cmap, n, round(fs / orc.CODE_RATE))


def element_prompts(rings, first_sample: int, doppler: float, epochs: int):
    """The prompt of every ring over `epochs` code periods from first_sample on, at the carrier and code phase beam 0 tracked
    -> complex [rings][epochs] (the oracle's EPL, one millisecond each, every epoch's carrier phase starting at zero)."""
    from oracle import sydr_oracle as orc
    fs = acases.E2E_FS
    code, step, n_code = orc.pad_code(orc.gold_code(acases.E2E_PRN)), orc.CODE_RATE / fs, orc.samples_per_code(fs)
    m = orc.required_samples(0.0, step)
    out = np.zeros((len(rings), epochs), dtype=np.complex128)
    for a, ring in enumerate(rings):
        x = orc.iq_to_complex(np.asarray(ring).astype(np.float64))
        for k in range(epochs):
            s = first_sample + k * n_code
            r = orc.epl(x[s:s + m], code, fs, doppler, 0.0, 0.0, step, (0.0,))
            out[a, k] = r[0] + 1j * r[1]
    return out


def why(raw):
    """The whole chain on the CPU: power inversion on beam 0, the four element beams, their prompts at what beam 0 found, the
    Wiener weights, the search on the Wiener beam.  -> dict of ([bin, sample], ratio) for 'element', 'power_inversion', 'wiener',
    and the weights."""
    per_ms = int(acases.E2E_FS * 1e-3)
    R, n = ar.covariance(acases.piece(raw, acases.E2E_LAYOUT, 0, acases.E2E_TRAIN_MS * per_ms), acases.E2E_LAYOUT, acases.E2E_LANES)
    w_pi = ar.power_inversion(R, n)
    sets = [w_pi] + list(ar.element_weights(4))
    rings = ar.beams_statement(e2e_config(), sets, [raw], [dc.FMT_CI16] * 5)
    found = {"power_inversion": search(rings[0]), "element": search(rings[1])}
    first = found["power_inversion"][0][1] + 1
    prompts = element_prompts(rings, first, acases.E2E_SAT["doppler"], acases.E2E_MS - 2)
    # every epoch's unknown carrier phase and data bit is beam 0's own prompt's: taken out before the epochs are added
    p = np.sum(prompts[1:] * np.conj(prompts[0] / np.abs(prompts[0])), axis=1)
    whole_R, _ = ar.covariance(raw, acases.E2E_LAYOUT, acases.E2E_LANES)
    w = ar.wiener_weights(whole_R, p)
    w = w * np.sqrt(np.real(np.vdot(w_pi, whole_R @ w_pi)) / np.real(np.vdot(w, whole_R @ w)))      # (beam 0's output power: the same ci16 scale)
    found["wiener"] = search(ar.statement(e2e_config(w), [raw], dc.FMT_CI16))
    found["weights"] = dict(power_inversion=w_pi, wiener=w)
    return found
