"""Shared streams, geometries and converter settings of the antenna-array tests (test_array.py, test_gpu_array.py).

Every stream is ddc_layout_cases.stream of the array's layout (seeded; packed streams are random bytes), N_FRAMES frames long:
a few thousand frames are several tiles of every shape used here.  Geometries have K = 2, 3 and 8 elements with lanes out of
order and not adjacent, on real and on complex layouts.  Converter shapes, taps, frequency words and gains are those of the
converter's own tests.  Where an existing code path computes the same thing -- a unit weight against the layout's converter, weights
in {+-1, +-i} against IN_CI16 on the host-combined integers, a packed array against the INT8 array on the unpacked bytes -- the
comparison demands equal ring bytes."""
from functools import lru_cache

import numpy as np

import downconvert_cases as dcases
import ddc_layout_cases as lcases

from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc

SEED = 20260020
N_FRAMES = 3000
FCWS = dcases.FCWS
SHAPES = [(1, 1), (33, 2), (3, 2, 7)]                           # (T, D) and (L, M, T): ddc_layout_cases.FRAME_SHAPES
FILTERED = [(33, 2), (3, 2, 7)]                                 # D > 1 and T > 1; a resampler (L > 1)
QUARTER = (1.0, -1.0, 1j, -1j)

# name -> (layout, lanes)
GEOMETRIES = {
    "K2_int8_real": (dc.InputLayout(dc.FIELD_INT8, 0, 4), (3, 0)),
    "K3_int8_complex": (dc.InputLayout(dc.FIELD_INT8, 0, 8, 0, True), (5, 0, 2)),
    "K3_int16_complex_swapped": (dc.InputLayout(dc.FIELD_INT16, 0, 7, 0, True, True), (4, 0, 2)),
    "K8_int8_real": (dc.InputLayout(dc.FIELD_INT8, 0, 11), (10, 0, 7, 2, 5, 3, 8, 1)),
    "K8_int8_complex": (dc.InputLayout(dc.FIELD_INT8, 0, 17, 0, True), (15, 0, 4, 2, 8, 6, 12, 10)),
}
INT8_GEOMETRIES = ["K2_int8_real", "K3_int8_complex", "K8_int8_real", "K8_int8_complex"]

# packed arrays: 1, 2 and 4 bits; a 6-bit frame (K = 3 complex 1-bit); frames that are whole bytes, frames that straddle them, and a
# frame wider than the 64-bit window the decode loads once per input (17 fields of 4 bits)
PACKED = {
    "K3_1bit_complex_6bit_frame": (1, 6, True, (4, 0, 2)),
    "K4_2bit_complex": (2, 8, True, (6, 0, 4, 2)),
    "K2_2bit_real_odd_table": (2, 3, False, (2, 0)),
    "K2_4bit_complex_20bit_frame": (4, 5, True, (3, 0)),
    "K8_4bit_complex_68bit_frame": (4, 17, True, (15, 0, 4, 2, 8, 6, 12, 10)),
}


def packed_layout(name: str, msb_first: bool) -> dc.InputLayout:
    bits, stride, cplx, _ = PACKED[name]
    return dc.InputLayout(dc.FIELD_PACKED, bits, stride, 0, cplx, False, msb_first, lcases.ODD_TABLE if "odd_table" in name else None)


def unpacked(raw, layout: dc.InputLayout):
    """-> (every field of the packed bytes as int8, the INT8 layout of the same frames)"""
    plain = np.ascontiguousarray(dc.fields(raw, layout)[:layout.frames_in(raw.nbytes) * layout.stride])
    return plain, dc.InputLayout(dc.FIELD_INT8, 0, layout.stride, 0, layout.complex, layout.swap_iq)


def stream(layout: dc.InputLayout, n: int = N_FRAMES) -> np.ndarray:
    return lcases.stream(layout, n, SEED)


def frames(n: int, layout: dc.InputLayout) -> int:
    """n rounded up to whole bytes of the layout."""
    g = layout.frame_group
    return -(-n // g) * g


def quarter_weights(K: int, turn: int = 0) -> np.ndarray:
    """Weights in {1, -1, i, -i}, all four where K allows."""
    return np.array([QUARTER[(a + turn) % 4] for a in range(K)], dtype=np.complex128)


def general_weights(K: int, seed: int = 0) -> np.ndarray:
    """Complex weights of about unit size whose products with the samples are inexact."""
    rng = np.random.default_rng(SEED + 101 * K + seed)
    return (rng.uniform(-1.0, 1.0, K) + 1j * rng.uniform(-1.0, 1.0, K)) / np.sqrt(K)


def combined_integers(raw, layout: dc.InputLayout, lanes, weights) -> np.ndarray:
    """x = sum_a conj(w_a) s_a of integer elements with weights in {+-1, +-i}, in INTEGER arithmetic, as an IN_CI16 stream
    (I, Q interleaved)."""
    sr, si = ar.elements(raw, layout, lanes)
    sr, si = sr.astype(np.int64), si.astype(np.int64)
    re, im = np.zeros(sr.shape[1], dtype=np.int64), np.zeros(sr.shape[1], dtype=np.int64)
    for a, w in enumerate(weights):
        if w == 1:
            re, im = re + sr[a], im + si[a]
        elif w == -1:
            re, im = re - sr[a], im - si[a]
        elif w == 1j:                       # conj(i) s = -i (sr + i si) = si - i sr
            re, im = re + si[a], im - sr[a]
        else:
            assert w == -1j
            re, im = re - si[a], im + sr[a]
    out = np.empty(2 * re.size, dtype=np.int16)
    out[0::2], out[1::2] = re, im
    assert np.array_equal(out[0::2], re) and np.array_equal(out[1::2], im)
    return out


def config(shape, fcw: int, gain: float, layout=None, array=None, in_fmt: int = dc.IN_CI16) -> dc.DownConverterConfig:
    cfg = lcases.config(shape, fcw, gain, in_fmt, layout)
    if array is not None:
        cfg = dc.DownConverterConfig(cfg.in_fmt, cfg.decimation, cfg.taps, cfg.fcw, cfg.gain, cfg.interpolation, layout, array)
    return cfg


def gain_for(layout: dc.InputLayout, ring_fmt: int, K: int) -> float:
    """The converter tests' irrational gain for the layout's width, over sqrt(K) for the sum of K elements."""
    return lcases.gain_for(layout, ring_fmt) / np.sqrt(K)


def x_max(cfg, raw, weights=None) -> float:
    """max |x_j| of the combined inputs."""
    sr, si = ar.elements(raw, cfg.layout, cfg.array.lanes)
    re, im = ar.combine(sr, si, cfg.array.weights if weights is None else weights)
    return float(np.max(np.hypot(re, im)))


def cut_with_marks(lengths, marks, total: int, group: int = 1):
    """Push lengths (frames) that follow `lengths`, then the rest of `total`, split so that every mark is a push boundary; every
    length a multiple of `group`.  -> [(first frame, frames)]"""
    out, at = [], 0
    pending = sorted(marks)
    todo = list(lengths) + [None]
    while todo:
        n = todo.pop(0)
        n = total - at if n is None else min(-(-n // group) * group, total - at)
        while pending and at < pending[0] < at + n:
            out.append((at, pending[0] - at))
            n -= pending[0] - at
            at = pending.pop(0)
        if pending and pending[0] == at + n:
            pending.pop(0)
        out.append((at, n))
        at += n
    assert at == total and all(m % group == 0 for m in marks)
    return out


def piece(raw, layout: dc.InputLayout, first: int, n: int) -> np.ndarray:
    per = np.dtype(layout.dtype).itemsize
    return np.ascontiguousarray(raw[layout.bytes_for(first) // per:layout.bytes_for(first + n) // per])


# ------------------------------------------------------------------------------------------------ a jammed 4-element recording
E2E_FS, E2E_MS, E2E_PRN = 4e6, 8, 7
E2E_SAT = dict(prn=E2E_PRN, doppler=1750.0, code_phase=300.25, phase=0.1)
E2E_SIGNAL_AMP, E2E_NOISE, E2E_JAMMER = 60.0, 300.0, 3000.0
E2E_SIGNAL_DIRECTION = np.exp(2j * np.pi * np.array([0.0, 0.11, 0.37, 0.62]))
E2E_JAMMER_DIRECTION = np.exp(2j * np.pi * np.array([0.0, 0.41, 0.83, 0.19]))
E2E_LAYOUT = dc.InputLayout(dc.FIELD_INT16, 0, 8, 0, True)
E2E_LANES = (0, 2, 4, 6)
E2E_TRAIN_MS = 2


@lru_cache(maxsize=None)
def jammed_recording(ms: int = E2E_MS) -> np.ndarray:
    """A 4-element int16 recording at 4 MHz: one GPS PRN, the same waveform on all elements with the element phases of
    E2E_SIGNAL_DIRECTION; a broadband complex Gaussian jammer with those of E2E_JAMMER_DIRECTION, 20 dB above the per-element
    noise; independent noise per element.  Frames of 8 int16 fields: I, Q of element 0, of element 1, ...; read-only."""
    from oracle import sydr_oracle as orc
    n = ms * int(E2E_FS * 1e-3)
    clean = orc.iq_to_complex(orc.synth_iq(E2E_FS, n, [dict(E2E_SAT, amp=1000.0)], 0.0, SEED + 70, dtype=np.int16).astype(np.float64)) / 1000.0
    rng = np.random.default_rng(SEED + 71)
    jam = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (E2E_JAMMER / np.sqrt(2.0))
    out = np.empty((n, 8), dtype=np.int16)
    for a in range(4):
        noise = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * (E2E_NOISE / np.sqrt(2.0))
        s = E2E_SIGNAL_AMP * E2E_SIGNAL_DIRECTION[a] * clean + E2E_JAMMER_DIRECTION[a] * jam + noise
        out[:, 2 * a], out[:, 2 * a + 1] = np.clip(np.rint(s.real), -32767, 32767), np.clip(np.rint(s.imag), -32767, 32767)
    out = out.reshape(-1)
    out.setflags(write=False)
    return out


def e2e_conf(path, **more):
    """[RFSIGNAL] of that recording: no mixer, no filter (decimation 1, one tap), gain 1 / 8 into a ci16 ring; element 0 alone
    unless `more` says otherwise (None removes a key)."""
    conf = dict(filepath=str(path), sampling_frequency=E2E_FS, is_complex="true", intermediate_frequency=0.0, data_size=16,
                decimation=1, filter_taps=1, output_gain=1.0 / 8.0, sample_format="int", frame_fields=8, array_lanes="0, 2, 4, 6")
    conf.update(more)
    return {k: v for k, v in conf.items() if v is not None}
