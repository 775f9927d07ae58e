"""Shared streams, layouts and converter settings of the input-layout tests (test_ddc_layout.py, test_gpu_ddc_layout.py).

Every stream is seeded and N_FRAMES frames long; packed streams are random bytes, that is codes uniform over the table.  The
converter shapes, taps, frequency words and gains are those of the converter's and the resampler's own tests
(downconvert_cases.py, resample_cases.py).  The yardstick of a layout is the OLD-format converter on the host-decoded stream
(`decoded`, `old_config`): the same arithmetic on the same doubles, so every comparison demands equal ring bytes."""
from functools import lru_cache

import numpy as np

import downconvert_cases as dcases
import resample_cases as rcases

from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import packing as pk

SEED = 20260019
N_FRAMES = 20000
FCWS = dcases.FCWS
CONVERTER_SHAPES = [(1, 1), (33, 2), (512, 16)]                 # (T, D)
RESAMPLER_SHAPES = [(3, 2, 7), (250, 341, 1500)]               # (L, M, T)
SHAPES = CONVERTER_SHAPES + RESAMPLER_SHAPES
ODD_TABLE = (-7, 2, 5, -128)                                    # a non-default 2-bit table, asymmetric, with -128


def shape_id(s) -> str:
    return f"T{s[0]}_D{s[1]}" if len(s) == 2 else rcases.shape_id(s)


def phase_taps(shape) -> int:
    """Tp: one more than the history holds."""
    return shape[0] if len(shape) == 2 else -(-shape[2] // shape[0])


def config(shape, fcw: int, gain: float, in_fmt: int = dc.IN_R8, layout=None) -> dc.DownConverterConfig:
    if len(shape) == 2:
        T, D = shape
        return dc.DownConverterConfig(in_fmt, D, dcases.taps_for(T, D), fcw, gain, 1, layout)
    L, M, T = shape
    return dc.DownConverterConfig(in_fmt, M, rcases.taps_for(L, M, T), fcw, gain, L, layout)


def out_total(shape, n_in: int) -> int:
    return dc.out_count(0, n_in, shape[1], 1 if len(shape) == 2 else shape[0])


def packed_layout(bits, complex=False, msb_first=False, levels=None, stride=None, lane=0, swap_iq=False) -> dc.InputLayout:
    return dc.InputLayout(dc.FIELD_PACKED, bits, stride, lane, complex, swap_iq, msb_first, levels)


@lru_cache(maxsize=None)
def stream(layout: dc.InputLayout, n: int = N_FRAMES, seed: int = SEED) -> np.ndarray:
    """The bytes of n frames of the layout, in the array type a push takes; read-only.  Packed: random bytes; int8 / int16:
    uniform over +-127 / +-3000; float32: the same integers as int16 would hold (`fractional` makes the others)."""
    rng = np.random.default_rng(seed + 31 * layout.field + layout.bits + 7 * layout.stride)
    n_fields = n * layout.stride
    if layout.field == dc.FIELD_PACKED:
        raw = rng.integers(0, 256, layout.bytes_for(n)).astype(np.uint8)
    elif layout.field == dc.FIELD_INT8:
        raw = rng.integers(-127, 128, n_fields).astype(np.int8)
    else:
        raw = rng.integers(-3000, 3001, n_fields).astype(layout.dtype)
    raw.setflags(write=False)
    return raw


@lru_cache(maxsize=None)
def fractional(complex: bool, n: int = N_FRAMES, seed: int = SEED) -> np.ndarray:
    """float32 uniform in +-1, interleaved when complex; read-only."""
    rng = np.random.default_rng(seed + 99)
    raw = rng.uniform(-1.0, 1.0, (2 if complex else 1) * n).astype(np.float32)
    raw.setflags(write=False)
    return raw


def old_format(layout: dc.InputLayout) -> int:
    """The old input format that holds the layout's decoded stream (float32: integers within int16)."""
    wide = layout.field in (dc.FIELD_INT16, dc.FIELD_FLOAT32)
    return {(False, False): dc.IN_R8, (True, False): dc.IN_R16, (False, True): dc.IN_CI8, (True, True): dc.IN_CI16}[(wide, layout.complex)]


def decoded(raw, layout: dc.InputLayout) -> np.ndarray:
    """The stream of `raw` as the old format holds it: the decoded integers, I,Q interleaved when complex."""
    xr, xi = dc.decode(raw, layout)
    dtype = dc.input_dtype(old_format(layout))
    if not layout.complex:
        out = xr.astype(dtype)
        assert np.array_equal(out.astype(np.float64), xr)
        return out
    out = np.empty(2 * xr.size, dtype=dtype)
    out[0::2], out[1::2] = xr, xi
    assert np.array_equal(out[0::2].astype(np.float64), xr) and np.array_equal(out[1::2].astype(np.float64), xi)
    return out


def gain_for(layout: dc.InputLayout, ring_fmt: int) -> float:
    return dcases.gain_for(old_format(layout), ring_fmt)


def ring_capacity(n_out: int) -> int:
    return -(-(n_out + 8) // 8) * 8


def push_all(engine, cfg, raw, n_out: int, offset: int = 0) -> np.ndarray:
    """A fresh converter of cfg, `raw` in one push at `offset` -> the window the push wrote, downloaded."""
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_out_count(ddc, cfg_frames(cfg, raw)) == n_out
        assert engine.ddc_push(ddc, raw, offset) == n_out
    finally:
        engine.ddc_destroy(ddc)
    return engine.iq_download(n_out, offset)


def cfg_frames(cfg, raw) -> int:
    if cfg.layout is not None:
        return cfg.layout.frames_in(raw.nbytes)
    return raw.size // (2 if dc.input_is_complex(cfg.in_fmt) else 1)


def rounded_lengths(Tp: int, group: int) -> list:
    """The converter tests' push lengths, each rounded up to whole bytes (a multiple of `group` frames); zero stays zero."""
    return [-(-n // group) * group for n in dcases.push_lengths(Tp)]


def cut_bytes(raw: np.ndarray, layout: dc.InputLayout, lengths) -> list:
    """`raw` cut into pushes of the given lengths in frames (whole bytes each), then the rest."""
    per = np.dtype(layout.dtype).itemsize
    out, at = [], 0
    for n in lengths:
        step = layout.bytes_for(n) // per
        out.append(raw[at:at + step])
        at += step
    out.append(raw[at:])
    return out


# ------------------------------------------------------------------------------------------------ a packed real IF recording
QUANT_BITS, QUANT_THRESHOLD, PACKED_GAIN = 2, 20.0, 16.0


@lru_cache(maxsize=None)
def packed_real_recording(ms: int = dcases.REAL_MS):
    """downconvert_cases.real_if_recording() quantised to 2 bits (threshold 20) and packed, four samples to a byte.
    -> (the packed bytes, the few-level int8 samples); read-only."""
    few = pk.quantise(dcases.real_if_recording(ms), QUANT_BITS, QUANT_THRESHOLD)
    packed = pk.pack(few, pk.Packing(QUANT_BITS))                # (field by field: every field one real sample)
    packed.setflags(write=False)
    few.setflags(write=False)
    return packed, few


def packed_real_conf(path, **more):
    return dcases.real_signal_conf(path, data_size=QUANT_BITS, sample_format="packed", output_gain=PACKED_GAIN, **more)


def write_packed_and_converted(tmp_path, ms: int = dcases.REAL_MS):
    """-> (RFSignal over the packed real file, RFSignal over the statement's ci8 output stored as an ordinary complex int8 file,
    that output as int8 I,Q)"""
    from sydr_amd.signal.iqsource import RFSignal
    packed, few = packed_real_recording(ms)
    packed_path, conv_path = tmp_path / "real_if_2bit.bin", tmp_path / "converted_ci8.bin"
    packed.tofile(packed_path)
    sig = RFSignal(packed_real_conf(packed_path))
    converted = dc.statement(sig.frontEnd.config, [packed], dc.FMT_CI8)
    converted.tofile(conv_path)
    return sig, RFSignal(dcases.converted_signal_conf(conv_path)), converted
