"""Packed 1-, 2- and 4-bit I,Q samples: the format of include/sydr_amd.h (`sdr_iq_packing`) in NumPy.

A packing is `bits` per component, a field order and a table of `1 << bits` int8 levels.  A byte holds `8 // bits`
fields; the components of a slab follow one another I0, Q0, I1, Q1, ... field by field, the first field of a byte in its
least significant bits (or its most significant ones with `msb_first`); a field's code indexes the table.  The engine
widens such slabs on the device (`Engine.iq_upload_packed*`); `unpack` here is the statement it is tested against, `pack` /
`quantise` make packed streams (tests, tools/pack_recording.py).
"""
from __future__ import annotations

import numpy as np

DEFAULT_LEVELS = {
    1: (1, -1),                                          # the sign bit
    2: (1, 3, -1, -3),                                   # sign / magnitude: bit 1 the sign, bit 0 the magnitude
    4: (0, 1, 2, 3, 4, 5, 6, 7, -8, -7, -6, -5, -4, -3, -2, -1),   # two's complement
}


class Packing:
    def __init__(self, bits: int, levels=None, msb_first: bool = False):
        bits = int(bits)
        if bits not in (1, 2, 4):
            raise ValueError(f"packed samples have 1, 2 or 4 bits per component, not {bits}")
        levels = DEFAULT_LEVELS[bits] if levels is None else tuple(int(v) for v in levels)
        if len(levels) != 1 << bits:
            raise ValueError(f"{bits}-bit samples need {1 << bits} levels, {len(levels)} given")
        if any(not -128 <= v <= 127 for v in levels):
            raise ValueError("levels are int8")
        self.bits = bits
        self.levels = np.array(levels, dtype=np.int8)
        self.levels.setflags(write=False)                # (the engine keeps the C image of a packing: a packing does not change)
        self.msb_first = bool(msb_first)
        self.fields_per_byte = 8 // bits
        self.samples_per_byte = 4 // bits

    def __eq__(self, other):
        return (isinstance(other, Packing) and self.bits == other.bits and self.msb_first == other.msb_first
                and np.array_equal(self.levels, other.levels))

    def __hash__(self):
        return hash((self.bits, self.msb_first, self.levels.tobytes()))

    def __repr__(self):
        return f"Packing({self.bits}, {tuple(int(v) for v in self.levels)}, msb_first={self.msb_first})"

    def _shifts(self) -> np.ndarray:
        """Bit position of the field at each position of a byte."""
        p = np.arange(self.fields_per_byte)
        return (self.bits * (self.fields_per_byte - 1 - p if self.msb_first else p)).astype(np.uint8)


def packed_bytes(packing: Packing, n_samples: int) -> int:
    """Bytes `n_samples` I,Q samples occupy packed."""
    n_samples = int(n_samples)
    if n_samples < 0 or n_samples % packing.samples_per_byte:
        raise ValueError(f"a {packing.bits}-bit slab holds a multiple of {packing.samples_per_byte} samples, not {n_samples}")
    return n_samples // packing.samples_per_byte


def unpack(packed, packing: Packing, n_samples: int | None = None) -> np.ndarray:
    """Packed bytes -> interleaved int8 [I0, Q0, I1, Q1, ...] (2 * n_samples values; all the bytes hold by default)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1)
    if n_samples is not None:
        need = packed_bytes(packing, n_samples)
        if packed.size < need:
            raise ValueError(f"{n_samples} samples need {need} packed bytes, {packed.size} given")
        packed = packed[:need]
    codes = (packed[:, None] >> packing._shifts()[None, :]) & np.uint8((1 << packing.bits) - 1)
    return packing.levels[codes.reshape(-1)]


def pack(values, packing: Packing) -> np.ndarray:
    """Interleaved int8 [I0, Q0, ...], every value one of the packing's levels -> packed bytes."""
    values = np.ascontiguousarray(values, dtype=np.int8).reshape(-1)
    if values.size % packing.fields_per_byte or values.size % 2:
        raise ValueError(f"{values.size} components are not whole samples in whole bytes of {packing.fields_per_byte} fields")
    if len(set(packing.levels.tolist())) != packing.levels.size:
        raise ValueError("a table with repeated levels unpacks but cannot pack: a value has several codes")
    code_of = np.full(256, -1, dtype=np.int16)
    code_of[packing.levels.view(np.uint8)] = np.arange(packing.levels.size)
    codes = code_of[values.view(np.uint8)]
    if (codes < 0).any():
        raise ValueError(f"value {int(values[np.argmax(codes < 0)])} is none of the packing's levels")
    fields = codes.astype(np.uint8).reshape(-1, packing.fields_per_byte) << packing._shifts()[None, :]
    return np.bitwise_or.reduce(fields, axis=1).astype(np.uint8)


def quantise(raw, bits: int, threshold: float = 1.0, packing: Packing | None = None) -> np.ndarray:
    """Interleaved integer samples -> int8 of a few levels, the values of `packing` (the default table of `bits` otherwise).
    The levels, sorted, label the bins of a uniform quantiser of step `threshold` whose boundaries are symmetric around zero
    (bin k of n is [(k - n/2) * threshold, (k + 1 - n/2) * threshold), the outer ones open-ended); the LEVELS need not be:
    the 4-bit default table names the bin [v * threshold, (v + 1) * threshold) v, half a step below its middle, so the unpacked
    stream carries an offset of -threshold / 2 (nothing to a correlator behind a carrier wipe-off).
    1 bit is the sign (zero counts as positive); 2 bits with the default table give +-1 below the threshold in magnitude and
    +-3 above it."""
    packing = Packing(bits) if packing is None else packing
    if packing.bits != int(bits):
        raise ValueError("packing and bits disagree")
    if not threshold > 0:
        raise ValueError("threshold must be positive")
    levels = np.sort(packing.levels)
    n = levels.size
    x = np.asarray(raw, dtype=np.float64).reshape(-1)
    idx = np.clip(np.floor(x / float(threshold)) + n // 2, 0, n - 1).astype(np.intp)
    return levels[idx]


__all__ = ["DEFAULT_LEVELS", "Packing", "pack", "packed_bytes", "quantise", "unpack"]
