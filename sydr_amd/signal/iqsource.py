"""IQ recording -> slabs for the device ring.

Reads the [RFSIGNAL] section of the reference's receiver.ini (keys `filepath`, `sampling_frequency`,
`is_complex`, `intermediate_frequency`, `data_size`; sydr/signal/rfsignal.py:13-54) and serves the file the way
the GPU wants it: the recording is memory-mapped and a slab is a zero-copy view of its native interleaved
integers (int8 / int16 I,Q -- 2 or 4 bytes per sample), which is byte for byte what the device ring stores.
Packed recordings (`data_size` 1, 2 or 4 bits per component, several samples to a byte: packing.py; optional keys
`sample_levels` -- comma-separated, `1 << data_size` integers -- and `bit_order` -- `lsb` / `msb`) are served as `uint8`
views of their packed bytes, which the engine widens on the device.
A recording at an intermediate frequency or at a wider band than the channels need -- real-valued ones included (`is_complex`
empty) -- goes through the device's down-converter (downconvert.py) when the key `decimation` is present (optional keys
`baseband_shift`, `filter_taps`, `filter_cutoff`, `output_gain`, `output_bits`): the front-end attributes the channels read
(`samplingFrequency`, `samplesPerMs`, `interFrequency`) are then the RING's, the slabs handed out are raw input, and
`frontEnd` says how the one becomes the other.  The optional key `interpolation` (L; only beside `decimation`, which is then
M) makes the converter a rational resampler: the ring's rate is `sampling_frequency * L / M` (16.368 MHz -> 12 MHz with 250 / 341),
the default filter comes from `design_resampler` and `filter_cutoff` is a fraction of the UP-SAMPLED rate.
Beside `decimation` the key `sample_format` describes recordings the four integer formats do not cover, as an input layout
(downconvert.py `InputLayout`) the converter's kernels decode where they load: `packed` (`data_size` 1, 2 or 4, with
`sample_levels` and `bit_order` as for packed recordings -- real or complex, at any intermediate frequency), `float` (`data_size`
32: float32 as GNU Radio writes it) or `int` (`data_size` 8 or 16); with it `frame_fields` (the fields of a frame: 2 if
`is_complex`, else 1, by default), `frame_lane` (the stream's first field in its frame, default 0) and `swap_iq` (1: pairs are
stored Q before I) pick one stream out of a file that interleaves several.  Such a recording's slabs are whole-byte views of
its bytes, counted in frames.
Beside `sample_format` the key `array_lanes` (a comma list of K = 2..8 lanes: each element's first field in the frame; `frame_lane`
is then not read) makes the recording a multi-antenna one whose elements the converter combines, x = w^H s, where it decodes the
frame (array.py): `array_mode` is `fixed` (the default; `array_weights`, K re,im pairs, default 1 on `array_reference`),
`power_inversion` or `mvdr` (`array_steering`, K re,im pairs); `array_reference` (default 0), `array_loading` (default 1e-3)
and `array_train_ms` (default 2) belong to the two adaptive modes, in which the receiver first pushes the recording's first
`array_train_ms` milliseconds with unit weight on the reference element, reads the covariance, solves for the weights, sets
them, resets the converter and begins the recording again from its first sample: the whole ring is made with one weight
vector.  `array_taps` (T = 1..8, default 1: everything above as it is) gives every element a T-tap FIR (stap.py): `array_weights` is
then T K pairs, tap by tap, an adaptive mode measures the lag covariance and solves on the K T x K T space-time matrix, and
`array_reference_tap` (default (T - 1) // 2) is the tap at which the reference element (or the steering vector) passes -- the
output is delayed by that many input samples (`ArrayPlan.delay`).  Mitigation keys beside array keys are refused.
Such a recording may also ask for interference mitigation between the converter and the ring (mitigate.py; keys
`blanking_factor` with `blanking_lead`, `blanking_hold`, and `excision_nfft` with `excision_margin_db`; `calibration_ms`):
the blanker's level and the excisor's limits are measured once, on the host, over the converter's output of the recording's
first `calibration_ms` milliseconds.  `decimation = 1` with `filter_taps = 1` is the identity converter for a plain complex
recording.
The reference instead reads 120 ms chunks and inflates every sample to complex128 (16 bytes) before anything
else touches it (rfsignal.py:58-132).  Only what the hot path's callers use is kept of that class's surface:
the front-end attributes, `getMilliseconds`, and `readFile` / `readFileBySamples` / `closeFile` /
`getCurrentSampleIndex` (rfsignal.py:92-204) as views of the mapped file with the reference's cursor semantics.
"""
from __future__ import annotations

import os

import numpy as np

from .packing import Packing, unpack


LAYOUT_KEYS = ("sample_format", "frame_fields", "frame_lane", "swap_iq")
ARRAY_KEYS = ("array_lanes", "array_mode", "array_weights", "array_steering", "array_reference", "array_loading", "array_train_ms", "array_taps",
              "array_reference_tap")
MITIGATION_KEYS = ("blanking_factor", "blanking_lead", "blanking_hold", "excision_nfft", "excision_margin_db", "calibration_ms")


class FrontEnd:
    """How a recording's raw input becomes the ring's samples: the down-converter's settings (downconvert.py), its group delay in
    INPUT samples -- common to all channels; reported, not compensated --, the ring's sample width and the shift in Hz."""

    def __init__(self, config, output_bits: int, shift_hz: float, calibrate=None, array=None):
        self.config = config
        self.array = array                              # ArrayPlan of a multi-antenna recording (`array_lanes`), else None
        self.decimation = config.decimation
        self.interpolation = config.interpolation
        self.groupDelay = config.group_delay
        self.outputBits = int(output_bits)
        self.shift = float(shift_hz)
        self._calibrate = calibrate                     # () -> mitigate.MitigationConfig, run when first asked for
        self._mitigation = None

    @property
    def mitigation(self):
        """The pulse blanker's and excisor's settings (mitigate.MitigationConfig) or None: measured on the recording's
        first milliseconds when first asked for, then kept."""
        if self._calibrate is not None:
            self._mitigation, self._calibrate = self._calibrate(), None
        return self._mitigation

    @property
    def delay(self) -> int:
        """The mitigator's delay in RING samples -- common to all channels; reported, not compensated."""
        m = self.mitigation
        return m.delay if m is not None else 0


class ArrayPlan:
    """How the weights of a multi-antenna recording come about: `fixed` (those of the configuration) or, measured on the
    recording's first `train_ms` milliseconds, `power_inversion` / `mvdr` (array.py)."""

    def __init__(self, mode: str, reference: int, loading: float, train_ms: int, steering=None, taps: int = 1, reference_tap: int = 0):
        self.mode, self.reference, self.loading, self.train_ms, self.steering = mode, reference, loading, train_ms, steering
        self.taps, self.reference_tap = taps, reference_tap          # `array_taps` > 1: space-time weights (stap.py)

    @property
    def delay(self) -> int:
        """The reference tap's delay in INPUT samples -- common to all channels; reported, not compensated."""
        return self.reference_tap if self.taps > 1 else 0

    @property
    def adaptive(self) -> bool:
        return self.mode != "fixed"

    def solve(self, R, n):
        """The weights for the covariance R of n inputs."""
        from . import array as ar
        if self.taps > 1:                 # R is the lag covariance C [T][K][K]; the weights are [T][K]
            from . import stap
            if self.mode == "power_inversion":
                return stap.power_inversion(R, n, self.reference, self.reference_tap, self.loading)
            if self.mode == "mvdr":
                return stap.mvdr(R, n, self.steering, self.reference_tap, self.loading)
            raise ValueError("fixed weights are not solved for")
        if self.mode == "power_inversion":
            return ar.power_inversion(R, n, self.reference, self.loading)
        if self.mode == "mvdr":
            return ar.mvdr(R, n, self.steering, self.loading)
        raise ValueError("fixed weights are not solved for")


class RFSignal:
    def __init__(self, configuration):
        self.filepath = str(configuration["filepath"])
        self.samplingFrequency = float(configuration["sampling_frequency"])
        self.interFrequency = float(configuration["intermediate_frequency"])
        # rfsignal.py:35: bool(<ini string>) -- ANY non-empty string is True there ("false" included); mirrored as is
        self.isComplex = bool(configuration["is_complex"])
        bits = int(configuration["data_size"])
        sample_format = str(configuration["sample_format"]).strip().lower() if "sample_format" in configuration else None
        if bits not in (1, 2, 4, 8, 16) and not (sample_format == "float" and bits == 32):
            raise ValueError(f"Data type of {bits} bit(s) is not valid.")
        self.layout = None                              # recordings with `sample_format`: downconvert.InputLayout
        self.packing = None                             # packed recordings: how the bytes hold the samples (packing.py)
        if bits < 8:
            levels = None
            if "sample_levels" in configuration:
                levels = [int(v) for v in str(configuration["sample_levels"]).split(",")]
            order = str(configuration["bit_order"]).strip().lower() if "bit_order" in configuration else "lsb"
            if order not in ("lsb", "msb"):
                raise ValueError(f"bit_order is 'lsb' or 'msb', not {order!r}")
            self.packing = Packing(bits, levels, msb_first=order == "msb")
        self.fileDataType = np.uint8 if bits < 8 else np.int8 if bits == 8 else np.int16 if bits == 16 else np.float32
        self.frontEnd = None                            # recordings that go through the down-converter: FrontEnd
        if "decimation" in configuration:
            self._front_end(configuration, bits)
        else:
            if "interpolation" in configuration:
                raise ValueError("`interpolation` needs `decimation` beside it: the ring's rate is sampling_frequency * L / M")
            for key in LAYOUT_KEYS + ARRAY_KEYS + MITIGATION_KEYS:
                if key in configuration:
                    raise ValueError(f"`{key}` needs a front end: set `decimation` (1 with `filter_taps = 1` converts nothing)")
        if not self.isComplex and self.frontEnd is None:
            raise ValueError("real-valued recordings are not supported: the correlators take I,Q samples")
        self.dtype = np.complex128                      # what a sample IS (the reference's rfSignal.dtype); storage stays integer
        self.samplesPerMs = int(self.samplingFrequency * 1e-3)
        if self.packing is not None and self.samplesPerMs % self.packing.samples_per_byte:
            raise ValueError(f"a millisecond of {self.samplesPerMs} samples at {bits} bit(s) is not a whole number of bytes")
        self._map = None
        self._next = 0                                  # samples handed out so far
        self._open = False                              # the reference's `file_id is not None` (readFile keep_open)

    def _front_end(self, configuration, bits: int):
        """The opt-in keys of a recording that is down-converted and decimated on its way into the ring."""
        from . import downconvert as dc
        sample_format = str(configuration["sample_format"]).strip().lower() if "sample_format" in configuration else None
        if sample_format is None:
            for key in LAYOUT_KEYS + ARRAY_KEYS:
                if key in configuration:
                    raise ValueError(f"`{key}` needs `sample_format` beside it")
            if self.packing is not None:
                raise ValueError("packed recordings cannot be down-converted: `decimation` needs data_size 8 or 16")
        else:
            self.layout = self._layout_keys(configuration, sample_format, bits)
        D = int(configuration["decimation"])
        L = int(configuration["interpolation"]) if "interpolation" in configuration else 1
        if not 1 <= L <= dc.MAX_INTERPOLATION:
            raise ValueError(f"interpolation {L} outside 1..{dc.MAX_INTERPOLATION}")
        d_max = min(dc.MAX_DECIMATION * L, dc.MAX_RATIONAL_DECIMATION)
        if not 1 <= D <= d_max:
            raise ValueError(f"decimation {D} outside 1..{d_max}")
        fs_in, if_in = self.samplingFrequency, self.interFrequency
        self.inputSamplingFrequency = fs_in
        self.inputSamplesPerMs = int(fs_in * 1e-3)
        if self.inputSamplesPerMs * L % D:
            raise ValueError(f"a millisecond of {self.inputSamplesPerMs} input samples" + (f" times interpolation {L}" if L != 1 else "")
                             + f" is not a whole multiple of decimation {D}")
        shift = float(configuration["baseband_shift"]) if "baseband_shift" in configuration else if_in
        # (L > 1: the prototype at the up-sampled rate, design_resampler's own defaults -- 16 max(L, M) + 1 taps, 0.45 / max(L, M))
        n_taps = int(configuration["filter_taps"]) if "filter_taps" in configuration else 16 * D + 1 if L == 1 else None
        cutoff = float(configuration["filter_cutoff"]) if "filter_cutoff" in configuration else 0.45 / D if L == 1 else None
        gain = float(configuration["output_gain"]) if "output_gain" in configuration else 1.0
        # (the ring's default width: the recording's own where that is one; 8 for packed samples, 16 for float32)
        out_bits = int(configuration["output_bits"]) if "output_bits" in configuration else bits if bits in (8, 16) else 8 if bits < 8 else 16
        if out_bits not in (8, 16):
            raise ValueError(f"output_bits is 8 or 16, not {out_bits}")
        in_fmt = {(False, 8): dc.IN_R8, (False, 16): dc.IN_R16, (True, 8): dc.IN_CI8, (True, 16): dc.IN_CI16}.get((self.isComplex, bits), dc.IN_R8)
        taps = dc.design_lowpass(n_taps, cutoff) if L == 1 else dc.design_resampler(L, D, n_taps, cutoff)
        geometry, plan = self._array_keys(configuration)
        config = dc.DownConverterConfig(in_fmt, D, taps, dc.frequency_word(shift, fs_in), gain, L, self.layout, geometry)
        self.frontEnd = FrontEnd(config, out_bits, shift, self._mitigation_keys(configuration, config), plan)
        # what the channels read is the ring's: its rate, and the carrier's residual offset there
        self.samplingFrequency = fs_in * L / D
        self.interFrequency = if_in - shift
        self._per_sample = 2 if self.isComplex else 1   # elements of the file per input sample

    def _layout_keys(self, configuration, sample_format: str, bits: int):
        """The opt-in keys `sample_format`, `frame_fields`, `frame_lane`, `swap_iq` -> the recording's input layout."""
        from . import downconvert as dc
        sizes = {"packed": (1, 2, 4), "float": (32,), "int": (8, 16)}
        if sample_format not in sizes:
            raise ValueError(f"sample_format is 'packed', 'float' or 'int', not {sample_format!r}")
        if bits not in sizes[sample_format]:
            raise ValueError(f"sample_format {sample_format!r} needs data_size {' or '.join(str(v) for v in sizes[sample_format])}, not {bits}")
        stride = int(configuration["frame_fields"]) if "frame_fields" in configuration else 2 if self.isComplex else 1
        lane = int(configuration["frame_lane"]) if "frame_lane" in configuration else 0
        swap = int(configuration["swap_iq"]) if "swap_iq" in configuration else 0
        if swap not in (0, 1):
            raise ValueError(f"swap_iq is 0 or 1, not {swap}")
        if sample_format == "packed":
            layout = dc.InputLayout(dc.FIELD_PACKED, bits, stride, lane, self.isComplex, bool(swap), self.packing.msb_first, self.packing.levels)
            self.packing = None                         # (not sdr_iq_upload_packed's route: the converter decodes the bytes)
        else:
            field = dc.FIELD_FLOAT32 if sample_format == "float" else dc.FIELD_INT8 if bits == 8 else dc.FIELD_INT16
            layout = dc.InputLayout(field, 0, stride, lane, self.isComplex, bool(swap))
        per_ms = int(self.samplingFrequency * 1e-3)
        if per_ms * layout.frame_bits % 8:
            raise ValueError(f"a millisecond of {per_ms} frames of {stride} fields of {bits} bit(s) is not a whole number of bytes")
        return layout

    def _array_keys(self, configuration):
        """The opt-in keys `array_lanes`, `array_mode`, `array_weights`, `array_steering`, `array_reference`, `array_loading`,
        `array_train_ms`, `array_taps`, `array_reference_tap` -> (array.ArrayGeometry -- with `array_taps` > 1 a
        stap.SpaceTimeGeometry --, ArrayPlan), or (None, None) without `array_lanes`."""
        from . import array as ar
        if "array_lanes" not in configuration:
            for key in ARRAY_KEYS:
                if key in configuration:
                    raise ValueError(f"`{key}` needs `array_lanes` beside it")
            return None, None
        for key in MITIGATION_KEYS:
            if key in configuration:
                raise ValueError(f"`{key}` beside `array_lanes`: the calibration of a mitigator behind an array is not offered")

        def pairs(key, K):
            v = [float.fromhex(t.strip()) if "0x" in t.lower() else float(t) for t in str(configuration[key]).split(",")]
            if len(v) != 2 * K:
                raise ValueError(f"`{key}` is {K} re,im pairs, {len(v)} numbers given")
            return ar.as_weights(np.array(v).reshape(K, 2), K)
        lanes = [int(v) for v in str(configuration["array_lanes"]).split(",")]
        K = len(lanes)
        mode = str(configuration["array_mode"]).strip().lower() if "array_mode" in configuration else "fixed"
        if mode not in ("fixed", "power_inversion", "mvdr"):
            raise ValueError(f"array_mode is 'fixed', 'power_inversion' or 'mvdr', not {mode!r}")
        reference = int(configuration["array_reference"]) if "array_reference" in configuration else 0
        if not 0 <= reference < K:
            raise ValueError(f"array_reference {reference} outside 0..{K - 1}")
        loading = float(configuration["array_loading"]) if "array_loading" in configuration else ar.DEFAULT_LOADING
        if not loading >= 0.0:
            raise ValueError("array_loading is not negative")
        train_ms = int(configuration["array_train_ms"]) if "array_train_ms" in configuration else 2
        if train_ms < 1:
            raise ValueError("array_train_ms is at least 1")
        taps = int(configuration["array_taps"]) if "array_taps" in configuration else 1
        if not 1 <= taps <= 8:
            raise ValueError(f"array_taps {taps} outside 1..8")
        reference_tap = int(configuration["array_reference_tap"]) if "array_reference_tap" in configuration else (taps - 1) // 2
        if not 0 <= reference_tap < taps:
            raise ValueError(f"array_reference_tap {reference_tap} outside 0..{taps - 1}")
        allowed = {"fixed": ("array_weights", "array_reference"), "power_inversion": ("array_reference", "array_loading", "array_train_ms"),
                   "mvdr": ("array_steering", "array_reference", "array_loading", "array_train_ms")}[mode]
        for key in ARRAY_KEYS[2:7]:
            if key in configuration and key not in allowed:
                raise ValueError(f"`{key}` does not belong to array_mode {mode!r}")
        if mode == "mvdr" and "array_steering" not in configuration:
            raise ValueError("array_mode 'mvdr' needs `array_steering`")
        # (an adaptive mode trains with unit weight on the reference element and measures the covariance)
        weights = None
        if taps == 1:
            weights = pairs("array_weights", K) if "array_weights" in configuration else ar.unit_weights(K, reference)
        steering = pairs("array_steering", K) if mode == "mvdr" else None
        if taps > 1:                      # T taps per element: weights [T][K], unit weight on the reference element at the reference tap
            from . import stap
            if "array_weights" in configuration:
                weights = pairs("array_weights", taps * K).reshape(taps, K)
            else:
                weights = stap.unit_weights(taps, K, reference, reference_tap)
            geometry = stap.SpaceTimeGeometry(lanes, taps, weights, measure=mode != "fixed")
        else:
            geometry = ar.ArrayGeometry(lanes, weights, measure=mode != "fixed")
        geometry.check(self.layout)
        return geometry, ArrayPlan(mode, reference, loading, train_ms, steering, taps, reference_tap)

    def _layout_span(self, first: int, n_samples: int):
        """Frames [first, first + n_samples) of a recording with a layout as elements of the mapped file: whole bytes."""
        lay = self.layout
        lo, hi = first * lay.frame_bits, (first + n_samples) * lay.frame_bits
        if lo % 8 or hi % 8:
            raise ValueError(f"frames [{first}, {first + n_samples}) of {lay.stride} fields of {lay.field_bits} bit(s) are not whole bytes")
        size = 8 * np.dtype(self.fileDataType).itemsize
        return lo // size, hi // size

    def _mitigation_keys(self, configuration, config):
        """The opt-in mitigation keys -> the calibration to run when the front end's `mitigation` is first asked for (None
        without `blanking_factor` and `excision_nfft`).  Everything but the measurement is checked here."""
        from . import mitigate as mt
        factor = float(configuration["blanking_factor"]) if "blanking_factor" in configuration else None
        nfft = int(configuration["excision_nfft"]) if "excision_nfft" in configuration else 0
        if factor is None and not nfft:
            for key in MITIGATION_KEYS:
                if key in configuration:
                    raise ValueError(f"`{key}` without `blanking_factor` or `excision_nfft`")
            return None
        lead = int(configuration["blanking_lead"]) if "blanking_lead" in configuration else 0
        hold = int(configuration["blanking_hold"]) if "blanking_hold" in configuration else 0
        margin = float(configuration["excision_margin_db"]) if "excision_margin_db" in configuration else 10.0
        ms = int(configuration["calibration_ms"]) if "calibration_ms" in configuration else 8
        if factor is not None and not factor > 0.0:
            raise ValueError("blanking_factor is a positive multiple of the noise amplitude")
        if ms < 1:
            raise ValueError("calibration_ms is at least 1")
        # (the ranges of nfft, lead and hold: MitigationConfig's own checks, on a stand-in that needs no measurement)
        mt.MitigationConfig(1.0 if factor is not None else 0.0, lead, hold, nfft, np.full(nfft, np.inf) if nfft else None)

        def calibrate():
            from . import downconvert as dc
            n_in = min(ms * self.inputSamplesPerMs, self.totalSamples)
            if self.layout is not None:
                n_in -= n_in % self.layout.frame_group      # (whole bytes)
            v = dc.statement(config, [self.samples(0, n_in)])
            level = mt.blanking_level(v, factor) if factor is not None else 0.0
            limit = mt.excision_limits(v, nfft, margin) if nfft else None
            return mt.MitigationConfig(level, lead, hold, nfft, limit)
        return calibrate

    # ------------------------------------------------------------------ the recording
    def _recording(self) -> np.ndarray:
        if self._map is None:
            if not os.path.isfile(self.filepath):
                raise FileNotFoundError(f"IQ recording {self.filepath!r} does not exist")
            self._mapping = np.memmap(self.filepath, dtype=self.fileDataType, mode="r")
            # (a plain ndarray over the mapping: slicing an np.memmap costs ~10 us per slab in subclass bookkeeping)
            self._map = np.asarray(self._mapping) if self._mapping.size else self._mapping
        return self._map

    @property
    def totalSamples(self) -> int:
        rec = self._recording()
        if self.layout is not None:                     # (frames)
            return 8 * rec.nbytes // self.layout.frame_bits
        if self.frontEnd is not None:                   # (INPUT samples: what `samples` and `getMilliseconds` hand out)
            return rec.size // self._per_sample
        return rec.size * self.packing.samples_per_byte if self.packing is not None else rec.size // 2

    def samples(self, first: int, n_samples: int) -> np.ndarray:
        """Samples [first, first + n_samples) as the file holds them -- a view of the mapping: interleaved integers, or
        the packed bytes (which then have to be whole: both numbers multiples of the samples per byte)."""
        rec = self._recording()
        first, n_samples = int(first), int(n_samples)
        if self.layout is not None:                     # the recording's bytes, counted in frames: whole bytes
            lo, hi = self._layout_span(first, n_samples)
            return rec[lo:hi]
        if self.frontEnd is not None:                   # raw input: real recordings hold one element per sample
            return rec[self._per_sample * first:self._per_sample * (first + n_samples)]
        if self.packing is None:
            return rec[2 * first:2 * (first + n_samples)]
        spb = self.packing.samples_per_byte
        if first % spb or n_samples % spb:
            raise ValueError(f"samples [{first}, {first + n_samples}) of a {self.packing.bits}-bit recording are not whole bytes")
        return rec[first // spb:(first + n_samples) // spb]

    def _complex(self, first: int, n_samples: int) -> np.ndarray:
        """Samples [first, first + n_samples) as complex128, the reference's sample type -- any two numbers: of a packed
        recording the bytes that cover them are unpacked and the samples cut out."""
        if self.layout is not None:                     # `decode` over the whole bytes that cover the frames
            from . import downconvert as dc
            lay = self.layout
            lead = first % lay.frame_group
            cover = min(-(-(lead + n_samples) // lay.frame_group) * lay.frame_group, (self.totalSamples - (first - lead)) // lay.frame_group * lay.frame_group)
            if cover < lead + n_samples:                # (a file that ends inside a group of frames: its last bytes field by field)
                f = dc.fields(self._recording().view(np.uint8)[(first - lead) * lay.frame_bits // 8:], lay).astype(np.float64)
                at = (lead + np.arange(n_samples)) * lay.stride + lay.lane
                xr, xi = (f[at], f[at + 1] if lay.complex else np.zeros(n_samples))
                xr, xi = (xi, xr) if lay.swap_iq else (xr, xi)
            else:
                xr, xi = dc.decode(self.samples(first - lead, cover), lay)
                xr, xi = xr[lead:lead + n_samples], xi[lead:lead + n_samples]
            return xr + 1j * xi
        if self.frontEnd is not None and not self.isComplex:
            return self.samples(first, n_samples).astype(np.float64) + 0j
        if self.packing is None:
            block = self.samples(first, n_samples)
        else:
            spb = self.packing.samples_per_byte
            lead = first % spb
            cover = -(-(lead + n_samples) // spb) * spb
            block = unpack(self.samples(first - lead, cover), self.packing)[2 * lead:2 * (lead + n_samples)]
        return block[0::2].astype(np.float64) + 1j * block[1::2].astype(np.float64)

    @property
    def position(self) -> int:
        """Index of the next sample `getMilliseconds` will deliver."""
        return self._next

    def seek(self, sample: int):
        if not 0 <= sample <= self.totalSamples:
            raise ValueError(f"sample {sample} outside the recording's {self.totalSamples}")
        self._next = int(sample)

    def slab(self, n_samples: int, raw: bool = True) -> np.ndarray:
        """The next n_samples as interleaved integers [I0, Q0, I1, Q1, ...] -- a view of the mapped file; of a packed
        recording as packed bytes, which have to be whole (ValueError when the cursor or n_samples is not a multiple of the
        samples per byte: a view cannot begin inside a byte).  raw=False: as complex128, from any cursor."""
        stop = self._next + int(n_samples)
        if stop > self.totalSamples:
            raise EOFError(f"recording ends at sample {self.totalSamples}, {stop} requested")
        out = self.samples(self._next, int(n_samples)) if raw else self._complex(self._next, int(n_samples))
        self._next = stop
        return out

    # ------------------------------------------------------------------ the reference's call (receiver.py:124)
    def getMilliseconds(self, nbMilliseconds: int = 1, raw: bool = True):
        """Next `nbMilliseconds` of signal.  raw=True (default): interleaved integers (packed bytes) for the device ring;
        raw=False: complex128 like the reference's RFSignal.getMilliseconds (rfsignal.py:58-88).  Of a recording with a
        front end: raw INPUT (a real recording's integers one per sample), a millisecond being `inputSamplesPerMs` of them."""
        per_ms = self.samplesPerMs if self.frontEnd is None else self.inputSamplesPerMs
        return self.slab(per_ms * int(nbMilliseconds), raw)

    # ------------------------------------------------------------------ the reference's file readers (rfsignal.py:92-204)
    def _read(self, n_samples: int, skip: int, keep_open: bool, raw: bool):
        """`skip` counts from the cursor while the file is "open" (np.fromfile(fid, offset=...) on a kept descriptor),
        from the start of the recording otherwise; a short read at the end of the file returns what is there.  raw=True on a
        packed recording hands out packed bytes and needs whole ones (ValueError otherwise, as `slab`)."""
        first = (self._next if self._open else 0) + int(skip)
        stop = min(first + int(n_samples), self.totalSamples)
        count = max(stop, first) - first
        block = self.samples(first, count) if raw else self._complex(first, count)
        if keep_open:
            self._open, self._next = True, max(stop, first)
        elif self._open:              # the kept descriptor is closed by a read without keep_open (rfsignal.py:118-121)
            self._open = False
        return block

    def readFile(self, timeLength, skip=0, keep_open=False, raw=False):
        """`timeLength` milliseconds of signal (complex128 like the reference; raw=True: the interleaved integers)."""
        fs = self.samplingFrequency if self.frontEnd is None else self.inputSamplingFrequency
        return self._read(int((timeLength * 1e-3) * fs), skip, keep_open, raw)

    def readFileBySamples(self, nb_values, skip=0, keep_open=False, raw=False):
        return self._read(int(nb_values), skip, keep_open, raw)

    def closeFile(self):
        if not self._open:
            raise Warning("File was already close.")
        self._open = False

    def getCurrentSampleIndex(self):
        if not self._open:
            raise Warning("Signal file not open, cannot return current cursor position.")
        return int(self._next)
