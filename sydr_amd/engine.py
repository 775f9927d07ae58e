"""Engine: one MI355X's correlator state (IQ ring, staged PRN replicas, work buffers)
behind the C-ABI.  NumPy arrays in, NumPy arrays out; the arithmetic all runs in the HIP
library (there is deliberately no host implementation to fall back to)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import (COH_RESULT_DTYPE, EPL_ITEM_DTYPE, FMT_CF32, FMT_CF64, FMT_CI16, FMT_CI8, LOOP_CFG_DTYPE, REFINE_ITEM_DTYPE,
                   REFINE_RESULT_DTYPE, SEC_ITEM_DTYPE, SEC_RESULT_DTYPE, TRACK_EPOCH_DTYPE, TRACK_STATE_DTYPE, LoopCfg, SynthSat,
                   TrackState, check, ptr)

__all__ = ["Engine", "EplPlan", "Bank", "make_items", "make_refine_items", "make_secondary_items", "FMT_CI8", "FMT_CI16", "FMT_CF32",
           "FMT_CF64"]


def make_refine_items(code_slot, start_sample, carrier_hz, code_hz=1.023e6) -> np.ndarray:
    """Pack acquisition results (scalars or equal-length arrays) into sdr_refine_item records."""
    arrs = np.broadcast_arrays(code_slot, start_sample, carrier_hz, code_hz)
    items = np.zeros(arrs[0].shape, dtype=REFINE_ITEM_DTYPE).reshape(-1)
    for name, a in zip(("code_slot", "start_sample", "carrier_hz", "code_hz"), arrs):
        items[name] = np.asarray(a).reshape(-1)
    return items


def make_secondary_items(code_slot, sec_row, start_sample, carrier_hz, code_hz) -> np.ndarray:
    """Pack acquisition results (scalars or equal-length arrays) into sdr_sec_item records."""
    arrs = np.broadcast_arrays(code_slot, sec_row, start_sample, carrier_hz, code_hz)
    items = np.zeros(arrs[0].shape, dtype=SEC_ITEM_DTYPE).reshape(-1)
    for name, a in zip(SEC_ITEM_DTYPE.names, arrs):
        items[name] = np.asarray(a).reshape(-1)
    return items


def make_items(code_slot, n_samples, start_sample, carrier_hz, rem_carrier, rem_code, code_step) -> np.ndarray:
    """Pack per-epoch NCO parameters (scalars or equal-length arrays) into sdr_epl_item records."""
    arrs = np.broadcast_arrays(code_slot, n_samples, start_sample, carrier_hz, rem_carrier, rem_code, code_step)
    items = np.zeros(arrs[0].shape, dtype=EPL_ITEM_DTYPE).reshape(-1)
    for name, a in zip(EPL_ITEM_DTYPE.names, arrs):
        items[name] = np.asarray(a).reshape(-1)
    return items


_addressof = C.addressof
_char_from_buffer = C.c_char.from_buffer


class EplPlan:
    """Items + outputs resident in HBM; run() only launches kernels (asynchronous)."""

    def __init__(self, engine: "Engine", items, spacing, fs: float, device_items: int = 0, n_items: int = 0):
        """items: the list (host array), or device_items: the address of n_items items in DEVICE memory
        (sdr_epl_plan_create_dev: copied there and checked there)."""
        self._e = engine
        self._lib = _lib.load()
        spacing = np.ascontiguousarray(spacing, dtype=np.float64)
        self.n_taps = len(spacing)
        self._h = C.c_void_p()
        if device_items:
            self.n_items = int(n_items)
            check(self._lib.sdr_epl_plan_create_dev(engine._h, C.c_void_p(int(device_items)), self.n_items, ptr(spacing),
                                                    self.n_taps, float(fs), C.byref(self._h)))
            return
        items = np.ascontiguousarray(items, dtype=EPL_ITEM_DTYPE)
        self.n_items = len(items)
        check(self._lib.sdr_epl_plan_create(engine._h, ptr(items), self.n_items, ptr(spacing), self.n_taps,
                                            float(fs), C.byref(self._h)))

    def run(self, first=None, count=None, stream=0):
        """Asynchronous launch of the whole plan or of items [first, first+count), on the engine's stream or on
        one made by Engine.stream_create() (one stream per channel batch)."""
        if first is None:
            first, count = 0, self.n_items
        check(self._lib.sdr_epl_plan_run_range_on(self._e._h, self._h, int(first), int(count), int(stream)))

    @property
    def variant(self) -> int:
        """Which correlator variant the items selected (sdr_epl_plan_variant: diagnostics)."""
        return int(self._lib.sdr_epl_plan_variant(self._h))

    def fetch(self) -> np.ndarray:
        out = np.empty((self.n_items, 2 * self.n_taps), dtype=np.float64)
        check(self._lib.sdr_epl_plan_fetch(self._e._h, self._h, ptr(out)))
        return out

    def close(self):
        if self._h:
            self._lib.sdr_epl_plan_destroy(self._e._h, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bank:
    """The tracking state of one GPU's channels, resident in HBM (sdr_bank_*): `put` a channel after acquisition,
    `step` / `tick` advance the listed channels on the device and hand back the epoch records and the new states."""

    def __init__(self, engine: "Engine", max_channels: int):
        self._e = engine
        self._lib = _lib.load()
        self.max_channels = int(max_channels)
        self._h = C.c_void_p()
        check(self._lib.sdr_bank_create(engine._h, self.max_channels, C.byref(self._h)))

    def put(self, ch: int, state: np.ndarray, cfg: np.ndarray):
        state = np.ascontiguousarray(state, dtype=TRACK_STATE_DTYPE).reshape(1)
        cfg = np.ascontiguousarray(cfg, dtype=LOOP_CFG_DTYPE).reshape(1)
        check(self._lib.sdr_bank_put(self._e._h, self._h, int(ch), ptr(state), ptr(cfg)))

    def get(self, ch: int) -> np.ndarray:
        out = np.zeros(1, dtype=TRACK_STATE_DTYPE)
        check(self._lib.sdr_bank_get(self._e._h, self._h, int(ch), ptr(out)))
        return out[0]

    def step(self, channels, n_epochs: int = 1, want_records=True, want_bits=False, stream=0, epochs_per_bit=20):
        """-> (records[n][n_epochs] or None, states[n], epochs_done[n], list of nav-bit arrays or None)"""
        channels = np.ascontiguousarray(channels, dtype=np.int32)
        n = len(channels)
        rec = np.zeros((n, n_epochs), dtype=TRACK_EPOCH_DTYPE) if want_records else None
        states = np.zeros(n, dtype=TRACK_STATE_DTYPE)
        done = np.zeros(n, dtype=np.int32)
        max_bits = n_epochs // max(1, int(epochs_per_bit)) + 2
        bits = np.zeros((n, max_bits), dtype=np.int8) if want_bits else None
        n_bits = np.zeros(n, dtype=np.int32) if want_bits else None
        check(self._lib.sdr_bank_step(self._e._h, self._h, ptr(channels), n, int(n_epochs),
                                      ptr(rec) if want_records else None, ptr(states), ptr(done),
                                      ptr(bits) if want_bits else None, max_bits if want_bits else 0,
                                      ptr(n_bits) if want_bits else None, int(stream)))
        nav = [bits[c, :n_bits[c]].copy() for c in range(n)] if want_bits else None
        return rec, states, done, nav

    def step_begin(self, channels, n_epochs: int):
        """`step` without the wait (sdr_bank_step_begin): the launch and the copies of its results are queued on the
        engine's stream; `step_end()` hands them out.  One step in flight per bank."""
        channels = np.ascontiguousarray(channels, dtype=np.int32)
        check(self._lib.sdr_bank_step_begin(self._e._h, self._h, ptr(channels), len(channels), int(n_epochs)))
        self._in_flight = (len(channels), int(n_epochs))

    def step_end(self):
        """-> (records[n][n_epochs], states[n], epochs_done[n]) of the step `step_begin` queued."""
        if getattr(self, "_in_flight", None) is None:
            # (never ask the library: a step begun through another wrapper would be collected into nothing and discarded)
            raise RuntimeError("step_end(): no step of this bank was begun through this object (step_begin first)")
        n, n_epochs = self._in_flight
        self._in_flight = None
        rec = np.empty((n, n_epochs), dtype=TRACK_EPOCH_DTYPE)
        states = np.empty(n, dtype=TRACK_STATE_DTYPE)
        done = np.zeros(n, dtype=np.int32)
        check(self._lib.sdr_bank_step_end(self._e._h, self._h, ptr(rec), ptr(states), ptr(done)))
        return rec, states, done

    def tick(self, raw, ring_offset: int, channels):
        """One receiver tick: `raw` (the ring's format, may be None) goes into the ring at ring_offset, then the
        listed channels run one epoch.  -> (records[n], states[n], epochs_done[n])"""
        channels = np.ascontiguousarray(channels, dtype=np.int32)
        n = len(channels)
        rec = np.empty(n, dtype=TRACK_EPOCH_DTYPE)          # (all three are filled by the call)
        states = np.empty(n, dtype=TRACK_STATE_DTYPE)
        done = np.zeros(n, dtype=np.int32)
        n_samples = 0
        if raw is not None:
            raw = self._e._ring_samples(raw)
            n_samples = raw.size // 2
        check(self._lib.sdr_bank_tick(self._e._h, self._h, ptr(raw) if n_samples else None, n_samples, int(ring_offset),
                                      ptr(channels) if n else None, n, ptr(rec) if n else None,
                                      ptr(states) if n else None, ptr(done) if n else None))
        return rec, states, done

    def bind_mirror(self, states, last, epochs_since_tow, tracking, lost, host_flags):
        """The caller's mirrors of the bank (NumPy arrays of max_channels rows, kept alive by the caller) as the
        sdr_tick_mirror `tick_mirrored` updates in place.  Per-tick outputs: `ran`, `records`, `updates` (views of
        arrays this object owns: copy what has to outlive the next tick)."""
        n = self.max_channels
        for a, dt in ((states, TRACK_STATE_DTYPE), (last, TRACK_EPOCH_DTYPE), (epochs_since_tow, np.int64),
                      (tracking, np.bool_), (lost, np.bool_), (host_flags, np.int64)):
            if a.dtype != dt or a.shape != (n,) or not a.flags.c_contiguous:
                raise ValueError("tick mirror arrays must be contiguous, one row per bank channel, in the bank's dtypes")
        self._mirror_arrays = (states, last, epochs_since_tow, tracking, lost, host_flags)
        # TWO sets of per-tick outputs, used alternately (`out_set`): what a tick left in `ran` / `records` / `updates` stays
        # untouched through the NEXT tick, so a caller that hands out views of them (the channel bank's lazy packets) need not
        # copy 8 KB per millisecond -- only what is still looked at when the set comes round again (ChannelBank.hold)
        self._sets = []
        for _ in range(2):
            ran = np.zeros(n, dtype=np.int32)
            records = np.zeros(n, dtype=TRACK_EPOCH_DTYPE)
            updates = np.zeros(n, dtype=_lib.TICK_UPDATE_DTYPE)
            m = _lib.TickMirror()
            m.max_channels = n
            m.states, m.last, m.epochs_since_tow = states.ctypes.data, last.ctypes.data, epochs_since_tow.ctypes.data
            m.tracking, m.lost, m.host_flags = tracking.ctypes.data, lost.ctypes.data, host_flags.ctypes.data
            m.ran, m.records, m.updates = ran.ctypes.data, records.ctypes.data, updates.ctypes.data
            self._sets.append((ran, records, updates, m, C.byref(m)))
        self.out_set = 0
        self.ran, self.records, self.updates, self._mirror, self._mirror_ref = self._sets[0]
        self._tick_no_slab = (self._e._h, self._h, None, 0)        # leading arguments of a tick whose slab is queued already
        return self._mirror

    double_buffered = True      # (per-tick outputs alternate between two sets: see bind_mirror)

    def _next_set(self):
        k = self.out_set = self.out_set ^ 1
        self.ran, self.records, self.updates, self._mirror, self._mirror_ref = self._sets[k]

    def tick_mirrored(self, raw, ring_offset: int, write_index: int):
        """One receiver tick with the readiness test and the mirror updates in the library (sdr_bank_tick_mirrored);
        `raw` None when the slab went in with Engine.iq_upload_begin.  -> the bound sdr_tick_mirror (n_ran, n_updates,
        n_nav_bits, n_lost, max_unread; the rows in `ran` / `records` / `updates`)."""
        self._next_set()
        if raw is None:
            status = self._lib.sdr_bank_tick_mirrored(*self._tick_no_slab, ring_offset, write_index, self._mirror_ref)
        else:
            raw = self._e._ring_samples(raw)
            status = self._lib.sdr_bank_tick_mirrored(self._e._h, self._h, ptr(raw), raw.size // 2, ring_offset, write_index,
                                                      self._mirror_ref)
        if status:
            check(status)
        return self._mirror

    def tick_mirrored_begin(self, raw, ring_offset: int, write_index: int):
        """First half of `tick_mirrored` (sdr_bank_tick_mirrored_begin): who is ready is decided and their epoch queued on
        the engine's stream; nothing is waited for.  A manager of several devices begins every device's tick, then ends
        each."""
        self._next_set()
        if raw is None:
            status = self._lib.sdr_bank_tick_mirrored_begin(*self._tick_no_slab, ring_offset, write_index, self._mirror_ref)
        else:
            raw = self._e._ring_samples(raw)
            status = self._lib.sdr_bank_tick_mirrored_begin(self._e._h, self._h, ptr(raw), raw.size // 2, ring_offset, write_index,
                                                            self._mirror_ref)
        if status:
            check(status)

    def tick_mirrored_end(self):
        """Second half: wait, mirrors and per-tick rows updated in place.  -> the bound sdr_tick_mirror."""
        status = self._lib.sdr_bank_tick_mirrored_end(self._e._h, self._h, self._mirror_ref)
        if status:
            check(status)
        return self._mirror

    def close(self):
        if self._h and self._e._h:
            self._lib.sdr_bank_destroy(self._e._h, self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def layout_struct(layout) -> "_lib.DdcLayout":
    """sdr_ddc_layout of a signal.downconvert.InputLayout."""
    c = _lib.DdcLayout(int(layout.field), int(layout.bits), int(layout.stride), int(layout.lane), int(layout.flags), 0)
    for i, v in enumerate(layout.levels.tolist()):
        c.levels[i] = v
    return c


def array_struct(array) -> "_lib.DdcArray":
    """sdr_ddc_array of a signal.array.ArrayGeometry."""
    c = _lib.DdcArray(int(array.n_elements), int(array.flags))
    for a, lane in enumerate(array.lanes):
        c.lanes[a] = lane
        c.weights[a][0], c.weights[a][1] = float(array.weights[a].real), float(array.weights[a].imag)
    return c


def stap_array_struct(array) -> "_lib.DdcArray":
    """sdr_ddc_array of a signal.stap.SpaceTimeGeometry: lanes and flags (its weights are not read)."""
    c = _lib.DdcArray(int(array.n_elements), int(array.flags))
    for a, lane in enumerate(array.lanes):
        c.lanes[a] = lane
    return c


class _Ddc:
    """Handle of a device-resident down-converter (Engine.ddc_create)."""
    __slots__ = ("handle", "in_fmt", "nfft", "layout", "n_elements", "n_taps")

    def __init__(self, handle, in_fmt, layout=None, n_elements=0, n_taps=0):
        self.handle, self.in_fmt = handle, in_fmt
        self.n_taps = n_taps          # T of a converter made by sdr_ddc_create_stap, else 0
        self.n_elements = n_elements  # K of a converter made by sdr_ddc_create_array, else 0
        self.layout = layout          # signal.downconvert.InputLayout of a converter made by sdr_ddc_create_layout, else None
        self.nfft = 0                 # of the attached mitigator's excisor (Engine.ddc_mitigate)


class Engine:
    def __init__(self, device_id: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        check(self._lib.sdr_engine_create(int(device_id), C.byref(self._h)))
        self.device_id = device_id
        self.iq_fmt = None
        self.iq_capacity = 0
        self._host_blocks = {}        # page-locked blocks handed out by host_alloc: address -> block

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if self._h:
            for block in list(getattr(self, "_host_blocks", {}).values()):
                self._lib.sdr_host_free(self._h, block)
            self._host_blocks = {}
            self._lib.sdr_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._lib.sdr_engine_sync(self._h))

    def prof_enable(self, on=True, calls_only=False):
        """Per-stage HIP-event timing (`prof_read`); calls_only: one event pair around each whole call instead
        (scopes named "call_*": the in-stream time of everything the call launched)."""
        check(self._lib.sdr_prof_enable(self._h, (2 if calls_only else 1) if on else 0))

    def prof_reset(self):
        check(self._lib.sdr_prof_reset(self._h))

    def prof_read(self, prefix=""):
        tot, cnt = C.c_double(0), C.c_int64(0)
        check(self._lib.sdr_prof_read(self._h, prefix.encode(), C.byref(tot), C.byref(cnt)))
        return tot.value, cnt.value

    def set_option(self, name: str, value: int):
        check(self._lib.sdr_set_option(self._h, name.encode(), int(value)))

    def hbm_copy_rate(self, n_bytes: int = 1 << 30, reps: int = 10) -> float:
        """Measured GB/s (read + written) of a hand-written stream-copy kernel on this GPU."""
        g = C.c_double(0)
        check(self._lib.sdr_hbm_copy_rate(self._h, int(n_bytes), int(reps), C.byref(g)))
        return g.value

    # ------------------------------------------------------------------ IQ ring
    def iq_alloc(self, capacity_samples: int, fmt: int = FMT_CI8):
        check(self._lib.sdr_iq_alloc(self._h, int(capacity_samples), int(fmt)))
        self.iq_fmt, self.iq_capacity = fmt, int(capacity_samples)

    def _ring_samples(self, raw) -> np.ndarray:
        """Interleaved I,Q in the ring's element type (complex input is split; no copy when already right)."""
        dt = _lib.fmt_dtype(self.iq_fmt)
        if np.iscomplexobj(raw):
            raw = np.ascontiguousarray(raw, dtype=np.complex128).view(np.float64)
            if self.iq_fmt != FMT_CF64:
                raw = raw.astype(dt)
        raw = np.ascontiguousarray(raw, dtype=dt).reshape(-1)
        if raw.size % 2:
            raise ValueError("interleaved IQ needs an even number of elements")
        return raw

    def iq_upload(self, raw: np.ndarray, ring_offset: int = 0):
        """raw: interleaved I,Q in the ring's element type (complex128 accepted for FMT_CF64)."""
        raw = self._ring_samples(raw)
        check(self._lib.sdr_iq_upload(self._h, ptr(raw), raw.size // 2, int(ring_offset)))

    def iq_upload_begin(self, raw: np.ndarray, ring_offset: int = 0):
        """iq_upload without the wait (sdr_iq_upload_begin): `raw` is copied before the call returns, the transfer is
        ordered before everything queued on the engine's stream afterwards; `sync()` completes it."""
        if not (type(raw) is np.ndarray and raw.ndim == 1 and raw.flags.c_contiguous and raw.dtype == _lib.fmt_dtype(self.iq_fmt)):
            raw = self._ring_samples(raw)
        # (the array's address through the buffer protocol: `raw.ctypes.data` builds a helper object per call -- a microsecond of
        # a tick that is made of thirty; a read-only array has no writable buffer to offer and takes the long way)
        try:
            address = _addressof(_char_from_buffer(raw))
        except (TypeError, ValueError):
            address = raw.ctypes.data
        status = self._lib.sdr_iq_upload_begin(self._h, address, raw.size >> 1, ring_offset)
        if status:
            check(status)

    def iq_upload_queue(self, raw: np.ndarray, ring_offset: int = 0):
        """A chunk of a recording queued for the ring without a copy of its own (sdr_iq_upload_queue): `raw` -- contiguous,
        the ring's element type -- must stay alive and unchanged until `sync()`.  From `host_alloc` memory the call returns at
        once and the transfer overlaps what other streams compute."""
        if not (isinstance(raw, np.ndarray) and raw.ndim == 1 and raw.flags.c_contiguous and raw.dtype == _lib.fmt_dtype(self.iq_fmt)
                and not raw.size & 1):
            raise ValueError("iq_upload_queue takes a contiguous 1-D array of interleaved I,Q in the ring's element type")
        status = self._lib.sdr_iq_upload_queue(self._h, raw.ctypes.data, raw.size >> 1, int(ring_offset))
        if status:
            check(status)

    # ------------------------------------------------------------------ packed recordings (signal/packing.py)
    def _packed_args(self, packed, n_samples, packing):
        """(sdr_iq_packing, address, n_samples) of a packed slab: contiguous uint8, as long as the samples need."""
        if not (isinstance(packed, np.ndarray) and packed.ndim == 1 and packed.dtype == np.uint8 and packed.flags.c_contiguous):
            raise ValueError("packed samples are a contiguous 1-D uint8 array")
        n_samples = int(n_samples)
        pk = getattr(packing, "_c_struct", None)
        if pk is None:
            pk = _lib.IqPacking(int(packing.bits), _lib.PACK_MSB_FIRST if packing.msb_first else 0)
            for i, v in enumerate(packing.levels.tolist()):
                pk.levels[i] = v
            packing._c_struct = pk
        need = self._lib.sdr_iq_packed_bytes(C.byref(pk), n_samples)
        if need >= 0 and packed.size != need:
            raise ValueError(f"{n_samples} samples at {packing.bits} bits are {need} packed bytes, {packed.size} given")
        # (need < 0: the library refuses the call below with its own status and text)
        return pk, packed.ctypes.data, n_samples

    def iq_upload_packed(self, packed: np.ndarray, n_samples: int, packing, ring_offset: int = 0):
        """Packed 1- / 2- / 4-bit I,Q into a ci8 ring, widened on the device (sdr_iq_upload_packed): synchronous."""
        pk, address, n = self._packed_args(packed, n_samples, packing)
        check(self._lib.sdr_iq_upload_packed(self._h, C.byref(pk), address, n, int(ring_offset)))

    def iq_upload_packed_begin(self, packed: np.ndarray, n_samples: int, packing, ring_offset: int = 0):
        """iq_upload_packed without the wait (sdr_iq_upload_packed_begin): a receiver tick's slab, copied before the call
        returns (a `host_alloc` block on a 16-byte boundary is read in place, as with `iq_upload_begin`)."""
        pk, address, n = self._packed_args(packed, n_samples, packing)
        check(self._lib.sdr_iq_upload_packed_begin(self._h, C.byref(pk), address, n, int(ring_offset)))

    def iq_upload_packed_queue(self, packed: np.ndarray, n_samples: int, packing, ring_offset: int = 0):
        """A packed chunk of a recording queued for the ring (sdr_iq_upload_packed_queue): `packed` stays alive and
        unchanged until `sync()`."""
        pk, address, n = self._packed_args(packed, n_samples, packing)
        check(self._lib.sdr_iq_upload_packed_queue(self._h, C.byref(pk), address, n, int(ring_offset)))

    # ------------------------------------------------------------------ down-conversion into the ring (signal/downconvert.py)
    def ddc_create(self, cfg):
        """A device-resident down-converter (sdr_ddc_create; with cfg.interpolation != 1 sdr_ddc_create_rational; with
        cfg.layout sdr_ddc_create_layout; with cfg.array sdr_ddc_create_array, or, when the array has `taps` -- a
        signal.stap.SpaceTimeGeometry --, sdr_ddc_create_stap) of a signal.downconvert.DownConverterConfig -> its handle."""
        taps = np.ascontiguousarray(cfg.taps, dtype=np.float64)
        c = _lib.DdcCfg(int(cfg.in_fmt), int(cfg.decimation), int(taps.size), 0, int(cfg.fcw), float(cfg.gain),
                        taps.ctypes.data_as(C.POINTER(C.c_double)))
        h = C.c_void_p()
        interpolation = int(cfg.interpolation)
        layout = getattr(cfg, "layout", None)
        array = getattr(cfg, "array", None)
        if array is not None and hasattr(array, "taps"):     # space-time weights: T taps per element (signal/stap.py)
            w = np.ascontiguousarray(np.stack([array.weights.real, array.weights.imag], axis=2))
            check(self._lib.sdr_ddc_create_stap(self._h, C.byref(c), interpolation, C.byref(layout_struct(layout)), C.byref(stap_array_struct(array)),
                                                int(array.taps), w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(h)))
            return _Ddc(h, int(cfg.in_fmt), layout, array.n_elements, int(array.taps))
        if array is not None:             # an antenna array: the K elements of the layout's frames combined (signal/array.py)
            check(self._lib.sdr_ddc_create_array(self._h, C.byref(c), interpolation, C.byref(layout_struct(layout)), C.byref(array_struct(array)),
                                                 C.byref(h)))
            return _Ddc(h, int(cfg.in_fmt), layout, array.n_elements)
        if layout is not None:            # an input layout: packed, float32 or interleaved recordings (in_fmt is not read)
            check(self._lib.sdr_ddc_create_layout(self._h, C.byref(c), interpolation, C.byref(layout_struct(layout)), C.byref(h)))
            return _Ddc(h, int(cfg.in_fmt), layout)
        if interpolation != 1:            # a rational resampler by L / M (sdr_ddc_create_rational): decimation is M
            check(self._lib.sdr_ddc_create_rational(self._h, C.byref(c), interpolation, C.byref(h)))
        else:
            check(self._lib.sdr_ddc_create(self._h, C.byref(c), C.byref(h)))
        return _Ddc(h, int(cfg.in_fmt))

    def _ddc_push(self, call, ddc, raw, ring_offset):
        from .signal.downconvert import input_dtype, input_is_complex
        if ddc.layout is not None:        # the recording's bytes as they are: whole frames (ValueError otherwise)
            n_in, n_out = ddc.layout.frames_in(ddc.layout.input_array(raw).nbytes), C.c_int64(0)
            status = call(self._h, ddc.handle, raw.ctypes.data, n_in, int(ring_offset), C.byref(n_out))
            if status:
                check(status)
            return n_out.value
        if not (isinstance(raw, np.ndarray) and raw.ndim == 1 and raw.flags.c_contiguous and raw.dtype == input_dtype(ddc.in_fmt)):
            raise ValueError("a push takes a contiguous 1-D array of raw inputs in the converter's input type")
        n_in = raw.size
        if input_is_complex(ddc.in_fmt):
            if n_in & 1:
                raise ValueError("interleaved IQ needs an even number of elements")
            n_in >>= 1
        n_out = C.c_int64(0)
        status = call(self._h, ddc.handle, raw.ctypes.data, n_in, int(ring_offset), C.byref(n_out))
        if status:
            check(status)
        return n_out.value

    def ddc_array_weights(self, ddc, weights):
        """The weights of an array converter from its next push on (sdr_ddc_array_weights; ordered on the stream)."""
        from .signal.array import as_weights
        w = as_weights(weights, ddc.n_elements or 1)
        flat = np.ascontiguousarray(np.stack([w.real, w.imag], axis=1))
        check(self._lib.sdr_ddc_array_weights(self._h, ddc.handle, flat.ctypes.data_as(C.POINTER(C.c_double))))

    def ddc_array_covariance(self, ddc, clear: bool = False):
        """(R [K][K] complex128, n) of an array converter made with `measure` (sdr_ddc_array_covariance; waits for the stream)."""
        K = max(ddc.n_elements, 1)
        R, n = np.zeros((K, K, 2)), C.c_int64(0)
        check(self._lib.sdr_ddc_array_covariance(self._h, ddc.handle, R.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n), int(bool(clear))))
        return R[..., 0] + 1j * R[..., 1], n.value

    def ddc_stap_weights(self, ddc, weights):
        """The [T][K] weights of a space-time converter from its next push on (sdr_ddc_stap_weights; ordered on the stream)."""
        from .signal.stap import as_weights
        w = as_weights(weights, ddc.n_taps or 1, ddc.n_elements or 1)
        flat = np.ascontiguousarray(np.stack([w.real, w.imag], axis=2))
        check(self._lib.sdr_ddc_stap_weights(self._h, ddc.handle, flat.ctypes.data_as(C.POINTER(C.c_double))))

    def ddc_stap_covariance(self, ddc, clear: bool = False):
        """(C [T][K][K] complex128, n) of a space-time converter made with `measure` (sdr_ddc_stap_covariance; waits for the
        stream)."""
        T, K = max(ddc.n_taps, 1), max(ddc.n_elements, 1)
        out, n = np.zeros((T, K, K, 2)), C.c_int64(0)
        check(self._lib.sdr_ddc_stap_covariance(self._h, ddc.handle, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n), int(bool(clear))))
        return out[..., 0] + 1j * out[..., 1], n.value

    def _beam_weights(self, ddc, weights):
        """A beam's weights in the converter's shape, [K] or [T][K], as the C-ABI's doubles."""
        if ddc.n_taps:
            from .signal.stap import as_weights
            w = as_weights(weights, ddc.n_taps, ddc.n_elements or 1)
        else:
            from .signal.array import as_weights
            w = as_weights(weights, ddc.n_elements or 1)
        return np.ascontiguousarray(np.stack([w.real, w.imag], axis=-1))

    def ddc_beam_attach(self, ddc, target_engine, weights) -> int:
        """A further beam of an array or space-time converter: `weights` in the converter's shape, the output into
        target_engine's ring (sdr_ddc_beam_attach; only before the converter's first input or after a reset) -> its index, 1 .."""
        flat, beam = self._beam_weights(ddc, weights), C.c_int(0)
        check(self._lib.sdr_ddc_beam_attach(self._h, ddc.handle, target_engine._h, flat.ctypes.data_as(C.POINTER(C.c_double)), C.byref(beam)))
        return beam.value

    def ddc_beam_weights(self, ddc, beam: int, weights):
        """The weights of attached beam `beam` >= 1 from the next push on (sdr_ddc_beam_weights; ordered on the stream)."""
        flat = self._beam_weights(ddc, weights)
        check(self._lib.sdr_ddc_beam_weights(self._h, ddc.handle, int(beam), flat.ctypes.data_as(C.POINTER(C.c_double))))

    def ddc_beam_count(self, ddc) -> int:
        """1 + the attached beams (sdr_ddc_beam_count)."""
        n = self._lib.sdr_ddc_beam_count(ddc.handle)
        if n < 0:
            check(int(n))
        return int(n)

    def ddc_beams_clear(self, ddc):
        """Release every attached beam (sdr_ddc_beams_clear; only before the converter's first input or after a reset)."""
        check(self._lib.sdr_ddc_beams_clear(self._h, ddc.handle))

    def ddc_push(self, ddc, raw: np.ndarray, ring_offset: int = 0) -> int:
        """Raw inputs (real: one integer each; complex: interleaved I,Q; a converter with a layout: the recording's bytes, whole
        frames, uint8 for packed fields and the field's type otherwise) through the converter into the ring at ring_offset
        (sdr_ddc_push, synchronous) -> the outputs written."""
        return self._ddc_push(self._lib.sdr_ddc_push, ddc, raw, ring_offset)

    def ddc_push_queue(self, ddc, raw: np.ndarray, ring_offset: int = 0) -> int:
        """ddc_push without the wait (sdr_ddc_push_queue): `raw` stays alive and unchanged until `sync()`."""
        return self._ddc_push(self._lib.sdr_ddc_push_queue, ddc, raw, ring_offset)

    def ddc_out_count(self, ddc, n_in: int) -> int:
        n = self._lib.sdr_ddc_out_count(ddc.handle, int(n_in))
        if n < 0:
            check(int(n))
        return int(n)

    def ddc_reset(self, ddc):
        check(self._lib.sdr_ddc_reset(self._h, ddc.handle))

    def ddc_mitigate(self, ddc, cfg):
        """Attach a pulse blanker / narrow-band excisor (sdr_ddc_mitigate) of a signal.mitigate.MitigationConfig to the
        converter, or detach it (cfg None); only before the converter's first input or after a reset."""
        if cfg is None:
            check(self._lib.sdr_ddc_mitigate(self._h, ddc.handle, None))
            ddc.nfft = 0
            return
        limit = np.ascontiguousarray(cfg.limit, dtype=np.float64) if cfg.nfft else None
        c = _lib.MitCfg(int(cfg.nfft), int(cfg.blank_lead), int(cfg.blank_hold), 0, float(cfg.blank_level),
                        limit.ctypes.data_as(C.POINTER(C.c_double)) if limit is not None else None)
        check(self._lib.sdr_ddc_mitigate(self._h, ddc.handle, C.byref(c)))
        ddc.nfft = int(cfg.nfft)

    def ddc_delay(self, ddc) -> int:
        """The attached mitigator's delay L in ring samples (sdr_ddc_delay); 0 without one."""
        n = self._lib.sdr_ddc_delay(ddc.handle)
        if n < 0:
            check(int(n))
        return int(n)

    def ddc_mitigation_stats(self, ddc):
        """The mitigator's counters (sdr_ddc_mitigation_stats) -> signal.mitigate.Stats."""
        from .signal.mitigate import Stats
        st = _lib.MitStats()
        bins = np.zeros(ddc.nfft, dtype=np.int64)
        check(self._lib.sdr_ddc_mitigation_stats(self._h, ddc.handle, C.byref(st), bins.ctypes.data if ddc.nfft else None))
        return Stats(st.n_outputs, st.n_triggers, st.n_blanked, st.n_segments, st.n_bins_excised, bins)

    def ddc_destroy(self, ddc):
        if ddc.handle:
            self._lib.sdr_ddc_destroy(self._h, ddc.handle)
            ddc.handle = None

    def host_alloc(self, n_elements: int, dtype=np.int8) -> np.ndarray:
        """Page-locked host memory as a NumPy array (sdr_host_alloc); `host_free(array)` gives it back -- the array must not
        be used afterwards."""
        dtype = np.dtype(dtype)
        block = C.c_void_p()
        check(self._lib.sdr_host_alloc(self._h, int(n_elements) * dtype.itemsize, C.byref(block)))
        buf = (C.c_char * (int(n_elements) * dtype.itemsize)).from_address(block.value)
        arr = np.frombuffer(buf, dtype=dtype)
        self._host_blocks[arr.ctypes.data] = block
        return arr

    def host_free(self, arr: np.ndarray):
        block = self._host_blocks.pop(arr.ctypes.data, None)
        if block is None:
            raise ValueError("not a block of host_alloc (or freed already)")
        check(self._lib.sdr_host_free(self._h, block))

    def iq_download(self, n_samples: int, ring_offset: int = 0) -> np.ndarray:
        out = np.empty(2 * int(n_samples), dtype=_lib.fmt_dtype(self.iq_fmt))
        check(self._lib.sdr_iq_download(self._h, ptr(out), int(n_samples), int(ring_offset)))
        return out

    def iq_probe(self, start: int, n_samples: int, nfft: int = 0, fs=None, hist: bool = True, hist_shift: int = 0):
        """What ring samples start .. start + n_samples - 1 hold (sdr_iq_probe): level statistics, with `hist` a histogram
        per component (integer rings), with `nfft` (a power of two in 64..4096) and `fs` a Welch spectrum -- one pass over
        the window on the device, behind every upload queued so far.  -> signal.probe.ProbeResult (the NumPy statement of the
        same: `signal.probe.probe`)."""
        from .signal.probe import HIST_BINS, ProbeResult
        res = _lib.ProbeResultC()
        nfft = int(nfft)
        table = np.zeros((2, HIST_BINS), dtype=np.int64) if hist else None
        psd = np.empty(max(0, min(nfft, 4096)), dtype=np.float64) if nfft else None
        check(self._lib.sdr_iq_probe(self._h, int(start), int(n_samples), int(hist_shift), nfft, float(fs) if fs is not None else 0.0,
                                     C.byref(res), ptr(table) if hist else None, ptr(psd) if nfft else None))
        return ProbeResult(res.n_samples, res.n_segments, res.n_nonfinite, tuple(res.n_rail), tuple(res.min), tuple(res.max),
                           tuple(res.sum), tuple(res.sum_sq), res.sum_iq, hist=table, psd=psd, fs=float(fs) if nfft else None)

    def iq_synth(self, sats, fs, noise_sigma, seed, first_sample, n_samples):
        arr = (SynthSat * max(1, len(sats)))()
        for i, s in enumerate(sats):
            arr[i].prn = int(s["slot"]) if "slot" in s else int(s["prn"])
            arr[i].flags = (1 if "slot" in s else 0) | (2 if s.get("boc") else 0)
            arr[i].doppler_hz = float(s["doppler"])
            arr[i].code_phase = float(s["code_phase"])
            arr[i].carrier_phase = float(s.get("phase", 0.0))
            arr[i].amplitude = float(s["amp"])
        check(self._lib.sdr_iq_synth(self._h, arr, len(sats), float(fs), float(noise_sigma), int(seed),
                                     int(first_sample), int(n_samples)))

    # ------------------------------------------------------------------ PRN replicas
    def code_slots(self, n_slots: int, max_chips: int = 1023, max_periods: int = 1):
        check(self._lib.sdr_code_slots_ex(self._h, int(n_slots), int(max_chips), int(max_periods)))
        self.n_slots, self.max_chips = int(n_slots), int(max_chips)
        self.code_generation = getattr(self, "code_generation", 0) + 1  # staged codes are gone

    def load_gps_code(self, slot: int, prn: int):
        check(self._lib.sdr_code_gps_l1ca(self._h, int(slot), int(prn)))

    def set_code(self, slot: int, chips):
        chips = np.ascontiguousarray(chips, dtype=np.int8)
        check(self._lib.sdr_code_custom(self._h, int(slot), ptr(chips), chips.size))

    def read_code(self, slot: int, max_chips: int = 65536) -> np.ndarray:
        out = np.empty(max_chips, dtype=np.int8)
        n = C.c_int(0)
        check(self._lib.sdr_code_read(self._h, int(slot), ptr(out), max_chips, C.byref(n)))
        return out[:n.value].copy()

    def upsample(self, slot: int, fs: float, n_samples: int) -> np.ndarray:
        out = np.empty(int(n_samples), dtype=np.int8)
        check(self._lib.sdr_code_upsample(self._h, int(slot), float(fs), int(n_samples), ptr(out)))
        return out

    # ------------------------------------------------------------------ correlators
    def epl_batch(self, items: np.ndarray, spacing, fs: float) -> np.ndarray:
        items = np.ascontiguousarray(items, dtype=EPL_ITEM_DTYPE)
        spacing = np.ascontiguousarray(spacing, dtype=np.float64)
        out = np.empty((len(items), 2 * len(spacing)), dtype=np.float64)
        check(self._lib.sdr_epl_batch(self._h, ptr(items), len(items), ptr(spacing), len(spacing), float(fs),
                                      ptr(out)))
        return out

    def corr_profile(self, items: np.ndarray, first: float, step: float, n_taps: int, fs: float) -> np.ndarray:
        """The correlation function on the tap grid first + step * arange(n_taps) [chips] (sdr_corr_profile): what
        `epl_batch` returns for every one of those spacings, in one pass over the samples -- any spacing, up to 1024 taps.
        `items` as for `epl_batch` (`make_items`).  -> float64[n_items, n_taps, 2] = I, Q."""
        items = np.ascontiguousarray(items, dtype=EPL_ITEM_DTYPE).reshape(-1)
        n_taps = int(n_taps)
        out = np.empty((len(items), max(0, min(n_taps, _lib.SDR_CORR_MAX_TAPS)), 2), dtype=np.float64)
        check(self._lib.sdr_corr_profile(self._h, ptr(items), len(items), float(first), float(step), n_taps, float(fs),
                                         ptr(out)))
        return out

    def ddm_bins(self, span_hz: float, step_hz: float) -> int:
        return int(self._lib.sdr_ddm_bins(float(span_hz), float(step_hz)))

    def ddm(self, items, fs, n_blocks, n_segments, first_chips, step_chips, n_taps, span_hz, step_hz, want_map=True,
            want_segments=False):
        """A delay-Doppler map around a known code phase and carrier (sdr_ddm; the NumPy statement is
        dsp.ddm.ddm_statement).  `items` as for `epl_batch` (`make_items`), read as predictions: start_sample, the whole
        window n_samples, the carrier, the NCO state at the start.  n_blocks non-coherent blocks of n_segments segments,
        taps first_chips + step_chips * arange(n_taps), frequencies carrier + (k - (K-1)/2) * step_hz within +-span_hz.
        -> (results (DDM_RESULT_DTYPE: peak_bin, peak_tap, peak_hz, peak_chips, peak_value, second_value, noise_mean),
        map[n][K][n_taps] or None, z[n][n_blocks*n_segments][n_taps] complex or None)."""
        items = np.ascontiguousarray(items, dtype=EPL_ITEM_DTYPE).reshape(-1)
        n = len(items)
        cfg = _lib.DdmCfg(float(fs), float(first_chips), float(step_chips), float(span_hz), float(step_hz), int(n_taps),
                          int(n_blocks), int(n_segments), 0)
        res = np.zeros(n, dtype=_lib.DDM_RESULT_DTYPE)
        taps = max(0, min(int(n_taps), _lib.SDR_CORR_MAX_TAPS))
        cmap = z = None
        if want_map:
            cmap = np.empty((n, max(0, self.ddm_bins(span_hz, step_hz)), taps), dtype=np.float64)
        if want_segments:
            q = max(0, int(n_blocks)) * max(0, int(n_segments))
            z = np.empty((n, q if q <= 4096 else 0, taps), dtype=np.complex128)
        check(self._lib.sdr_ddm(self._h, ptr(items), n, C.byref(cfg), ptr(res), ptr(cmap) if want_map else None,
                                ptr(z) if want_segments else None))
        return res, cmap, z

    def iq_cancel(self, items, amps=None, fs=None, window=None, dst=None, dst_offset=0) -> dict:
        """Subtract tracked signals' replicas from a window of the ring (sdr_iq_cancel; the NumPy statement is
        signal.cancel.cancel_statement).  items[n_ch][n_epochs] (`make_items` records; one row = one channel, epochs
        ascending, n_samples == 0 = padding), amps[n_ch][n_epochs][2] or complex [n_ch][n_epochs] -- None: each epoch's
        prompt over its n_samples (`epl_batch` on this ring, signal.cancel.amplitudes_from_prompts).  window = (start,
        samples) -- None: the hull of the items.  dst None: in place; another Engine on this device (or this one, with a
        window that shares no sample with the source's): the cancelled window goes to its ring at dst_offset and this ring
        stays as it is.  -> the counters of sdr_cancel_stats as a dict."""
        from .signal import cancel as _cancel
        if fs is None:
            raise TypeError("iq_cancel needs the sampling frequency fs")
        items = np.ascontiguousarray(np.atleast_2d(np.asarray(items, dtype=EPL_ITEM_DTYPE)))
        n_ch, n_epochs = items.shape
        if amps is None:
            flat = items.reshape(-1)
            live = flat["n_samples"] > 0
            prompts = np.zeros((flat.size, 2), dtype=np.float64)
            if live.any():
                prompts[live] = self.epl_batch(flat[live], [0.0], fs)
            amps = _cancel.amplitudes_from_prompts(prompts, flat["n_samples"])
        amps = np.asarray(amps)
        if np.iscomplexobj(amps):
            amps = np.stack([amps.real, amps.imag], axis=-1)
        amps = np.ascontiguousarray(amps, dtype=np.float64)
        if amps.size != 2 * items.size:
            raise ValueError(f"amps of {amps.shape} for items of {items.shape}")
        w0, W = _cancel.hull(items) if window is None else (int(window[0]), int(window[1]))
        in_place = dst is None
        stats = _lib.CancelStats()
        check(self._lib.sdr_iq_cancel(self._h, ptr(items), ptr(amps), n_ch, n_epochs, float(fs), w0, W,
                                      None if in_place else dst._h, w0 if in_place else int(dst_offset), C.byref(stats)))
        return dict(samples_written=stats.samples_written, samples_changed=stats.samples_changed,
                    clipped_components=stats.clipped_components)

    def epl_plan_dev(self, device_items: int, n_items: int, spacing, fs) -> EplPlan:
        """A plan of n_items items that are already in device memory at address device_items."""
        return EplPlan(self, None, spacing, fs, device_items=device_items, n_items=n_items)

    def epl_plan(self, items, spacing, fs) -> EplPlan:
        return EplPlan(self, items, spacing, fs)

    # ------------------------------------------------------------------ acquisition
    def pcps(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh=1, noncoh=1,
             want_map=False):
        slots = np.ascontiguousarray(code_slots, dtype=np.int32)
        n = len(slots)
        nbins = self._lib.sdr_pcps_bins(float(doppler_range), float(doppler_step))
        n_code = int(round(fs * 1023 / 1.023e6))
        pb = np.empty(n, dtype=np.int64)
        pc = np.empty(n, dtype=np.int64)
        pr = np.empty(n, dtype=np.float64)
        cmap = np.empty((n, nbins, n_code), dtype=np.float64) if want_map else None
        nb = C.c_int(0)
        check(self._lib.sdr_pcps(self._h, ptr(slots), n, int(start_sample), float(fs), float(if_hz),
                                 float(doppler_range), float(doppler_step), int(coh), int(noncoh), ptr(pb),
                                 ptr(pc), ptr(pr), ptr(cmap) if want_map else None, C.byref(nb)))
        return pb, pc, pr, cmap

    def pcps_spectra(self, code_spectra, start_sample, fs, if_hz, doppler_range, doppler_step, coh=1, noncoh=1,
                     want_map=True):
        """PCPS with caller-supplied codeFFT rows (complex128 [n_prn][n_code]) -- the reference's PCPS() signature."""
        spec = np.ascontiguousarray(np.atleast_2d(code_spectra), dtype=np.complex128)
        n, n_code = spec.shape
        nbins = self._lib.sdr_pcps_bins(float(doppler_range), float(doppler_step))
        pb = np.empty(n, dtype=np.int64)
        pc = np.empty(n, dtype=np.int64)
        pr = np.empty(n, dtype=np.float64)
        cmap = np.empty((n, nbins, n_code), dtype=np.float64) if want_map else None
        nb = C.c_int(0)
        check(self._lib.sdr_pcps_spectra(self._h, ptr(spec), n, n_code, int(start_sample), float(fs), float(if_hz),
                                         float(doppler_range), float(doppler_step), int(coh), int(noncoh), ptr(pb),
                                         ptr(pc), ptr(pr), ptr(cmap) if want_map else None, C.byref(nb)))
        return pb, pc, pr, cmap

    def pcps_signal(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, chip_rate_hz, pad=0,
                    excl_samples=0, coh=1, noncoh=1, want_map=False, n_chips=None, reserved=(0, 0)):
        """PCPS for any staged code (sdr_pcps_signal; the NumPy statement is dsp.signalsearch.pcps_signal_statement): the
        slots' codes, all of one length, at `chip_rate_hz`; pad = 1 searches zero-padded over two code periods (coh = 1),
        `excl_samples` is the second peak's exclusion half-width (0: round(fs / chip_rate_hz)).  `n_chips`: the slots' code
        length where a map is wanted (None: read back from the first slot).
        -> (peak_bin, peak_code, peak_ratio, map[n_prn][bins][N] or None)."""
        slots = np.ascontiguousarray(code_slots, dtype=np.int32)
        n = len(slots)
        sig = _lib.AcqSignal(float(chip_rate_hz), int(pad), int(excl_samples), (C.c_int32 * 2)(int(reserved[0]), int(reserved[1])))
        nbins = self._lib.sdr_pcps_bins(float(doppler_range), float(doppler_step))
        cmap = None
        if want_map:
            if n_chips is None:
                n_chips = len(self.read_code(int(slots[0]))) if n else 0
            ratio = float(fs) * int(n_chips) / float(chip_rate_hz) if chip_rate_hz and chip_rate_hz > 0 else 0.0
            n_code = int(np.rint(ratio)) if np.isfinite(ratio) and 0 <= ratio <= 1 << 24 else 0
            cmap = np.empty((n, max(0, nbins), n_code), dtype=np.float64)
        pb, pc, pr = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float64)
        nb, nc = C.c_int(0), C.c_int(0)
        check(self._lib.sdr_pcps_signal(self._h, C.byref(sig), ptr(slots), n, int(start_sample), float(fs), float(if_hz),
                                        float(doppler_range), float(doppler_step), int(coh), int(noncoh), ptr(pb), ptr(pc),
                                        ptr(pr), ptr(cmap) if want_map else None, C.byref(nb), C.byref(nc)))
        if want_map and cmap.shape[2] != nc.value:
            raise ValueError(f"map of {cmap.shape[2]} columns allocated, the search wrote {nc.value}")
        return pb, pc, pr, cmap

    def serial_search(self, code_slots, start_sample, fs, doppler_range, doppler_step, noncoh=1, want_map=False,
                      n_chips=None):
        """SerialSearch (sdr_serial_search) of the slots' codes, all of one length.  `n_chips`: that length where a map is
        wanted (None: read back from the first slot; a value that disagrees with the slot raises ValueError, since the
        library writes map[n_prn][bins][L] with the staged length L).
        -> (peak_bin, peak_code, peak_ratio, map[n_prn][bins][L] or None)."""
        slots = np.ascontiguousarray(code_slots, dtype=np.int32)
        n = len(slots)
        nbins = self._lib.sdr_pcps_bins(float(doppler_range), float(doppler_step))
        pb, pc, pr = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.float64)
        cmap = None
        if want_map:
            try:
                staged = len(self.read_code(int(slots[0]))) if n else 0
            except _lib.SdrError:       # (no such slot, nothing staged: the search itself says what is wrong)
                staged = 0
            if n_chips is not None and staged and int(n_chips) != staged:
                raise ValueError(f"n_chips = {int(n_chips)}, code slot {int(slots[0])} holds {staged} chips")
            cmap = np.empty((n, max(0, nbins), staged), dtype=np.float64)
        nb = C.c_int(0)
        check(self._lib.sdr_serial_search(self._h, ptr(slots), n, int(start_sample), float(fs), float(doppler_range),
                                          float(doppler_step), int(noncoh), ptr(pb), ptr(pc), ptr(pr),
                                          ptr(cmap) if want_map else None, C.byref(nb)))
        return pb, pc, pr, cmap

    def acq_refine_bins(self, span_hz: float, step_hz: float) -> int:
        return int(self._lib.sdr_acq_refine_bins(float(span_hz), float(step_hz)))

    def acq_refine(self, items, fs, n_periods=10, n_segments=8, span_hz=125.0, step_hz=5.0, want_tables=False):
        """Fine carrier frequency and bit edge behind an acquisition (sdr_acq_refine): `items` = sdr_refine_item records
        (REFINE_ITEM_DTYPE, see `make_refine_items`) -- one call for all of them.  -> results (REFINE_RESULT_DTYPE:
        fine_hz, power, power_no_edge, fine_idx, bit_edge), and with want_tables also (power[n][n_periods][K],
        segment_sums[n][n_periods][n_segments] complex)."""
        items = np.ascontiguousarray(items, dtype=REFINE_ITEM_DTYPE).reshape(-1)
        n = len(items)
        res = np.zeros(n, dtype=REFINE_RESULT_DTYPE)
        power = z = None
        if want_tables:
            k = max(0, self.acq_refine_bins(span_hz, step_hz))
            power = np.empty((n, max(0, int(n_periods)), k), dtype=np.float64)
            z = np.empty((n, max(0, int(n_periods)), max(0, int(n_segments))), dtype=np.complex128)
        check(self._lib.sdr_acq_refine(self._h, ptr(items), n, float(fs), int(n_periods), int(n_segments), float(span_hz),
                                       float(step_hz), ptr(res), ptr(power) if want_tables else None,
                                       ptr(z) if want_tables else None))
        return (res, power, z) if want_tables else res

    def acq_secondary(self, items, sec_codes, fs, n_periods, n_segments=4, span_hz=125.0, step_hz=5.0, mode=0, want_tables=False):
        """Secondary-code phase and fine carrier frequency behind an acquisition (sdr_acq_secondary): `items` = sdr_sec_item
        records (SEC_ITEM_DTYPE, see `make_secondary_items`), `sec_codes` = the +-1 secondary codes, one per row (a single
        code may be given as one row) -- one call for all items.  mode 0: a pilot, 1: a data symbol as long as the secondary
        period.  -> results (SEC_RESULT_DTYPE: fine_hz, power, power_other, prompt_re, prompt_im, fine_idx, sec_phase), and
        with want_tables also (power[n][sec_len][K], segment_sums[n][n_periods][n_segments] complex)."""
        items = np.ascontiguousarray(items, dtype=SEC_ITEM_DTYPE).reshape(-1)
        sec = np.asarray(sec_codes)
        if sec.ndim != 2:
            sec = sec.reshape(1, -1)
        if not np.array_equal(sec, sec.astype(np.int8)):
            raise ValueError("secondary chips are +1 or -1")
        sec = np.ascontiguousarray(sec, dtype=np.int8)
        n = len(items)
        res = np.zeros(n, dtype=SEC_RESULT_DTYPE)
        power = z = None
        if want_tables:
            k = max(0, self.acq_refine_bins(span_hz, step_hz))
            power = np.empty((n, sec.shape[1], k), dtype=np.float64)
            z = np.empty((n, max(0, int(n_periods)), max(0, int(n_segments))), dtype=np.complex128)
        check(self._lib.sdr_acq_secondary(self._h, ptr(items), n, ptr(sec), sec.shape[0], sec.shape[1], float(fs), int(n_periods),
                                          int(n_segments), float(span_hz), float(step_hz), int(mode), ptr(res),
                                          ptr(power) if want_tables else None, ptr(z) if want_tables else None))
        return (res, power, z) if want_tables else res

    def pcps_coherent(self, code_slots, sec_rows, sec_codes, start_sample, fs, if_hz, doppler_range, doppler_step, chip_rate_hz,
                      n_periods, span_hz=125.0, step_hz=25.0, mode=0, excl_samples=0, want_map=False, want_power=False,
                      n_chips=None, reserved=(0, 0)):
        """The coherent search under secondary-code hypotheses (sdr_pcps_coherent; the NumPy statement is
        dsp.signalsearch.pcps_coherent_statement): the slots' codes, all of one length, at `chip_rate_hz`, each under its row
        `sec_rows[p]` of the +-1 overlay codes `sec_codes` (a single code may be given as one row); `n_periods` code periods
        are added coherently under every overlay phase and every frequency of the fine grid (span_hz, step_hz).  mode 0: a
        pilot, 1: a data symbol as long as the overlay code.  `n_chips`: the slots' code length where a map is wanted (None:
        read back from the first slot).
        -> (results: COH_RESULT_DTYPE records -- carrier_hz, peak, peak_ratio, power, power_other, prompt_re, prompt_im,
        peak_code, peak_bin, fine_idx, sec_phase --, R[n_prn][bins][N] or None, power[n_prn][sec_len][K] or None)."""
        slots = np.ascontiguousarray(code_slots, dtype=np.int32)
        n = len(slots)
        rows = np.ascontiguousarray(np.broadcast_to(np.asarray(sec_rows, dtype=np.int32), (n,)))
        sec = np.asarray(sec_codes)
        if sec.ndim != 2:
            sec = sec.reshape(1, -1)
        if not np.array_equal(sec, sec.astype(np.int8)):
            raise ValueError("secondary chips are +1 or -1")
        sec = np.ascontiguousarray(sec, dtype=np.int8)
        cfg = _lib.CohCfg(float(chip_rate_hz), float(span_hz), float(step_hz), int(n_periods), sec.shape[1], int(mode),
                          int(excl_samples), (C.c_int32 * 2)(int(reserved[0]), int(reserved[1])))
        nbins = self._lib.sdr_pcps_bins(float(doppler_range), float(doppler_step))
        cmap = power = None
        if want_map:
            if n_chips is None:
                n_chips = len(self.read_code(int(slots[0]))) if n else 0
            ratio = float(fs) * int(n_chips) / float(chip_rate_hz) if chip_rate_hz and chip_rate_hz > 0 else 0.0
            n_code = int(np.rint(ratio)) if np.isfinite(ratio) and 0 <= ratio <= 1 << 24 else 0
            cmap = np.empty((n, max(0, nbins), n_code), dtype=np.float64)
        if want_power:
            power = np.empty((n, sec.shape[1], max(0, self.acq_refine_bins(span_hz, step_hz))), dtype=np.float64)
        res = np.zeros(n, dtype=COH_RESULT_DTYPE)
        nb, nc = C.c_int(0), C.c_int(0)
        check(self._lib.sdr_pcps_coherent(self._h, C.byref(cfg), ptr(slots), ptr(rows), n, ptr(sec), sec.shape[0], int(start_sample),
                                          float(fs), float(if_hz), float(doppler_range), float(doppler_step), ptr(res),
                                          ptr(cmap) if want_map else None, ptr(power) if want_power else None, C.byref(nb),
                                          C.byref(nc)))
        if want_map and cmap.shape[2] != nc.value:
            raise ValueError(f"map of {cmap.shape[2]} columns allocated, the search wrote {nc.value}")
        return res, cmap, power

    def acq_deep(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh, groups=1,
                 carrier_rf_hz=0.0, want_map=False):
        """The deep search (sdr_acq_deep): coherent blocks of `coh` code periods folded in front of one transform, `noncoh`
        blocks added into `groups` bit-edge groups at the code-Doppler shift `carrier_rf_hz` gives (0: none).
        -> (results: DEEP_RESULT_DTYPE records -- peak_bin, peak_code, peak_code_end, peak_group, peak_ratio, peak_value --
        one per slot, map float64[n][groups][bins][N] or None)."""
        slots = np.ascontiguousarray(code_slots, dtype=np.int32)
        n = len(slots)
        cfg = _lib.DeepCfg(float(fs), float(if_hz), float(doppler_range), float(doppler_step), float(carrier_rf_hz),
                           int(coh), int(noncoh), int(groups), 0)
        res = np.zeros(n, dtype=_lib.DEEP_RESULT_DTYPE)
        cmap = None
        if want_map:
            nbins = max(0, self._lib.sdr_pcps_bins(float(doppler_range), float(doppler_step)))
            cmap = np.empty((n, max(0, int(groups)), nbins, int(round(fs * 1023 / 1.023e6))), dtype=np.float64)
        check(self._lib.sdr_acq_deep(self._h, ptr(slots), n, int(start_sample), C.byref(cfg), ptr(res),
                                     ptr(cmap) if want_map else None))
        return res, cmap

    def acq_deep_detect(self, code_slots, start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh, groups=1,
                        carrier_rf_hz=0.0, n_peaks=1, excl_code=0, excl_bins=0, want_map=False):
        """The deep search with detection statistics made on the resident maps (sdr_acq_deep_detect): the `n_peaks`
        strongest peaks that lie outside each other's zones (`excl_code` samples circularly, `excl_bins` bins) and the
        count, mean and variance of the cells whose code column is clear of every peak.
        -> (results as `acq_deep`, peaks: DETECT_PEAK_DTYPE[n][n_peaks] -- bin, code, code_end, group, value, z --,
        noise: DETECT_NOISE_DTYPE[n] -- n_cells, mean, variance --, map or None)."""
        slots = np.ascontiguousarray(code_slots, dtype=np.int32)
        n = len(slots)
        cfg = _lib.DeepCfg(float(fs), float(if_hz), float(doppler_range), float(doppler_step), float(carrier_rf_hz),
                           int(coh), int(noncoh), int(groups), 0)
        det = _lib.DetectCfg(int(n_peaks), int(excl_code), int(excl_bins), 0)
        res = np.zeros(n, dtype=_lib.DEEP_RESULT_DTYPE)
        peaks = np.zeros((n, max(0, min(int(n_peaks), 8))), dtype=_lib.DETECT_PEAK_DTYPE)
        noise = np.zeros(n, dtype=_lib.DETECT_NOISE_DTYPE)
        cmap = None
        if want_map:
            nbins = max(0, self._lib.sdr_pcps_bins(float(doppler_range), float(doppler_step)))
            cmap = np.empty((n, max(0, int(groups)), nbins, int(round(fs * 1023 / 1.023e6))), dtype=np.float64)
        check(self._lib.sdr_acq_deep_detect(self._h, ptr(slots), n, int(start_sample), C.byref(cfg), C.byref(det), ptr(res),
                                            ptr(peaks), ptr(noise), ptr(cmap) if want_map else None))
        return res, peaks, noise, cmap

    def two_peak_compare_ss(self, cmap: np.ndarray):
        cmap = np.ascontiguousarray(cmap, dtype=np.float64)
        pb, pc, pr = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(self._lib.sdr_two_peak_compare_ss(self._h, ptr(cmap), cmap.shape[0], cmap.shape[1], C.byref(pb),
                                                C.byref(pc), C.byref(pr)))
        return [pb.value, pc.value], pr.value

    def two_peak_compare(self, cmap: np.ndarray, samples_per_chip: int):
        cmap = np.ascontiguousarray(cmap, dtype=np.float64)
        pb, pc, pr = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(self._lib.sdr_two_peak_compare(self._h, ptr(cmap), cmap.shape[0], cmap.shape[1],
                                             int(samples_per_chip), C.byref(pb), C.byref(pc), C.byref(pr)))
        return [pb.value, pc.value], pr.value

    # ------------------------------------------------------------------ closed loop
    def track_cluster(self, parts: int = 0):
        """Workgroups cooperating on one channel in `track_closed_loop` (0 = fill the GPU; 1, 2, 4, 8)."""
        check(self._lib.sdr_track_cluster(self._h, int(parts)))

    def tick_server_stats(self) -> dict:
        """The resident tick server of this engine (set_option("tick_server", 1)): is one resident now, requests answered,
        servers started, and whether the engine went back to plain ticks for good (a launch refused, a server that died)."""
        out = (C.c_int64 * 4)()
        check(self._lib.sdr_tick_server_stats(self._h, out))
        ph = (C.c_double * 4)()
        check(self._lib.sdr_tick_server_phases(self._h, ph))
        return {"running": bool(out[0]), "served": int(out[1]), "starts": int(out[2]), "disabled": bool(out[3]),
                "device_us_total": {"slab": ph[0], "release": ph[1], "channels": ph[2], "gather": ph[3]},
                "channel0_us_total": dict(zip(("release_seen", "samples_visible", "correlated", "exchanged", "updated", "answered"),
                                              self._tracker_phases()))}

    def _tracker_phases(self):
        t = (C.c_double * 6)()
        check(self._lib.sdr_tick_server_tracker_phases(self._h, t))
        return list(t)

    def stream_create(self) -> int:
        """A further HIP stream of this engine (north_star: one stream per channel batch); 0 is the default one."""
        sid = C.c_int(0)
        check(self._lib.sdr_stream_create(self._h, C.byref(sid)))
        return sid.value

    def stream_sync(self, stream: int = 0):
        check(self._lib.sdr_stream_sync(self._h, int(stream)))

    def bank(self, max_channels: int) -> Bank:
        return Bank(self, max_channels)

    def track_closed_loop_ex(self, states, cfgs, n_epochs: int, want_traj=True, want_bits=False, epochs_per_bit=20):
        """Per-channel outcome: -> (end states, trajectory or None, bits or None, epochs_done[n_ch]).  `cfgs`: one
        LoopCfg for all channels or a sequence with one per channel."""
        n_ch = len(states)
        arr = (TrackState * n_ch)(*states)
        per_channel = not isinstance(cfgs, LoopCfg)
        carr = (LoopCfg * n_ch)(*cfgs) if per_channel else (LoopCfg * 1)(cfgs)
        traj = np.zeros((n_ch, n_epochs), dtype=TRACK_EPOCH_DTYPE) if want_traj else None
        max_bits = n_epochs // max(1, int(epochs_per_bit)) + 2
        bits = np.zeros((n_ch, max_bits), dtype=np.int8) if want_bits else None
        n_bits = np.zeros(n_ch, dtype=np.int32) if want_bits else None
        done = np.zeros(n_ch, dtype=np.int32)
        check(self._lib.sdr_track_closed_loop_ex(self._h, n_ch, arr, carr, 1 if per_channel else 0, int(n_epochs),
                                                 ptr(traj) if want_traj else None, ptr(bits) if want_bits else None,
                                                 max_bits if want_bits else 0, ptr(n_bits) if want_bits else None,
                                                 ptr(done)))
        nav = [bits[c, :n_bits[c]].copy() for c in range(n_ch)] if want_bits else None
        return list(arr), traj, nav, done

    def track_closed_loop(self, states, cfg: LoopCfg, n_epochs: int, want_traj=True, want_bits=False):
        """Returns (end states, trajectory or None[, list of per-channel nav-bit arrays])."""
        n_ch = len(states)
        arr = (TrackState * n_ch)(*states)
        traj = np.zeros((n_ch, n_epochs), dtype=TRACK_EPOCH_DTYPE) if want_traj else None
        if not want_bits:
            check(self._lib.sdr_track_closed_loop(self._h, n_ch, arr, C.byref(cfg), int(n_epochs),
                                                  ptr(traj) if want_traj else None))
            return list(arr), traj
        max_bits = n_epochs // 20 + 2
        bits = np.zeros((n_ch, max_bits), dtype=np.int8)
        n_bits = np.zeros(n_ch, dtype=np.int32)
        check(self._lib.sdr_track_closed_loop_bits(self._h, n_ch, arr, C.byref(cfg), int(n_epochs),
                                                   ptr(traj) if want_traj else None, ptr(bits), max_bits, ptr(n_bits)))
        return list(arr), traj, [bits[c, :n_bits[c]].copy() for c in range(n_ch)]
