"""Packed 1-, 2- and 4-bit I,Q widened on the device (sdr_iq_upload_packed / _begin / _queue): after a packed upload the
ring equals, byte for byte, the ring after the host unpacks (sydr_amd/signal/packing.py) and uploads the ordinary way --
whatever the width, field order, table, route, length, offset or source address; and everything downstream of the ring
(correlator plans fed chunk by chunk, a receiver over a packed file) gives the bits the unpacked samples give."""
import ctypes as C

import numpy as np
import pytest

import packed_cases as cases

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CI8, FMT_CI16, Engine
from sydr_amd.signal import packing as pk
from sydr_amd.utils.enumerations import ChannelMessage

pytestmark = pytest.mark.gpu

# (begin_copy_command: `_begin` under the option "ingest_by_copy_command" -- the staged slab goes into HBM by a copy command)
ROUTES = ["sync", "begin_staged", "begin_in_place", "queue_pageable", "queue_page_locked", "begin_copy_command"]
INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6


def hostile_table(rng, bits):
    levels = rng.choice(np.arange(-127, 127), (1 << bits) - 2, replace=False).tolist() + [-128, 127]
    return [int(v) for v in rng.permutation(levels)]


# ------------------------------------------------------------------------------------------------ 1. ring equality
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("msb", [False, True])
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_ring_after_a_packed_upload_equals_the_host_unpack(engine, bits, msb, route):
    rng = np.random.default_rng(1000 * bits + 100 * msb + ROUTES.index(route))
    cap = 1 << 16
    spb = 4 // bits
    engine.iq_alloc(cap, FMT_CI8)
    mirror = rng.integers(-128, 128, 2 * cap).astype(np.int8)          # a ring full of other data
    engine.iq_upload(mirror, 0)
    pinned = engine.host_alloc(2 * cap * bits // 8 + 64, np.uint8)
    engine.set_option("ingest_by_copy_command", 1 if route == "begin_copy_command" else 0)
    try:
        for k in range(40):
            p = pk.Packing(bits, hostile_table(rng, bits), msb_first=msb)
            n = spb * int(rng.integers(1, 3000 // spb))
            if k == 7:
                n = spb
            if k == 23:
                n = cap
            off = int(rng.integers(0, cap)) if k % 3 else cap - int(rng.integers(1, n + 1))   # (every third across the ring's end)
            shift = 1 + 2 * int(rng.integers(0, 8))                     # the source at an odd byte address
            if k % 2 == 0 and n >= 8:                                   # every other one whole granules: the dwordx4 kernel ...
                n, off = n // 8 * 8, off // 8 * 8
                if route == "begin_in_place":                           # ... which reads a 16-byte aligned block in place
                    shift = 16 * int(rng.integers(0, 4))
            if k == 11:
                off += 5 * cap                                          # (any offset >= 0, taken modulo the capacity)
            nbytes = pk.packed_bytes(p, n)
            data = rng.integers(0, 256, nbytes).astype(np.uint8)
            if route in ("begin_in_place", "queue_page_locked"):
                src = pinned[shift:shift + nbytes]
                src[:] = data
            else:
                src = np.empty(nbytes + 16, dtype=np.uint8)[shift:shift + nbytes]
                src[:] = data
            assert src.ctypes.data % 2 == 1 or (route == "begin_in_place" and k % 2 == 0)
            if route == "sync":
                engine.iq_upload_packed(src, n, p, off)
            elif route.startswith("begin"):
                engine.iq_upload_packed_begin(src, n, p, off)
                if route != "begin_in_place":
                    src[:] = 0                                          # copied before the call returned
                engine.sync()
            else:
                engine.iq_upload_packed_queue(src, n, p, off)
                engine.sync()
            idx = (2 * off + np.arange(2 * n)) % (2 * cap)
            mirror[idx] = pk.unpack(data, p)
            if k % 4 == 0 or k in (7, 23):
                assert np.array_equal(engine.iq_download(cap, 0), mirror), (k, n, off)   # the WHOLE ring: its surroundings too
        assert np.array_equal(engine.iq_download(cap, 0), mirror)
    finally:
        engine.set_option("ingest_by_copy_command", 0)
        engine.host_free(pinned)


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_packed_uploads_refuse_what_they_cannot_take(engine):
    lib, h = engine._lib, engine._h
    cap = 4096
    engine.iq_alloc(cap, FMT_CI8)
    buf = np.zeros(4 * cap, dtype=np.uint8)
    calls = [lib.sdr_iq_upload_packed, lib.sdr_iq_upload_packed_begin, lib.sdr_iq_upload_packed_queue]
    good = _lib.IqPacking(2, 0)
    for call in calls:
        assert call(h, C.byref(good), buf.ctypes.data, 64, 0) == 0
        assert call(None, C.byref(good), buf.ctypes.data, 64, 0) == INVALID
        assert call(h, None, buf.ctypes.data, 64, 0) == INVALID
        assert call(h, C.byref(good), None, 64, 0) == INVALID
        for bits in (0, 3, 8, 16):
            assert call(h, C.byref(_lib.IqPacking(bits, 0)), buf.ctypes.data, 64, 0) == INVALID
        assert call(h, C.byref(_lib.IqPacking(2, 2)), buf.ctypes.data, 64, 0) == INVALID     # unknown flag bits
        assert call(h, C.byref(_lib.IqPacking(2, 1)), buf.ctypes.data, 64, 0) == 0           # SDR_PACK_MSB_FIRST
        assert call(h, C.byref(good), buf.ctypes.data, 63, 0) == INVALID                     # two samples to a byte
        assert call(h, C.byref(_lib.IqPacking(1, 0)), buf.ctypes.data, 6, 0) == INVALID      # four samples to a byte
        assert call(h, C.byref(good), buf.ctypes.data, cap + 2, 0) == RANGE
        assert call(h, C.byref(good), buf.ctypes.data, -2, 0) == RANGE
        assert call(h, C.byref(good), buf.ctypes.data, 64, -1) == RANGE
        assert call(h, C.byref(good), buf.ctypes.data, cap, 3 * cap + 5) == 0                # any offset >= 0, n up to the capacity
    engine.sync()
    # through the Python layer: the status travels in the exception; lengths and dtypes are checked before the call
    with pytest.raises(SdrError) as err:
        engine.iq_upload_packed(buf[:16], 63, pk.Packing(2), 0)
    assert err.value.status == INVALID
    with pytest.raises(ValueError):
        engine.iq_upload_packed(buf[:31], 64, pk.Packing(2), 0)
    with pytest.raises(ValueError):
        engine.iq_upload_packed_queue(buf[:32].astype(np.int8), 64, pk.Packing(2), 0)
    with pytest.raises(ValueError):
        engine.iq_upload_packed_begin(buf[:64:2], 64, pk.Packing(2), 0)
    engine.iq_alloc(cap, FMT_CI16)
    for call in calls:
        assert call(h, C.byref(good), buf.ctypes.data, 64, 0) == UNSUPPORTED
    with pytest.raises(SdrError) as err:
        engine.iq_upload_packed(buf[:32], 64, pk.Packing(2), 0)
    assert err.value.status == UNSUPPORTED
    e2 = Engine(0)
    try:
        assert lib.sdr_iq_upload_packed(e2._h, C.byref(good), buf.ctypes.data, 64, 0) == STATE   # no ring yet
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ 3. beside a correlating stream
@pytest.mark.parametrize("pageable", [False, True])
@pytest.mark.parametrize("bits", [2, 4])
def test_packed_chunks_queued_from_the_host_equal_the_one_launch_pass(engine, tmp_path, bits, pageable):
    """tests/test_gpu_hostfed.py's first test with packed chunks: a chunk at a time through sdr_iq_upload_packed_queue while
    another stream correlates the chunk before; outputs equal to the one-launch pass over the same samples uploaded unpacked."""
    fs, n_ch, chunk = 25e6, 8, 200_000
    total = 12 * chunk
    rng = np.random.default_rng(6160 + 10 * bits + pageable)
    p = pk.Packing(bits, msb_first=bool(pageable))
    packed = rng.integers(0, 256, pk.packed_bytes(p, total)).astype(np.uint8)
    raw = pk.unpack(packed, p)
    engine.iq_alloc(total, FMT_CI8)
    engine.code_slots(n_ch)
    for c in range(n_ch):
        engine.load_gps_code(c, 3 + c)
    items, n_epochs = cases.epoch_items(fs, n_ch, total, rng)
    spacing = (-0.5, 0.0, 0.5)
    engine.iq_upload(raw, 0)
    plan = engine.epl_plan(items, spacing, fs)
    plan.run()
    want = plan.fetch().copy()
    variant = plan.variant
    plan.close()
    assert variant & 0xF00                                   # (a straight-line kernel: reads the flipped ring image)
    if pageable:
        path = tmp_path / "recording.packed"
        packed.tofile(path)
        source = np.asarray(np.memmap(path, dtype=np.uint8, mode="r"))
    else:
        source = engine.host_alloc(packed.size, np.uint8)
        source[:] = packed
    per_chunk = pk.packed_bytes(p, chunk)
    try:
        engine.iq_alloc(total, FMT_CI8)
        assert not engine.iq_download(4096, 0).any()
        plan = engine.epl_plan(items, spacing, fs)
        batch = engine.stream_create()
        ends = (items["start_sample"] + items["n_samples"]).reshape(n_epochs, n_ch).max(axis=1)
        done = 0
        for k in range(total // chunk):
            engine.iq_upload_packed_queue(source[k * per_chunk:(k + 1) * per_chunk], chunk, p, k * chunk)
            upto = int(np.searchsorted(ends, (k + 1) * chunk, side="right")) * n_ch
            if upto > done:
                plan.run(done, upto - done, stream=batch)
                done = upto
        engine.stream_sync(batch)
        engine.sync()
        assert done == len(items)
        assert plan.fetch().tobytes() == want.tobytes()
        assert np.array_equal(engine.iq_download(total, 0), raw)
        plan.close()
    finally:
        if not pageable:
            engine.host_free(source)


# ------------------------------------------------------------------------------------------------ 4. end to end
def test_receiver_over_a_packed_file_equals_the_same_levels_as_int8(engine, tmp_path):
    """The synthetic stream of tests/test_gpu_bank.py's read-ahead test (twelve satellites, amplitude 5, noise 10, 10 MHz),
    quantised to 2 bits at one standard deviation of the composite, written packed and as int8 of the same levels:
    ChannelManager over both files on the device -- plain ticks, runBlock, read-ahead, four satellites joining late -- gives
    equal packets bit for bit, acquisition included; with the tick server switched on, equal packets again and no request
    answered (packed ticks take the plain path)."""
    fs, n_ms = 10e6, 400
    spms = int(fs * 1e-3)
    rng = np.random.default_rng(5050)
    sats = [dict(prn=1 + c, doppler=float(250.0 * rng.integers(-15, 16) + rng.uniform(-40, 40)),
                 code_phase=float(rng.uniform(0, 1023)), phase=float(rng.uniform(0, 1)), amp=5.0) for c in range(12)]
    total = n_ms * spms
    engine.iq_alloc(total, FMT_CI8)
    engine.code_slots(32)
    engine.iq_synth(sats, fs, 10.0, 5051, 0, total)
    raw = engine.iq_download(total, 0)
    sigma = float(raw.astype(np.float64).std())
    packed2, plain2, packing2, few2 = cases.write_both(tmp_path, raw, 2, sigma)
    cfg = cases.kaplan_config()
    prns, late_prns = [s["prn"] for s in sats[:8]], [s["prn"] for s in sats[8:]]

    def receiver(path, data_size, mode, server=False):
        engine.set_option("tick_server", 1 if server else 0)
        try:
            # (four satellites join at tick 150 -- tick 50 where the ticks end at 100 and a block follows)
            ticks, mgr = cases.receive(cases.signal(path, fs, data_size), engine, prns, cfg, n_ms, mode,
                                       late=(50 if mode == "block" else 150, late_prns), ring_ms=600 if mode == "block" else 100, keep_map=False)
            stats = engine.tick_server_stats()
            mgr.close()
        finally:
            engine.set_option("tick_server", 0)
        return ticks, stats

    cn0 = lambda ticks: {p["cid"]: p["cn0"] for t in ticks for p in t if p["type"] is ChannelMessage.TRACKING_UPDATE}
    for mode in ("ticks", "block", "readahead"):
        got, _ = receiver(packed2, 2, mode)
        want, _ = receiver(plain2, 8, mode)
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a == b, (mode, k)
        assert cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 12, mode
        assert cases.count(got) > (8 * 350 + 4 * 200 if mode != "block" else 12 * 280), mode
        if mode == "ticks":
            plain_ticks = got
    # the tick server: this receiver IS served when its slabs are int8 (so the option is live here) ...
    before = engine.tick_server_stats()
    served8, stats8 = receiver(plain2, 8, "ticks", server=True)
    assert stats8["served"] - before["served"] > 100, stats8
    assert len(served8) == len(plain_ticks)
    for k, (a, b) in enumerate(zip(served8, plain_ticks)):
        assert a == b, k
    # ... and not when they are packed: equal packets, no request answered, no server started
    before = engine.tick_server_stats()
    served, stats = receiver(packed2, 2, "ticks", server=True)
    assert len(served) == len(plain_ticks)
    for k, (a, b) in enumerate(zip(served, plain_ticks)):
        assert a == b, k
    assert stats["served"] == before["served"] and stats["starts"] == before["starts"] and not stats["running"]
    # reported, not asserted: the quantisation loss in C/N0, per channel, of the 8-bit, 4-bit and 2-bit streams
    packed4, _, _, _ = cases.write_both(tmp_path, raw, 4, sigma / 2.0)
    raw_path = tmp_path / "iq8.bin"
    raw.tofile(raw_path)
    report = {8: cn0(receiver(raw_path, 8, "ticks")[0]), 4: cn0(receiver(packed4, 4, "ticks")[0]), 2: cn0(plain_ticks)}
    for cid in sorted(report[8]):
        print(f"C/N0 channel {cid}: 8-bit {report[8][cid]:.2f}  4-bit {report[4].get(cid, float('nan')):.2f}  2-bit {report[2].get(cid, float('nan')):.2f} dB-Hz")


# ------------------------------------------------------------------------------------------------ 5. determinism, nothing, long slabs
def test_identical_packed_uploads_leave_identical_rings_and_zero_samples_nothing(engine):
    rng = np.random.default_rng(77)
    cap = 1 << 23                                                       # 4 bits: 8 MiB packed -- `_begin` beyond its staging halves
    p = pk.Packing(4, hostile_table(rng, 4))
    packed = rng.integers(0, 256, pk.packed_bytes(p, cap)).astype(np.uint8)
    engine.iq_alloc(cap, FMT_CI8)
    engine.iq_upload_packed(packed, cap, p, 0)
    first = engine.iq_download(cap, 0)
    assert np.array_equal(first, pk.unpack(packed, p))
    engine.iq_alloc(cap, FMT_CI8)
    engine.iq_upload_packed_begin(packed, cap, p, 0)
    packed_again = packed.copy()
    packed[:] = 0                                                       # (copied before the call returned)
    assert engine.iq_download(cap, 0).tobytes() == first.tobytes()
    engine.iq_upload_packed_queue(packed_again, cap, p, 24)             # the same samples, rotated by 24
    engine.sync()
    assert engine.iq_download(cap, 24).tobytes() == first.tobytes()
    # zero samples: a no-op whatever the pointer
    before = engine.iq_download(4096, 0)
    empty = np.zeros(0, dtype=np.uint8)
    engine.iq_upload_packed(empty, 0, p, 5)
    engine.iq_upload_packed_begin(empty, 0, p, 5)
    engine.iq_upload_packed_queue(empty, 0, p, 5)
    assert engine._lib.sdr_iq_upload_packed(engine._h, C.byref(_lib.IqPacking(4, 0)), None, 0, 0) == 0
    engine.sync()
    assert np.array_equal(engine.iq_download(4096, 0), before)
    # the profiling scopes of the packed route
    engine.prof_enable(True)
    engine.prof_reset()
    engine.iq_upload_packed(packed_again[:4096], 4096, p, 0)
    ms, launches = engine.prof_read("unpack_kernel")
    engine.prof_enable(True, calls_only=True)
    engine.prof_reset()
    engine.iq_upload_packed(packed_again[:4096], 4096, p, 0)
    ms_call, calls = engine.prof_read("call_upload_packed")
    engine.prof_enable(False)
    engine.prof_reset()
    assert launches == 1 and calls == 1 and ms > 0 and ms_call > 0
