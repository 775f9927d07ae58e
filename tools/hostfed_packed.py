#!/usr/bin/env python3
"""A recording fed from the host packed at 4, 2 and 1 bit against its int8 image: bench.py's `host_fed` leg, step for step
(60 s, 32 channels, 25 MHz, 1 s chunks, one plan made inside the timed region, minimum of three passes), on ONE few-level
stream, in ONE process, the legs alternated.

  leg a      the stream's int8 image through sdr_iq_upload_queue (the yardstick);
  legs b4/b2/b1   the same samples packed through sdr_iq_upload_packed_queue;
each from page-locked memory (the whole stream) and from a pageable np.memmap (its first --pageable-seconds).  The stream is
the device-born one of bench.py reduced to its signs (+-1): the one set of samples every width's default table holds.
Every leg's outputs must equal, byte for byte, the one-launch pass over the resident stream, or the tool exits non-zero.
Reported per leg: x real time, link GB/s in the bytes that crossed, the spread of its passes; beside them the resident rate
(one plan re-run on the resident ring), the unpack kernel alone on a 1 s chunk against sdr_hbm_copy_rate and against the
chunk's link transfer, and -- with --per-tick -- the per-millisecond Python loop with a packed slab and with an int8 slab.
One JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from sydr_amd.engine import FMT_CI8, Engine  # noqa: E402
from sydr_amd.signal import packing as pk  # noqa: E402

FS, N_CH, SPACING = bench.FS, bench.N_CH, bench.SPACING
WIDTHS = (4, 2, 1)


def pack_signs(negative, bits):
    """+-1 samples (negative: bool per component) packed with the default table of `bits`, least significant field first --
    np.packbits on the codes' bits (1 bit: code 1 = -1; 2 bits: +1 = 00, -1 = 10; 4 bits: +1 = 0001, -1 = 1111): what
    packing.pack gives (checked by the caller on a slice), at memory speed."""
    if bits == 1:
        return np.packbits(negative, bitorder="little")
    planes = np.empty((negative.size, bits), dtype=np.uint8)
    if bits == 2:
        planes[:, 0], planes[:, 1] = 0, negative
    else:
        planes[:, 0] = 1
        planes[:, 1:] = negative[:, None]
    return np.packbits(planes.reshape(-1), bitorder="little")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--pageable-seconds", type=float, default=12.0)
    ap.add_argument("--chunk-seconds", type=float, default=1.0)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--per-tick", action="store_true", help="also the per-millisecond Python loop, packed and int8 slabs")
    args = ap.parse_args(argv)

    eng = Engine(0)
    try:
        eng.set_option("bind_thread_to_device", 1)
    except Exception:
        pass
    chunk = int(args.chunk_seconds * FS) // 8 * 8
    total = int(args.seconds * FS) // chunk * chunk
    n_chunks = total // chunk
    sats = bench.satellites(N_CH)
    eng.iq_alloc(total, FMT_CI8)
    eng.code_slots(N_CH)
    for c, s in enumerate(sats):
        eng.load_gps_code(c, s["prn"])
    eng.iq_synth(sats, FS, 12.0, 20260003, 0, total)
    items, n_epochs = bench.truth_items(sats, FS, total)
    batch = eng.stream_create()

    # the recording: signs of the device-born stream, as int8 and packed at every width, in page-locked memory
    packings = {b: pk.Packing(b) for b in WIDTHS}
    host = {8: eng.host_alloc(2 * total, np.int8)}
    for b in WIDTHS:
        host[b] = eng.host_alloc(pk.packed_bytes(packings[b], total), np.uint8)
    t_prep = time.perf_counter()
    for k in range(n_chunks):
        a = k * chunk
        negative = eng.iq_download(chunk, a) < 0
        host[8][2 * a:2 * (a + chunk)] = np.where(negative, np.int8(-1), np.int8(1))
        for b in WIDTHS:
            per = pk.packed_bytes(packings[b], chunk)
            host[b][k * per:(k + 1) * per] = pack_signs(negative, b)
    for b in WIDTHS:       # (the fast packer against the format module, on the stream's first samples)
        head = 1 << 16
        if not np.array_equal(pk.unpack(host[b][:pk.packed_bytes(packings[b], head)], packings[b]), host[8][:2 * head]):
            raise SystemExit(f"{b}-bit image of the stream is not its int8 image")
    t_prep = time.perf_counter() - t_prep

    # the resident stream: the ceiling, and the outputs every leg has to reproduce
    for k in range(n_chunks):
        eng.iq_upload(host[8][2 * k * chunk:2 * (k + 1) * chunk], k * chunk)
    plan = eng.epl_plan(items, SPACING, FS)
    plan.run()
    want = plan.fetch().copy()
    resident = []
    for _ in range(args.passes):
        eng.sync()
        t0 = time.perf_counter()
        plan.run()
        eng.stream_sync(0)
        resident.append(time.perf_counter() - t0)
    plan.close()

    ends = (items["start_sample"] + items["n_samples"])[:n_epochs * N_CH].reshape(n_epochs, N_CH).max(axis=1)
    upto = np.searchsorted(ends, [(k + 1) * chunk for k in range(n_chunks)], side="right") * N_CH

    def one_pass(source, bits, chunks, zero_first):
        if zero_first:
            eng.iq_alloc(total, FMT_CI8)                   # a ring of zeros: what is correlated came over the link
        eng.sync()
        per = 2 * chunk if bits == 8 else pk.packed_bytes(packings[bits], chunk)
        t0 = time.perf_counter()
        plan = eng.epl_plan(items, SPACING, FS)
        done = 0
        for k in range(chunks):
            if bits == 8:
                eng.iq_upload_queue(source[k * per:(k + 1) * per], k * chunk)
            else:
                eng.iq_upload_packed_queue(source[k * per:(k + 1) * per], chunk, packings[bits], k * chunk)
            if upto[k] > done:
                plan.run(done, int(upto[k]) - done, stream=batch)
                done = int(upto[k])
        eng.stream_sync(batch)
        eng.sync()
        return plan, done, time.perf_counter() - t0

    def run_legs(sources, chunks, label):
        out = {}
        for bits in (8,) + WIDTHS:                          # first pass of each: into a ring of zeros, outputs compared
            plan, done, dt = one_pass(sources[bits], bits, chunks, True)
            same = plan.fetch()[:done].tobytes() == np.ascontiguousarray(want[:done]).tobytes()
            plan.close()
            if not same or (chunks == n_chunks and done != n_epochs * N_CH):
                raise SystemExit(f"{label} leg at {bits} bits differs from the one-launch pass over the resident stream")
            out[bits] = dict(first_pass_ms=dt * 1e3, passes_ms=[], bitwise_identical_to_one_launch=True)
        for _ in range(args.passes):                        # the legs alternated
            for bits in (8,) + WIDTHS:
                plan, done, dt = one_pass(sources[bits], bits, chunks, False)
                plan.close()
                out[bits]["passes_ms"].append(dt * 1e3)
        seconds = chunks * chunk / FS
        for bits, leg in out.items():
            dt = min(leg["passes_ms"]) * 1e-3
            crossed = chunks * (2 * chunk if bits == 8 else pk.packed_bytes(packings[bits], chunk))
            leg.update(x_realtime=seconds / dt, link_GBps=crossed / dt / 1e9, ms_per_pass=dt * 1e3,
                       spread_ms=max(leg["passes_ms"]) - min(leg["passes_ms"]), stream_seconds=seconds, memory=label)
        return {("a_int8" if bits == 8 else f"b{bits}"): leg for bits, leg in out.items()}

    result = {"config": dict(stream_seconds=total / FS, channels=N_CH, fs_hz=FS, chunk_s=chunk / FS, passes=args.passes,
                             stream="signs (+-1) of bench.py's device-born stream", build_id=eng._lib.sdr_build_id().decode(),
                             host_preparation_s=t_prep),
              "resident": dict(x_realtime=total / FS / min(resident), passes_ms=[t * 1e3 for t in resident])}
    result["page_locked"] = run_legs(host, n_chunks, "page-locked (sdr_host_alloc)")
    page_chunks = min(n_chunks, int(args.pageable_seconds * FS) // chunk)
    if page_chunks >= 2:
        with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
            maps = {}
            for bits in (8,) + WIDTHS:
                per = 2 * chunk if bits == 8 else pk.packed_bytes(packings[bits], chunk)
                path = os.path.join(tmp, f"recording.{bits}")
                host[bits][:page_chunks * per].tofile(path)
                maps[bits] = np.asarray(np.memmap(path, dtype=host[bits].dtype, mode="r"))
            result["pageable"] = run_legs(maps, page_chunks, "np.memmap of a file (pageable)")
            del maps
    # the one condition: no packed leg slower than leg (a) of the same run by more than the spread of leg (a)'s passes
    verdict = {}
    for memory in ("page_locked", "pageable"):
        legs = result.get(memory)
        if legs:
            a = legs["a_int8"]
            verdict[memory] = {name: bool(leg["ms_per_pass"] <= a["ms_per_pass"] + a["spread_ms"]) for name, leg in legs.items() if name != "a_int8"}
    result["no_packed_leg_slower_than_int8"] = verdict

    # the unpack kernel alone on a 1 s chunk that is already in HBM (the staging buffer), and the chunk's link transfer
    eng.iq_alloc(total, FMT_CI8)
    result["hbm_copy_GBps"] = eng.hbm_copy_rate(1 << 30, 10)
    kernel = {}
    for bits in WIDTHS:
        per = pk.packed_bytes(packings[bits], chunk)
        eng.iq_upload_packed_queue(host[bits][:per], chunk, packings[bits], 0)       # warm: staging buffer, code object
        eng.sync()
        eng.prof_enable(True)
        eng.prof_reset()
        for _ in range(5):
            eng.iq_upload_packed_queue(host[bits][:per], chunk, packings[bits], 0)
        k_ms, n = eng.prof_read("unpack_kernel")
        eng.prof_enable(True, calls_only=True)
        eng.prof_reset()
        for _ in range(5):
            eng.iq_upload_packed_queue(host[bits][:per], chunk, packings[bits], 0)
        c_ms, n_c = eng.prof_read("call_upload_packed")
        eng.prof_enable(False)
        eng.prof_reset()
        k_ms, c_ms = k_ms / n, c_ms / n_c
        kernel[f"{bits}bit"] = dict(kernel_ms=k_ms, GBps_read_plus_written=(per + 2 * chunk) / (k_ms * 1e-3) / 1e9,
                                    copy_plus_kernel_ms=c_ms, link_transfer_ms=c_ms - k_ms, transfer_over_kernel=(c_ms - k_ms) / k_ms)
    result["unpack_kernel_1s_chunk"] = kernel
    for block in host.values():
        eng.host_free(block)
    if args.per_tick:
        import per_tick_rate
        keys = ("ms_per_tick", "x_realtime", "ms_per_tick_all_packets_read", "ticks_all_tracking", "channels_tracking_at_end")
        pick = lambda r: {k: r[k] for k in keys}
        result["per_tick"] = {"int8_slab_of_2bit_levels": pick(per_tick_rate.measure(600, N_CH, engine=eng, few_bits=2)),
                              "packed_2bit_slab": pick(per_tick_rate.measure(600, N_CH, engine=eng, few_bits=2, packed=True))}
    eng.close()
    print(json.dumps(result))
    ok = all(all(v.values()) for v in verdict.values())
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
