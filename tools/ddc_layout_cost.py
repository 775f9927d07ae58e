#!/usr/bin/env python3
"""What an input layout (sdr_ddc_create_layout: packed and float32 recordings decoded where the converter's kernels load them)
costs against widening the same samples on the host, and against the link -- the yardsticks of docs/notes/downconvert.md.

    python tools/ddc_layout_cost.py [--json out.json] [--seconds 1.0] [--timeout 300]

One MI355X, one JSON line.  Three legs, one second of input each, pushed in one call from page-locked memory:
  p2r_16368k_to_12M     2-bit real at 16.368 MHz, IF 4.092 MHz (fs / 4), L / M = 250 / 341, the default prototype -> ci8 at 12 MHz
  p2c_25MHz_T33_D2      2-bit complex at 25 MHz, 33 taps, decimation 2 -> ci8 at 12.5 MHz
  f32c_25MHz_mix_only   float32 complex at 25 MHz, one tap, decimation 1 (mixing only), gain 1 -> ci16 at 25 MHz
Every leg runs in a process of its own under its own `timeout`, one after the other, and the first that fails ends the run:
nothing more is started on a GPU behind a fault, an abort or a time limit.
Per leg, warm: the medians of 25 pushes by wall clock around the synchronous call and of 25 HIP-event brackets
(sdr_prof_enable: the whole call's scope "call_ddc_push" -- copy command and kernels --, then the kernel's scope "ddc_kernel" or
"resample_kernel" and "ddc_history_kernel"), and beside them, in the same run,
  (a) widened_*     the same samples widened on the host (`packing.unpack`; `astype(int16)` for the float leg -- the samples are
                    integers) into page-locked memory, widen_host_ms once by wall clock, and pushed through the old-format
                    converter: wall, call and kernel medians as above; equal_to_widened = the two rings are equal byte for byte;
  (b) link_copy_ms  the host-link copy of the leg's own input bytes out of the same page-locked block (one copy command and the
                    wait for it), wall clock, median of 25; widened_link_copy_ms the same for (a)'s bytes.
The expectation is reported, not made a condition (exit status 1 only when a ring differs): push_not_slower_than_widened_push
= the layout's push is no slower than (a)'s push alone, four to eight times fewer bytes crossing the link."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPS = 25
#        name                    fs_in      shift      L    M    taps  ring is ci16
LEGS = [("p2r_16368k_to_12M", 16.368e6, 4.092e6, 250, 341, None, False),
        ("p2c_25MHz_T33_D2", 25e6, 0.0, 1, 2, 33, False),
        ("f32c_25MHz_mix_only", 25e6, 1.0e6, 1, 1, 1, True)]


def median_ms(call, reps=REPS):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def event_ms(engine, call, prefix, calls_only, reps=REPS):
    engine.prof_enable(True, calls_only=calls_only)
    t = []
    try:
        for _ in range(reps):
            engine.prof_reset()
            call()
            t.append(engine.prof_read(prefix)[0])
    finally:
        engine.prof_enable(False)
    return float(np.median(t))


def run_leg(name, seconds):
    """One leg on the GPU -> its row."""
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI16, FMT_CI8, Engine
    from sydr_amd.signal import downconvert as dc
    from sydr_amd.signal import packing as pk

    _, fs_in, shift, L, M, T, wide = next(leg for leg in LEGS if leg[0] == name)
    ring_fmt = FMT_CI16 if wide else FMT_CI8
    kernel = "resample_kernel" if L != 1 else "ddc_kernel"
    rng = np.random.default_rng(20260020)
    e = Engine(0)
    try:
        n_in = int(fs_in * seconds) // (64 * M) * (64 * M)                 # (whole periods, whole bytes, both rings whole granules)
        n_out = n_in * L // M
        taps = dc.design_resampler(L, M) if L != 1 else dc.design_lowpass(T, 0.45 / M)
        fcw = dc.frequency_word(shift, fs_in)
        if name.startswith("f32"):
            layout, old_fmt = dc.InputLayout(dc.FIELD_FLOAT32, complex=True), dc.IN_CI16
            block = e.host_alloc(2 * n_in, np.float32)
            block[:] = rng.integers(-2500, 2501, 2 * n_in).astype(np.float32)

            def widen(dst):
                dst[:] = block.astype(np.int16)
        else:
            cplx = name.startswith("p2c")
            layout, old_fmt = dc.InputLayout(dc.FIELD_PACKED, 2, complex=cplx), dc.IN_CI8 if cplx else dc.IN_R8
            block = e.host_alloc(layout.bytes_for(n_in), np.uint8)
            block[:] = rng.integers(0, 256, block.size).astype(np.uint8)
            packing = pk.Packing(2)

            def widen(dst):
                dst[:] = pk.unpack(block, packing)
        per = 2 if layout.complex else 1
        wide_block = e.host_alloc(per * n_in, dc.input_dtype(old_fmt))
        t0 = time.perf_counter()
        widen(wide_block)
        widen_ms = (time.perf_counter() - t0) * 1e3
        cfg = dc.DownConverterConfig(old_fmt, M, taps, fcw, 1.0, L, layout)
        old_cfg = dc.DownConverterConfig(old_fmt, M, taps, fcw, 1.0, L)
        row = dict(leg=name, build_id=_lib.load().sdr_build_id().decode(), n_in=n_in, n_out=n_out, interpolation=L, decimation=M,
                   taps=int(taps.size), in_bytes=block.nbytes, widened_bytes=wide_block.nbytes, out_bytes=n_out * (4 if wide else 2),
                   widen_host_ms=widen_ms)

        # (b) the link: the bytes by one copy command into a ring that takes them as they are (ci16: no sign flip behind it)
        def link_of(data):
            as_i16 = data.view(np.uint8).view(np.int16)
            e.iq_alloc(as_i16.size // 2, FMT_CI16)

            def link():
                e.iq_upload_queue(as_i16, 0)
                e.sync()
            for _ in range(3):
                link()
            return median_ms(link)
        row["link_copy_ms"], row["widened_link_copy_ms"] = link_of(block), link_of(wide_block)
        e.iq_alloc(n_out, ring_fmt)
        rings = []
        for prefix, c, data in (("", cfg, block), ("widened_", old_cfg, wide_block)):
            ddc = e.ddc_create(c)

            def push():
                e.ddc_reset(ddc)
                e.ddc_push(ddc, data, 0)
            for _ in range(3):
                push()
            row.update({prefix + "wall_ms": median_ms(push), prefix + "call_ms": event_ms(e, push, "call_ddc_push", True),
                        prefix + "kernel_ms": event_ms(e, push, kernel, False),
                        prefix + "history_kernel_ms": event_ms(e, push, "ddc_history_kernel", False)})
            rings.append(e.iq_download(n_out, 0))
            e.ddc_destroy(ddc)
        row["equal_to_widened"] = bool(np.array_equal(rings[0], rings[1]))
        row["push_over_widened_push"] = row["wall_ms"] / row["widened_wall_ms"]
        row["push_not_slower_than_widened_push"] = bool(row["wall_ms"] <= row["widened_wall_ms"])
        row["kernel_over_widened_kernel"] = row["kernel_ms"] / row["widened_kernel_ms"]
        row["kernel_over_link_copy"] = row["kernel_ms"] / row["link_copy_ms"]
        e.host_free(block)
        e.host_free(wide_block)
        return row
    finally:
        e.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of the input")
    ap.add_argument("--timeout", type=int, default=300, help="time limit of a leg's process in seconds")
    ap.add_argument("--leg", default=None, help="run this one leg in this process (what the driver starts under `timeout`)")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if args.leg:
        row = run_leg(args.leg, args.seconds)
        text = json.dumps(row)
        print(text)
        if args.json:
            with open(args.json, "w") as f:
                f.write(text + "\n")
        return 0 if row["equal_to_widened"] else 1
    # the driver: it never opens the GPU itself; a leg that faults, aborts or runs out of time ends the run there
    out = dict(seconds=args.seconds, reps=REPS, rows=[])
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for leg in LEGS:
            path = os.path.join(tmp, leg[0] + ".json")
            rc = subprocess.call(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg[0],
                                  "--seconds", str(args.seconds), "--json", path], stdout=subprocess.DEVNULL)
            if os.path.exists(path):
                with open(path) as f:
                    out["rows"].append(json.load(f))
                print(f"{leg[0]}: " + json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
            if rc not in (0, 1) or not os.path.exists(path):
                print(f"{leg[0]}: ended with status {rc}; nothing more is started", file=sys.stderr, flush=True)
                out["stopped_at"], status = leg[0], rc or 1
                break
            status = status or rc
    out["rings_equal"] = bool(status == 0 and len(out["rows"]) == len(LEGS))
    text = json.dumps(out)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
