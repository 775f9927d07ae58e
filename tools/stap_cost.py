#!/usr/bin/env python3
"""What T taps per element in the array converter (sdr_ddc_create_stap) cost against the spatial array converter
(sdr_ddc_create_array) on the same bytes, and against the link -- the yardsticks of docs/notes/stap.md.

    python tools/stap_cost.py [--json out.json] [--seconds 1.0] [--timeout 300]

One MI355X, one JSON line.  Two legs, one second at 25 MHz each, 33 taps, decimation 2, into a ci8 ring at 12.5 MHz, pushed in
one call from page-locked memory:
  ci8_K4      4 complex int8 elements, frames of 8 fields (200 MB a second)
  p2_K4       4 complex 2-bit elements, frames of 8 packed fields, two bytes a frame (50 MB a second)
Every leg runs in a process of its own under its own `timeout`, one after the other, and the first that fails ends the run:
nothing more is started on a GPU behind a fault, an abort or a time limit.
Per leg, warm, the medians of 25 pushes by wall clock around the synchronous call and of 25 HIP-event brackets (sdr_prof_enable:
"ddc_kernel" and, where it runs, the covariance pass) of
  array_*, array_measured_*    the spatial array converter without and with SDR_DDC_ARRAY_MEASURE, general complex weights -- first,
                               so that every leg has the same process order;
  stapT_*, stapT_measured_*    the space-time converter with T = 1, 3, 5, 7 taps per element, general weights, without and with it
                               (the lag pass of T lags behind the converter's kernel);
and link_copy_ms, the host-link copy of the leg's bytes out of the same page-locked block (one copy command and the wait for
it), reported separately.  stapT_over_array_* = stapT / array and stapT_measured_over_array_* = stapT_measured / array_measured,
by wall clock and by kernel time (converter kernel plus covariance pass); no target is fixed.  one_tap_equals_array: the
space-time converter with T = 1 leaves the ring the array converter leaves, byte for byte (exit status 1 otherwise)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPS = 25
FS, TAPS, DECIMATION = 25e6, 33, 2
LEGS = ["ci8_K4", "p2_K4"]
LANES = (0, 2, 4, 6)
STAP_TAPS = (1, 3, 5, 7)


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
    from sydr_amd.signal import array as ar
    from sydr_amd.signal import downconvert as dc

    rng = np.random.default_rng(20260021)
    e = Engine(0)
    try:
        n_in = int(FS * seconds) // 128 * 128
        n_out = n_in // DECIMATION
        packed = name == "p2_K4"
        layout = dc.InputLayout(dc.FIELD_PACKED, 2, 8, 0, True) if packed else dc.InputLayout(dc.FIELD_INT8, 0, 8, 0, True)
        block = e.host_alloc(layout.bytes_for(n_in), layout.dtype)
        block[:] = rng.integers(0, 256, block.size).astype(np.uint8) if packed else rng.integers(-127, 128, block.size).astype(np.int8)
        taps = dc.design_lowpass(TAPS, 0.45 / DECIMATION)
        fcw = dc.frequency_word(1.0e6, FS)
        w = (rng.uniform(-1, 1, 4) + 1j * rng.uniform(-1, 1, 4)) / 2.0
        gain = 8.0 if packed else 0.25

        def config(array=None):
            return dc.DownConverterConfig(dc.IN_R8, DECIMATION, taps, fcw, gain, 1, layout, array)
        row = dict(leg=name, build_id=_lib.load().sdr_build_id().decode(), n_in=n_in, n_out=n_out, elements=4, taps=TAPS, decimation=DECIMATION,
                   in_bytes=block.nbytes, out_bytes=2 * n_out)
        as_i16 = block.view(np.uint8).view(np.int16)
        e.iq_alloc(as_i16.size // 2, FMT_CI16)

        def link():
            e.iq_upload_queue(as_i16, 0)
            e.sync()
        for _ in range(3):
            link()
        row["link_copy_ms"] = median_ms(link)
        e.iq_alloc(n_out, FMT_CI8)
        from sydr_amd.signal import stap
        rings = {}
        made = [("array_", config(ar.ArrayGeometry(LANES, w)), None), ("array_measured_", config(ar.ArrayGeometry(LANES, w, measure=True)), "ddc_array_cov_kernel")]
        for T in STAP_TAPS:
            wt = np.zeros((T, 4), dtype=np.complex128)
            wt[0] = w
            if T > 1:
                wt[1:] = (rng.uniform(-1, 1, (T - 1, 4)) + 1j * rng.uniform(-1, 1, (T - 1, 4))) / (2.0 * T)
            made.append((f"stap{T}_", config(stap.SpaceTimeGeometry(LANES, T, wt)), None))
            made.append((f"stap{T}_measured_", config(stap.SpaceTimeGeometry(LANES, T, wt, measure=True)), "ddc_stap_cov_kernel"))
        for prefix, cfg, cov_scope in made:
            ddc = e.ddc_create(cfg)

            def push():
                e.ddc_reset(ddc)
                e.ddc_push(ddc, block, 0)
            for _ in range(3):
                push()
            row.update({prefix + "wall_ms": median_ms(push), prefix + "kernel_ms": event_ms(e, push, "ddc_kernel", False)})
            row[prefix + "covariance_ms"] = event_ms(e, push, cov_scope, False) if cov_scope else 0.0
            rings[prefix] = e.iq_download(n_out, 0)
            e.ddc_destroy(ddc)
        row["one_tap_equals_array"] = bool(np.array_equal(rings["stap1_"], rings["array_"]))
        for T in STAP_TAPS:
            for kind, base in (("", "array_"), ("measured_", "array_measured_")):
                mine = f"stap{T}_{kind}"
                row[f"{mine}over_array_wall"] = row[mine + "wall_ms"] / row[base + "wall_ms"]
                row[f"{mine}over_array_kernels"] = (row[mine + "kernel_ms"] + row[mine + "covariance_ms"]) / (row[base + "kernel_ms"] + row[base + "covariance_ms"])
        e.host_free(block)
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
        return 0 if row["one_tap_equals_array"] else 1
    # the driver: it never opens the GPU itself; a leg that faults, aborts or runs out of time ends the run there
    out = dict(seconds=args.seconds, reps=REPS, rows=[])
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for leg in LEGS:
            path = os.path.join(tmp, leg + ".json")
            rc = subprocess.call(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
                                  "--seconds", str(args.seconds), "--json", path], stdout=subprocess.DEVNULL)
            if os.path.exists(path):
                with open(path) as f:
                    out["rows"].append(json.load(f))
                print(f"{leg}: " + json.dumps(out["rows"][-1]), file=sys.stderr, flush=True)
            if rc not in (0, 1) or not os.path.exists(path):
                print(f"{leg}: ended with status {rc}; nothing more is started", file=sys.stderr, flush=True)
                out["stopped_at"], status = leg, rc or 1
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
