#!/usr/bin/env python3
"""What R beams over one push (sdr_ddc_beam_attach) cost against R converters on R engines pushed one after the other, which is
what the same rings cost without the call -- the yardsticks of docs/notes/beams.md.

    python tools/beams_cost.py [--json out.json] [--seconds 1.0] [--timeout 300] [--tree DIR]

One MI355X, one JSON line.  Two legs, one second at 25 MHz each, 33 taps, decimation 2, K = 4, into ci8 rings at 12.5 MHz, pushed
in one call from page-locked memory:
  ci8_K4      4 complex int8 elements, frames of 8 fields (200 MB a second)
  p2_K4       4 complex 2-bit elements, frames of 8 packed fields, two bytes a frame (50 MB a second)
Every leg runs in a process of its own under its own `timeout`, one after the other, and the first that fails ends the run:
nothing more is started on a GPU behind a fault, an abort or a time limit.
Per leg and R in 1, 2, 4, 8, 16, warm, ALTERNATING between the two routes rep by rep, the medians of 15 repetitions of
  (a) fan_*        one converter with R - 1 beams attached, one synchronous push: wall clock around it, the call's in-stream time
                   ("call_ddc_push") and the kernels' ("ddc_kernel" + "ddc_beam_kernel");
  (b) separate_*   R converters with the same weights on R engines, pushed one after the other, each push with its own copy of the
                   same bytes over the link: wall clock around all R, the sum of their calls' and of their kernels' times;
and fan_min / fan_max / separate_min / separate_max of the wall clock, so that "every run of one beats every run of the other"
can be read off.  rings_equal: every beam's ring equals its separate converter's, byte for byte.
With --tree (another checkout with its build: the parent commit's) the R = 1 rows are measured once more in processes that import
that checkout's package -- parent_rows, on the same box.
Exit status: 0 when the rings are equal and, at R = 8, the fan-out's median wall clock is not above the eight pushes'."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPS = 15
FS, TAPS, DECIMATION = 25e6, 33, 2
LEGS = ["ci8_K4", "p2_K4"]
LANES = (0, 2, 4, 6)
BEAMS = (1, 2, 4, 8, 16)


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def events(engines, call, prefixes, calls_only):
    """The in-stream time of the scopes `prefixes`, summed over the engines, of one `call`."""
    for e in engines:
        e.prof_enable(True, calls_only=calls_only)
        e.prof_reset()
    try:
        call()
        return float(sum(e.prof_read(p)[0] for e in engines for p in prefixes))
    finally:
        for e in engines:
            e.prof_enable(False)


def run_leg(name, seconds, only_one):
    """One leg on the GPU -> its rows, one per R (only_one: R = 1 alone, without a beam call -- what a parent build can run)."""
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine
    from sydr_amd.signal import array as ar
    from sydr_amd.signal import downconvert as dc

    rng = np.random.default_rng(20260022)
    engines = [Engine(0) for _ in range(1 if only_one else max(BEAMS))]
    lead = engines[0]
    try:
        n_in = int(FS * seconds) // 128 * 128
        n_out = n_in // DECIMATION
        packed = name == "p2_K4"
        layout = dc.InputLayout(dc.FIELD_PACKED, 2, 8, 0, True) if packed else dc.InputLayout(dc.FIELD_INT8, 0, 8, 0, True)
        block = lead.host_alloc(layout.bytes_for(n_in), layout.dtype)
        block[:] = rng.integers(0, 256, block.size).astype(np.uint8) if packed else rng.integers(-127, 128, block.size).astype(np.int8)
        taps = dc.design_lowpass(TAPS, 0.45 / DECIMATION)
        fcw = dc.frequency_word(1.0e6, FS)
        weights = [(rng.uniform(-1, 1, 4) + 1j * rng.uniform(-1, 1, 4)) / 2.0 for _ in range(max(BEAMS))]
        gain = 8.0 if packed else 0.25
        for e in engines:
            e.iq_alloc(n_out, FMT_CI8)
        rows = []
        for R in ((1,) if only_one else BEAMS):
            used = engines[:R]
            configs = [dc.DownConverterConfig(dc.IN_R8, DECIMATION, taps, fcw, gain, 1, layout, ar.ArrayGeometry(LANES, w)) for w in weights[:R]]
            fan = lead.ddc_create(configs[0])
            for b in range(1, R):
                lead.ddc_beam_attach(fan, used[b], weights[b])
            own = [e.ddc_create(cfg) for e, cfg in zip(used, configs)]

            def push_fan():
                lead.ddc_reset(fan)
                lead.ddc_push(fan, block, 0)

            def push_separate():
                for e, d in zip(used, own):
                    e.ddc_reset(d)
                    e.ddc_push(d, block, 0)
            t = dict(fan_wall=[], separate_wall=[], fan_call=[], separate_call=[], fan_kernel=[], separate_kernel=[])
            for _ in range(3):
                push_fan()
                push_separate()
            for e in used:
                e.sync()
            for _ in range(REPS):
                t["fan_wall"].append(timed(push_fan))
                t["separate_wall"].append(timed(push_separate))
                t["fan_call"].append(events([lead], push_fan, ("call_ddc_push",), True))
                t["separate_call"].append(events(used, push_separate, ("call_ddc_push",), True))
                t["fan_kernel"].append(events([lead], push_fan, ("ddc_kernel", "ddc_beam_kernel"), False))
                t["separate_kernel"].append(events(used, push_separate, ("ddc_kernel",), False))
            push_fan()
            for e in used:
                e.sync()
            fan_rings = [e.iq_download(n_out, 0) for e in used]
            push_separate()
            equal = all(np.array_equal(e.iq_download(n_out, 0), ring) for e, ring in zip(used, fan_rings))
            row = dict(leg=name, beams=R, build_id=_lib.load().sdr_build_id().decode(), n_in=n_in, n_out=n_out, in_bytes=block.nbytes,
                       rings_equal=bool(equal))
            row.update({k + "_ms": float(np.median(v)) for k, v in t.items()})
            row.update(fan_min_ms=min(t["fan_wall"]), fan_max_ms=max(t["fan_wall"]), separate_min_ms=min(t["separate_wall"]),
                       separate_max_ms=max(t["separate_wall"]))
            rows.append(row)
            lead.ddc_destroy(fan)
            for e, d in zip(used, own):
                e.ddc_destroy(d)
        lead.host_free(block)
        return rows
    finally:
        for e in engines:
            e.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of the input")
    ap.add_argument("--timeout", type=int, default=300, help="time limit of a leg's process in seconds")
    ap.add_argument("--tree", default=None, help="another checkout with its build (the parent commit's): the R = 1 rows once more on it")
    ap.add_argument("--package-root", default=None, help="with --leg: import the package from this checkout")
    ap.add_argument("--leg", default=None, help="run this one leg in this process (what the driver starts under `timeout`)")
    ap.add_argument("--only-one", action="store_true", help="with --leg: R = 1 alone, without a beam call")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.package_root) if args.package_root else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if args.leg:
        rows = run_leg(args.leg, args.seconds, args.only_one)
        text = json.dumps(rows)
        print(text)
        if args.json:
            with open(args.json, "w") as f:
                f.write(text + "\n")
        return 0 if all(r["rings_equal"] for r in rows) else 1
    # the driver: it never opens the GPU itself; a leg that faults, aborts or runs out of time ends the run there
    out = dict(seconds=args.seconds, reps=REPS, rows=[], parent_rows=[])
    status = 0
    runs = [(leg, False) for leg in LEGS] + ([(leg, True) for leg in LEGS] if args.tree else [])
    with tempfile.TemporaryDirectory() as tmp:
        for leg, parent in runs:
            path = os.path.join(tmp, leg + ("_parent" if parent else "") + ".json")
            rc = subprocess.call(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", leg,
                                  "--seconds", str(args.seconds), "--json", path] + (["--only-one", "--package-root", args.tree] if parent else []),
                                 stdout=subprocess.DEVNULL)
            if os.path.exists(path):
                with open(path) as f:
                    out["parent_rows" if parent else "rows"] += json.load(f)
                print(f"{leg}{' (parent build)' if parent else ''}: " + json.dumps(json.load(open(path))), file=sys.stderr, flush=True)
            if rc not in (0, 1) or not os.path.exists(path):
                print(f"{leg}: ended with status {rc}; nothing more is started", file=sys.stderr, flush=True)
                out["stopped_at"], status = leg, rc or 1
                break
            status = status or rc
    out["rings_equal"] = bool(status == 0 and len(out["rows"]) == len(LEGS) * len(BEAMS))
    at_8 = [r for r in out["rows"] if r["beams"] == 8]
    out["fan_out_not_slower_at_8"] = bool(len(at_8) == len(LEGS) and all(r["fan_wall_ms"] <= r["separate_wall_ms"] for r in at_8))
    text = json.dumps(out)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
    return status or (0 if out["fan_out_not_slower_at_8"] else 1)


if __name__ == "__main__":
    sys.exit(main())
