#!/usr/bin/env python3
"""What the device's rational resampler (sdr_ddc_create_rational, sydr_amd/csrc/resample.hip) costs against the yardsticks of
docs/notes/resample.md.

    python tools/resample_cost.py [--json out.json] [--seconds 1.0] [--timeout 420]

One MI355X, one JSON line.  Four legs, one second of input each, pushed in one call from page-locked memory:
  ci8_16368k_to_12M     ci8 at 16.368 MHz, L / M = 250 / 341, the default prototype (5457 taps, 22 per phase) -> ci8 at 12 MHz
  ci8_16368k_to_24M     ci8 at 16.368 MHz, 500 / 341 (8001 taps, 17 per phase) -> ci8 at 24 MHz
  r8_38192k_IF_2_3      real int8 at 38.192 MHz, IF 9.548 MHz (fs / 4), 2 / 3 (49 taps, 25 per phase) -> ci8 at 25.461 MHz
  ci16_5456k_to_10M     ci16 at 5.456 MHz, 625 / 341 (10001 taps, 17 per phase) -> ci16 at 10 MHz
Every leg runs in a process of its own under its own `timeout`, one after the other, and the first that fails ends the run (the
equivalent of chaining them with &&): nothing more is started on a GPU behind a fault, an abort or a time limit.
Per leg, warm: the medians of 25 pushes by wall clock around the synchronous call and of 25 HIP-event brackets
(sdr_prof_enable: the whole call's scope "call_ddc_push" -- copy command and kernels --, then "resample_kernel" and
"ddc_history_kernel"), and beside them
  parent_route_ms    (i) the only route without the resampler: the NumPy statement (sydr_amd/signal/downconvert.py) on the host
                     plus Engine.iq_upload of its output, wall clock, once, same box, same run;
  ddc_kernel_ms      (ii) the integer converter's ddc_kernel on the same input with ceil(T / L) taps and D = max(1, round(M / L)):
                     the same number of products per output by scalar tap loads, HIP events, median of 25 -- and, the two making
                     different numbers of outputs, kernel_per_output_over_ddc = the ratio of the kernels' times per output;
  link_copy_ms       (iii) the host-link copy of the same input bytes out of the same page-locked block (one copy command and the
                     wait for it), wall clock, median of 25, same run.
The one condition (exit status 1 when it fails): no leg's push is slower than (i).  The ratios to (ii) and (iii) are reported."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPS = 25
#        name                  input   fs_in      shift     L    M    ring is ci16  gain
LEGS = [("ci8_16368k_to_12M", "ci8", 16.368e6, 0.0, 250, 341, False, 1.0),
        ("ci8_16368k_to_24M", "ci8", 16.368e6, 0.0, 500, 341, False, 1.0),
        ("r8_38192k_IF_2_3", "r8", 38.192e6, 9.548e6, 2, 3, False, 2.0),
        ("ci16_5456k_to_10M", "ci16", 5.456e6, 0.0, 625, 341, True, 1.0)]


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

    _, kind, fs_in, shift, L, M, wide, gain = next(leg for leg in LEGS if leg[0] == name)
    in_fmt = dict(ci8=dc.IN_CI8, r8=dc.IN_R8, ci16=dc.IN_CI16)[kind]
    ring_fmt = FMT_CI16 if wide else FMT_CI8
    rng = np.random.default_rng(20260019)
    e = Engine(0)
    try:
        n_in = int(fs_in * seconds) // (64 * M) * (64 * M)               # (whole periods, both rings whole granules)
        n_out = n_in * L // M
        per = 2 if dc.input_is_complex(in_fmt) else 1
        dtype = dc.input_dtype(in_fmt)
        amp = 100 if dtype == np.int8 else 2500
        block = e.host_alloc(per * n_in, dtype)
        block[:] = rng.integers(-amp, amp + 1, per * n_in).astype(dtype)
        in_bytes, out_bytes = block.nbytes, n_out * (4 if wide else 2)
        taps = dc.design_resampler(L, M)
        cfg = dc.DownConverterConfig(in_fmt, M, taps, dc.frequency_word(shift, fs_in), gain, L)
        row = dict(leg=name, build_id=_lib.load().sdr_build_id().decode(), n_in=n_in, n_out=n_out, interpolation=L, decimation=M,
                   taps=int(taps.size), taps_per_phase=cfg.phase_taps, in_bytes=in_bytes, out_bytes=out_bytes)
        # (iii) the link: the same bytes by one copy command into a ring that takes them as they are (ci16: no sign flip behind it)
        e.iq_alloc(-(-in_bytes // 4), FMT_CI16)
        as_i16 = block.view(np.int8).view(np.int16) if in_bytes % 4 == 0 else None

        def link():
            e.iq_upload_queue(as_i16, 0)
            e.sync()
        if as_i16 is not None:
            for _ in range(3):
                link()
            row["link_copy_ms"] = median_ms(link)
        # (ii) the integer converter on the same input: as many products per output, the taps by scalar loads
        D2, T2 = max(1, round(M / L)), cfg.phase_taps
        cfg2 = dc.DownConverterConfig(in_fmt, D2, dc.design_lowpass(T2, 0.45 / D2) if T2 > 1 else np.ones(1), cfg.fcw, gain)
        n_out2 = dc.out_count(0, n_in, D2)
        e.iq_alloc(n_out2, ring_fmt)
        ddc2 = e.ddc_create(cfg2)

        def push2():
            e.ddc_reset(ddc2)
            e.ddc_push(ddc2, block, 0)
        for _ in range(3):
            push2()
        row.update(ddc_taps=T2, ddc_decimation=D2, ddc_n_out=n_out2, ddc_wall_ms=median_ms(push2), ddc_kernel_ms=event_ms(e, push2, "ddc_kernel", False))
        e.ddc_destroy(ddc2)
        # the resampler
        e.iq_alloc(n_out, ring_fmt)
        ddc = e.ddc_create(cfg)

        def push():
            e.ddc_reset(ddc)
            e.ddc_push(ddc, block, 0)
        for _ in range(3):
            push()
        row.update(wall_ms=median_ms(push), call_ms=event_ms(e, push, "call_ddc_push", True),
                   kernel_ms=event_ms(e, push, "resample_kernel", False), history_kernel_ms=event_ms(e, push, "ddc_history_kernel", False))
        got = e.iq_download(n_out, 0)
        e.ddc_destroy(ddc)
        print(f"{name}: device done, the statement on the host ...", file=sys.stderr, flush=True)
        # (i) the only route without the resampler, once: the statement on the host, then an ordinary upload of its output
        t0 = time.perf_counter()
        want = dc.statement(cfg, [block], ring_fmt)
        e.iq_upload(want, 0)
        row["parent_route_ms"] = (time.perf_counter() - t0) * 1e3
        row["equal_to_statement"] = bool(np.array_equal(got, want))
        row["speedup_over_parent_route"] = row["parent_route_ms"] / row["wall_ms"]
        row["not_slower_than_parent_route"] = bool(row["wall_ms"] <= row["parent_route_ms"])
        row["kernel_over_ddc_kernel"] = row["kernel_ms"] / row["ddc_kernel_ms"]
        row["kernel_per_output_over_ddc"] = (row["kernel_ms"] / n_out) / (row["ddc_kernel_ms"] / n_out2)
        if "link_copy_ms" in row:
            row["kernel_over_link_copy"] = row["kernel_ms"] / row["link_copy_ms"]
        e.host_free(block)
        return row
    finally:
        e.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of the input")
    ap.add_argument("--timeout", type=int, default=420, help="time limit of a leg's process in seconds")
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
        return 0 if row["not_slower_than_parent_route"] else 1
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
    out["conditions_hold"] = bool(status == 0 and len(out["rows"]) == len(LEGS))
    text = json.dumps(out)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
