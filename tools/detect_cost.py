#!/usr/bin/env python3
"""What the detection statistics of sdr_acq_deep_detect (sydr_amd/csrc/acq_detect.hip) cost on top of the deep search, and
against fetching the map and applying the NumPy statement (docs/notes/detect.md).

    python tools/detect_cost.py [--json out.json] [--prns 32] [--fs 25e6] [--step 50] [--coh 10] [--noncoh 10] [--groups 2]
    python tools/detect_cost.py --tree /path/to/a/checkout/of/the/parent      # sdr_acq_deep alone, as that tree's library runs it

One MI355X, one JSON line.  The README's deep-search row: 32 PRNs at 25 MHz, +-5 kHz by 50 Hz (201 bins), C = 10 x K = 10, two
bit-edge groups, on 100 ms from the device's synthesiser (ci8):
  deep        sdr_acq_deep, no map download: wall clock and the call's in-stream time (scope "call_acq_deep")
  detect_K    sdr_acq_deep_detect with K = 1, 4, 8 peaks (excl_code = rint(fs / 1.023e6) samples, excl_bins = 1): wall clock, the
              call's in-stream time (scope "call_acq_deep_detect"), the in-stream time of "deep_detect_peaks" and
              "deep_detect_noise", and the bytes each of them reads -- (K - 1) and 2 passes over the maps -- as a rate
              against sdr_hbm_copy_rate (which counts bytes read + written: a pure read pass is held against the same figure)
  statement   Engine.acq_deep(want_map=True) -- the download of n_prn * G * bins * N * 8 bytes -- and `deep_detect` in NumPy on
              --statement-prns of the maps, scaled to all of them
A library without sdr_acq_deep_detect (--tree pointing at the parent's checkout, built) gives the deep leg alone: the parent's
time for the same search, same box when both are run from one job.  Warm, medians of --reps calls.  The measuring process
runs under its own `timeout`; nothing is asserted."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

SCOPES = ("deep_detect_peaks", "deep_detect_noise")


def measure(args):
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine

    fs, C, K, G, n_prn = args.fs, args.coh, args.noncoh, args.groups, args.prns
    n = int(round(fs * 1023 / 1.023e6))
    e = Engine(0)
    try:
        e.iq_alloc(C * K * n, FMT_CI8)
        e.code_slots(n_prn)
        for s in range(n_prn):
            e.load_gps_code(s, s + 1)
        rng = np.random.default_rng(20260018)
        sats = [dict(prn=p + 1, doppler=float(rng.integers(-90, 91) * 50.0), code_phase=float(rng.uniform(0, 1023)),
                     phase=float(rng.random()), amp=1.5) for p in range(0, n_prn, 4)]
        e.iq_synth(sats, fs, 20.0, 20260018, 0, C * K * n)
        slots = np.arange(n_prn)
        lib = _lib.load()
        n_bins = int(lib.sdr_pcps_bins(args.range, args.step))
        map_bytes = n_prn * G * n_bins * n * 8
        row = dict(build_id=lib.sdr_build_id().decode(), date=time.strftime("%Y-%m-%d"), n_prn=n_prn, fs=fs, n_code=n,
                   doppler_range=args.range, doppler_step=args.step, n_bins=n_bins, coh=C, noncoh=K, groups=G, reps=args.reps,
                   map_bytes=map_bytes)

        def timed(call, scope, scopes=()):
            call()
            wall, events, parts = [], [], {s: [] for s in scopes}
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            e.prof_enable(True, calls_only=True)
            try:
                for _ in range(args.reps):
                    e.prof_reset()
                    call()
                    events.append(e.prof_read(scope)[0])
            finally:
                e.prof_enable(False)
            if scopes:
                e.prof_enable(True)
                try:
                    for _ in range(args.reps):
                        e.prof_reset()
                        call()
                        for s in scopes:
                            parts[s].append(e.prof_read(s)[0])
                finally:
                    e.prof_enable(False)
            return float(np.median(wall)), float(np.median(events)), {s: float(np.median(v)) for s, v in parts.items()}

        def deep():
            e.acq_deep(slots, 0, fs, 0.0, args.range, args.step, C, K, G, 0.0)
        row["deep_wall_ms"], row["deep_call_ms"], _ = timed(deep, "call_acq_deep")
        if not hasattr(e, "acq_deep_detect"):
            return row
        row["hbm_copy_gbs"] = float(e.hbm_copy_rate())
        excl_code = int(np.rint(fs / 1.023e6))
        for k in (1, 4, 8):
            def detect(k=k):
                e.acq_deep_detect(slots, 0, fs, 0.0, args.range, args.step, C, K, G, 0.0, k, excl_code, 1)
            wall, call, parts = timed(detect, "call_acq_deep_detect", SCOPES)
            reads = dict(deep_detect_peaks=(k - 1) * map_bytes, deep_detect_noise=2 * map_bytes)
            row[f"detect_{k}"] = dict(
                wall_ms=wall, call_ms=call, scopes_ms=parts, over_deep_call=call / row["deep_call_ms"], bytes_read=reads,
                read_gbs={s: (reads[s] / (parts[s] * 1e-3) / 1e9 if parts[s] > 0 and reads[s] else 0.0) for s in SCOPES})
        # the other way to the same figures: the maps through corr_map, the statement in NumPy
        from sydr_amd.dsp.deepsearch import deep_detect
        t0 = time.perf_counter()
        res, cmap = e.acq_deep(slots, 0, fs, 0.0, args.range, args.step, C, K, G, 0.0, want_map=True)
        row["deep_with_map_wall_ms"] = (time.perf_counter() - t0) * 1e3
        m = min(args.statement_prns, n_prn)
        t0 = time.perf_counter()
        want = [deep_detect(cmap[p], 4, excl_code, 1) for p in range(m)]
        row["statement_4_peaks_ms_per_prn"] = (time.perf_counter() - t0) * 1e3 / m
        row["statement_4_peaks_ms_all_prns"] = row["statement_4_peaks_ms_per_prn"] * n_prn
        _, peaks, noise, _ = e.acq_deep_detect(slots[:m], 0, fs, 0.0, args.range, args.step, C, K, G, 0.0, 4, excl_code, 1)
        row["same_peaks_as_statement"] = bool(all(
            [(int(q["group"]), int(q["bin"]), int(q["code"])) for q in peaks[p]] == [(w["group"], w["bin"], w["code"]) for w in want[p][0]]
            and int(noise[p]["n_cells"]) == want[p][1]["n_cells"] for p in range(m)))
        return row
    finally:
        e.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--prns", type=int, default=32)
    ap.add_argument("--fs", type=float, default=25e6)
    ap.add_argument("--range", type=float, default=5000.0)
    ap.add_argument("--step", type=float, default=50.0)
    ap.add_argument("--coh", type=int, default=10)
    ap.add_argument("--noncoh", type=int, default=10)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--statement-prns", dest="statement_prns", type=int, default=2,
                    help="maps the NumPy statement is timed on (its time is scaled to all PRNs)")
    ap.add_argument("--timeout", type=int, default=420, help="time limit of the measuring process in seconds")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose sydr_amd package and library are measured (default: this one)")
    ap.add_argument("--inner", action="store_true", help="measure in this process (what the driver starts under `timeout`)")
    args = ap.parse_args(argv)
    if args.inner:
        sys.path.insert(0, os.path.abspath(args.tree))
        text = json.dumps(measure(args))
        print(text)
        if args.json:
            with open(args.json, "w") as f:
                f.write(text + "\n")
        return 0
    # the driver never opens the GPU itself: a measurement that faults, aborts or runs out of time ends there
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner"]
    for k in ("prns", "fs", "range", "step", "coh", "noncoh", "groups", "reps", "statement_prns", "tree"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    if args.json:
        cmd += ["--json", args.json]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
