#!/usr/bin/env python3
"""What the deep search (sdr_acq_deep, sydr_amd/csrc/acq_deep.hip + pcps.hip run_deep) costs against the search it replaces
(docs/notes/deep_acq.md).

    python tools/deep_acq_cost.py [--json out.json] [--prns 32] [--fs 25e6] [--step 50] [--coh 10] [--noncoh 10] [--timeout 420]
    python tools/deep_acq_cost.py --tree /path/to/a/checkout/of/the/parent      # sdr_pcps alone, as that tree's library runs it

One MI355X, one JSON line.  32 PRNs at 25 MHz, +-5 kHz by 50 Hz (201 bins), C = 10 coherent periods x K = 10 blocks on 100 ms
from the device's synthesiser (ci8):
  deep      sdr_acq_deep, G = 1, no compensation, no map download: wall clock around the synchronous call, the call's in-stream
            time (HIP events, scope "call_acq_deep") and the in-stream time of every "deep_*" scope
  pcps      sdr_pcps(coh = 10, noncoh = 10) with the map wanted (the only way the library runs that search: ROUTE_MAP): the
            call's in-stream time (scope "call_pcps": the kernels, not the 1.3 GB download of the map) and the wall clock
A library without sdr_acq_deep (--tree pointing at the parent's checkout, built) gives the pcps leg alone: the parent's time
for that call, same box when both are run from one job.  Warm, medians of --reps calls.  The measuring process runs under its
own `timeout`; nothing is asserted about the ratio -- by transform count the deep route makes C times fewer inverse
transforms, what that buys is what this prints."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

SCOPES = ("deep_fold", "deep_fwd_fft", "deep_inv_fft", "deep_shift_acc", "deep_peak")


def measure(args):
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine

    fs, C, K, n_prn = args.fs, args.coh, args.noncoh, args.prns
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
        row = dict(build_id=_lib.load().sdr_build_id().decode(), n_prn=n_prn, fs=fs, n_code=n, doppler_range=args.range,
                   doppler_step=args.step, n_bins=int(_lib.load().sdr_pcps_bins(args.range, args.step)), coh=C, noncoh=K, reps=args.reps)

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

        if hasattr(e, "acq_deep"):
            peaks = {}

            def deep():
                peaks["deep"] = e.acq_deep(slots, 0, fs, 0.0, args.range, args.step, C, K, 1, 0.0)[0]
            row["deep_wall_ms"], row["deep_call_ms"], row["deep_scopes_ms"] = timed(deep, "call_acq_deep", SCOPES)

        def pcps():
            peaks_pcps[:] = e.pcps(slots, 0, fs, 0.0, args.range, args.step, C, K, want_map=True)[:2]
        peaks_pcps = [None, None]
        row["pcps_wall_ms"], row["pcps_call_ms"], _ = timed(pcps, "call_pcps")
        if "deep_call_ms" in row:
            row["pcps_over_deep_call"] = row["pcps_call_ms"] / row["deep_call_ms"]
            present = [s["prn"] - 1 for s in sats]
            row["same_peaks_on_present_prns"] = bool(
                np.array_equal(peaks["deep"]["peak_bin"][present], peaks_pcps[0][present]) and
                np.array_equal(peaks["deep"]["peak_code"][present], peaks_pcps[1][present]))
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
    ap.add_argument("--reps", type=int, default=5)
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
    for k in ("prns", "fs", "range", "step", "coh", "noncoh", "reps", "tree"):
        cmd += ["--" + k, str(getattr(args, k))]
    if args.json:
        cmd += ["--json", args.json]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
