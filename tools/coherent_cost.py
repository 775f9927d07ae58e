#!/usr/bin/env python3
"""What sdr_pcps_coherent costs, beside the search it supersedes and the only other route to its numbers
(docs/notes/coherent_search.md):

    python tools/coherent_cost.py [--slots 32] [--reps 5] [--small-only] [--json out]

One MI355X, one JSON line.  A ci8 ring from the device's synthesiser, `slots` seeded 1023-chip codes at 1.023 Mcps under NH20,
M = 20 periods, 9 coarse bins at 250 Hz, K = 11 fine frequencies at 25 Hz, results only -- at 4 MHz (N = 4000) and at 25 MHz
(N = 25 000); the cost does not depend on what the search finds.
  (a) coherent    Engine.pcps_coherent: "coherent_fwd_fft", "coherent_inv_fft", "coherent_combine", "coherent_peak",
                  "coherent_pick" and "call_pcps_coherent" in stream time, the host clock around the synchronous call
                  (medians of --reps warm calls)
  (b) padded      Engine.pcps_signal(pad=1, noncoh=20) on the same window and bins: "call_pcps_signal" and the host clock
  (c) statement   iq_download of the window plus dsp.signalsearch.pcps_coherent_statement for ONE slot: host clock
Nothing is asserted about any ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CODE_HZ, CHIPS, M = 1.023e6, 1023, 20
RANGE, STEP, SPAN, FINE = 1000.0, 250.0, 125.0, 25.0
SCOPES = ("coherent_fwd_fft", "coherent_inv_fft", "coherent_combine", "coherent_peak", "coherent_pick", "call_pcps_coherent")


def median(v):
    return float(np.median(v))


def timed(e, call, reps, scopes):
    """-> {wall_ms, <scope>_ms}: medians of `reps` warm calls; the stages' brackets, then the one bracket around the call."""
    call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    got = {k: [] for k in scopes}
    for calls_only in (False, True):
        e.prof_enable(True, calls_only=calls_only)
        try:
            for _ in range(reps):
                e.prof_reset()
                call()
                for k in scopes:
                    if k.startswith("call_") == calls_only:
                        got[k].append(e.prof_read(k)[0])
        finally:
            e.prof_enable(False)
    return dict(wall_ms=median(wall), **{k + "_ms": median(v) for k, v in got.items()})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    from sydr_amd import _lib
    from sydr_amd.dsp.signalsearch import NH20, pcps_coherent_statement
    from sydr_amd.engine import FMT_CI8, Engine

    lib = _lib.load()
    n = args.slots
    rng = np.random.default_rng(20261025)
    codes = (rng.integers(0, 2, (n, CHIPS)) * 2 - 1).astype(np.int8)
    row = dict(build_id=lib.sdr_build_id().decode(), slots=n, M=M, bins=lib.sdr_pcps_bins(RANGE, STEP), K=lib.sdr_acq_refine_bins(SPAN, FINE),
               reps=args.reps, shapes=[])
    e = Engine(0)
    try:
        for fs in (4e6,) if args.small_only else (4e6, 25e6):
            N = int(np.rint(fs * CHIPS / CODE_HZ))
            cap = ((M + 1) * N + 7) // 8 * 8
            e.iq_alloc(cap, FMT_CI8)
            e.code_slots(n + 1)
            e.load_gps_code(n, 1)
            e.iq_synth([dict(slot=n, doppler=1630.0, code_phase=300.25, phase=0.1, amp=4.0)], fs, 12.0, 20261025, 0, cap)
            for s in range(n):
                e.set_code(s, codes[s])
            slots = np.arange(n)

            def coherent():
                return e.pcps_coherent(slots, 0, NH20, 0, fs, 0.0, RANGE, STEP, CODE_HZ, M, SPAN, FINE)

            def padded():
                return e.pcps_signal(slots, 0, fs, 0.0, RANGE, STEP, CODE_HZ, pad=1, noncoh=M)
            out = dict(fs=fs, n_code=N, coherent=timed(e, coherent, args.reps, SCOPES),
                       padded=timed(e, padded, args.reps, ("call_pcps_signal",)))
            t0 = time.perf_counter()
            raw = e.iq_download((M + 1) * N, 0).astype(np.float64)
            x = raw[0::2] + 1j * raw[1::2]
            res, _, _ = pcps_coherent_statement(x, codes[:1], NH20, [0], fs, 0.0, RANGE, STEP, CODE_HZ, M, SPAN, FINE)
            out["statement_one_slot_wall_ms"] = (time.perf_counter() - t0) * 1e3
            dev = e.pcps_coherent([0], 0, NH20, 0, fs, 0.0, RANGE, STEP, CODE_HZ, M, SPAN, FINE)[0]
            out["statement_agrees"] = bool(all(int(res[0][k]) == int(dev[0][k]) for k in ("peak_bin", "peak_code", "fine_idx", "sec_phase")))
            row["shapes"].append(out)
    finally:
        e.close()
    line = json.dumps(row)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
