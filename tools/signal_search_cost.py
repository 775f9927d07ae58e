#!/usr/bin/env python3
"""What sdr_pcps_signal's zero-padded search costs, against the circular search at the same N and against what a user of the
library before it had to do for the same map (docs/notes/signal_search.md):

    python tools/signal_search_cost.py [--fs 4.092e6] [--slots 32] [--noncoh 2] [--reps 5] [--range 1000] [--step 250] [--json out]

One MI355X, one JSON line.  A ci8 ring at `fs` from the device's synthesiser, `slots` seeded 4092-chip codes at 1.023 Mcps
(N = fs * 4 ms: 16368 at 4.092 MHz, 200 000 at 50 MHz).
  (a) padded      Engine.pcps_signal(pad = 1), indices and ratio only and with the map: "call_pcps_signal" in stream time and
                  the host clock around the synchronous call (medians of --reps warm calls)
  (b) circular    Engine.pcps_signal(pad = 0) at the same N, the same two figures
  (c) composed    the same map without the call: sdr_pcps_spectra with host-made conj(fft(replica + N zeros)) of 2N samples,
                  one call per non-coherent block at start + j N (overlapping windows), the 2N-column maps downloaded, the host's
                  fold to N columns and their sum -- host clock, all of it, the spectra made once outside the clock; the largest
                  difference to (a)'s map over its maximum is reported
A library without sdr_pcps_signal (another build through SYDR_AMD_LIB) runs (c) alone.  Nothing is asserted about any ratio."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median(v):
    return float(np.median(v))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=float, default=4.092e6)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--noncoh", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--range", type=float, default=1000.0)
    ap.add_argument("--step", type=float, default=250.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    from sydr_amd import _lib
    from sydr_amd.dsp import signalsearch as ss
    from sydr_amd.engine import FMT_CI8, Engine

    fs, n_prn, K = args.fs, args.slots, args.noncoh
    chips, rate = 4092, 1.023e6
    n_code = ss.samples_per_code(fs, chips, rate)
    # (a build from before the call: its prototype is dropped so that the library loads, and (c) runs alone)
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib._PROTOTYPES if not hasattr(probe, n)]:
        del _lib._PROTOTYPES[name]
    lib = _lib.load()
    has_call = "sdr_pcps_signal" in _lib._PROTOTYPES
    rng = np.random.default_rng(20261020)
    codes = np.where(rng.random((n_prn, chips)) < 0.5, -1, 1).astype(np.int8)
    row = dict(build_id=lib.sdr_build_id().decode(), fs=fs, slots=n_prn, n_code=n_code, noncoh=K, doppler_range=args.range,
               doppler_step=args.step, reps=args.reps, has_pcps_signal=has_call)
    e = Engine(0)
    try:
        cap = ((K + 2) * n_code + 7) // 8 * 8
        e.iq_alloc(cap, FMT_CI8)
        e.code_slots(n_prn, chips)
        for s in range(n_prn):
            e.set_code(s, codes[s])
        sats = [dict(slot=s, doppler=-1000.0 + 250.0 * (s % 9), code_phase=101.0 * s + 0.5, phase=0.1 * s, amp=4.0) for s in range(n_prn)]
        e.iq_synth(sats, fs, 12.0, 20261020, 0, cap)
        slots = list(range(n_prn))
        padded_map = None

        def timed(call, scope):
            call()
            wall = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            e.prof_enable(True, calls_only=True)
            stream = []
            try:
                for _ in range(args.reps):
                    e.prof_reset()
                    call()
                    stream.append(e.prof_read(scope)[0])
            finally:
                e.prof_enable(False)
            return dict(call_ms=median(stream), wall_ms=median(wall))

        if has_call:
            for name, pad in (("padded", 1), ("circular", 0)):
                for want_map in (False, True):
                    def call():
                        return e.pcps_signal(slots, 0, fs, 0.0, args.range, args.step, rate, pad=pad, noncoh=K, want_map=want_map,
                                             n_chips=chips)
                    row[name + ("_map" if want_map else "")] = timed(call, "call_pcps_signal")
            padded_map = e.pcps_signal(slots, 0, fs, 0.0, args.range, args.step, rate, pad=1, noncoh=K, want_map=True, n_chips=chips)[3]

        # (c) what the library offered before: 2N-point spectra from the host, one call per block, the fold on the host
        spectra = np.stack([np.conj(np.fft.fft(np.r_[ss.replica(c.astype(np.float64), fs, rate, n_code), np.zeros(n_code)])) for c in codes])

        def composed():
            total = None
            for j in range(K):
                cmap = e.pcps_spectra(spectra, j * n_code, fs, 0.0, args.range, args.step, 1, 1, want_map=True)[3]
                part = cmap[:, :, :n_code]
                total = part.copy() if total is None else total + part
            return total
        folded = composed()
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            composed()
            wall.append((time.perf_counter() - t0) * 1e3)
        row["composed"] = dict(wall_ms=median(wall), calls=K)
        if padded_map is not None:
            row["composed"]["map_difference"] = float(np.abs(folded - padded_map).max() / padded_map.max())
    finally:
        e.close()
    line = json.dumps(row)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
