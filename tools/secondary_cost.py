#!/usr/bin/env python3
"""What sdr_acq_secondary costs, against the only route to the same table a library without it offers
(docs/notes/secondary.md):

    python tools/secondary_cost.py [--fs 25e6] [--items 32] [--reps 9] [--json out]

One MI355X, one JSON line.  A ci8 ring at `fs` from the device's synthesiser, `items` C/A primaries (GPS PRN 1..), one item per
code at its own start sample and coarse carrier, results only.  Two shapes: M = 40 periods under a 20-chip secondary code,
S = 4, K = 51, and M = 128 under a 100-chip code, S = 16, K = 401 (seeded rows; the synthesised signals carry none -- the cost
does not depend on what the search finds).
  (a) call        Engine.acq_secondary: "secondary_segments", "secondary_search", "secondary_pick" and "call_secondary" in
                  stream time, the host clock around the synchronous call (medians of --reps warm calls)
  (b) composed    the segment sums from Engine.acq_refine(..., want_tables=True) in windows of at most 20 periods (each window's
                  carrier phase restarts: the host turns it back), then stage 2 in NumPy on the host (the phasors, one matrix
                  product per item for all hypotheses) -- host clock, all of it; the largest difference of its power table to
                  (a)'s over the table's maximum is reported
A library without sdr_acq_secondary (another build through SYDR_AMD_LIB) runs (b) alone.  Nothing is asserted about any ratio."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (dict(M=40, Ls=20, S=4, span=125.0, step=5.0), dict(M=128, Ls=100, S=16, span=1000.0, step=5.0))
CODE_HZ, CHIPS = 1.023e6, 1023


def median(v):
    return float(np.median(v))


def host_stage2(z, N, fs, f0, first, sec, span, step):
    """P[Ls][K] of one item from window-wise segment sums: z[M][S], `first`[M] = the period each one's window began at."""
    M, S = z.shape
    m = np.arange(M)[:, None]
    s = np.arange(S)[None, :]
    a, b = m * N + (s * N) // S, m * N + ((s + 1) * N) // S
    tau = (a + b - 1) / 2.0 / fs
    z = z * np.exp(-2j * np.pi * f0 * (first[:, None] * N) / fs)      # the carrier phase a later window restarted with
    K = 2 * int(np.floor(span / step)) + 1
    d = (np.arange(K) - (K - 1) // 2) * step
    per = (z[:, :, None] * np.exp(-2j * np.pi * d[None, None, :] * tau[:, :, None])).sum(axis=1)
    Ls = len(sec)
    w = sec[(np.arange(Ls)[:, None] + np.arange(M)[None, :]) % Ls].astype(np.float64)
    return np.abs(w @ per) ** 2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=float, default=25e6)
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine, make_refine_items

    # (a build from before the call: its prototype is dropped so that the library loads, and (b) runs alone)
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib._PROTOTYPES if not hasattr(probe, n)]:
        del _lib._PROTOTYPES[name]
    lib = _lib.load()
    has_call = "sdr_acq_secondary" in _lib._PROTOTYPES
    fs, n = args.fs, args.items
    N = int(np.rint(fs * CHIPS / CODE_HZ))
    row = dict(build_id=lib.sdr_build_id().decode(), fs=fs, items=n, n_code=N, reps=args.reps, has_acq_secondary=has_call, shapes=[])
    e = Engine(0)
    try:
        cap = (130 * N + 7) // 8 * 8
        e.iq_alloc(cap, FMT_CI8)
        e.code_slots(n)
        for s in range(n):
            e.load_gps_code(s, s + 1)
        sats = [dict(slot=s, doppler=-2000.0 + 250.0 * (s % 17), code_phase=31.0 * s + 0.5, phase=0.1 * s, amp=4.0) for s in range(n)]
        e.iq_synth(sats, fs, 12.0, 20261021, 0, cap)
        starts = np.array([101 * s for s in range(n)], dtype=np.int64)
        carriers = np.array([s["doppler"] for s in sats])
        rng = np.random.default_rng(20261021)
        for shp in SHAPES:
            M, Ls, S, span, step = shp["M"], shp["Ls"], shp["S"], shp["span"], shp["step"]
            sec = (rng.integers(0, 2, Ls) * 2 - 1).astype(np.int8)
            out = dict(shp, K=e.acq_refine_bins(span, step))
            table = None
            if has_call:
                from sydr_amd.engine import make_secondary_items
                items = make_secondary_items(np.arange(n), 0, starts, carriers, CODE_HZ)

                def call():
                    return e.acq_secondary(items, sec, fs, M, S, span, step)
                call()
                wall = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    call()
                    wall.append((time.perf_counter() - t0) * 1e3)
                scopes = {k: [] for k in ("secondary_segments", "secondary_search", "secondary_pick", "call_secondary")}
                for calls_only in (False, True):      # (the stages' brackets, then the one bracket around the whole call)
                    e.prof_enable(True, calls_only=calls_only)
                    try:
                        for _ in range(args.reps):
                            e.prof_reset()
                            call()
                            for k in scopes:
                                if k.startswith("call_") == calls_only:
                                    scopes[k].append(e.prof_read(k)[0])
                    finally:
                        e.prof_enable(False)
                out["call"] = dict(wall_ms=median(wall), **{k + "_ms": median(v) for k, v in scopes.items()})
                table = e.acq_secondary(items, sec, fs, M, S, span, step, want_tables=True)[1]

            first = np.concatenate([np.full(min(20, M - m0), m0) for m0 in range(0, M, 20)])

            def composed():
                zs = [e.acq_refine(make_refine_items(np.arange(n), starts + m0 * N, carriers, CODE_HZ), fs, min(20, M - m0), S, span, step,
                                   want_tables=True)[2] for m0 in range(0, M, 20)]
                z = np.concatenate(zs, axis=1)
                return np.stack([host_stage2(z[i], N, fs, carriers[i], first, sec, span, step) for i in range(n)])
            host = composed()
            wall = []
            for _ in range(max(3, args.reps // 3)):
                t0 = time.perf_counter()
                composed()
                wall.append((time.perf_counter() - t0) * 1e3)
            out["composed"] = dict(wall_ms=median(wall), refine_calls=len(range(0, M, 20)))
            if table is not None:
                out["composed"]["table_difference"] = float(np.abs(host - table).max() / table.max())
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
