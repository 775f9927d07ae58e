#!/usr/bin/env python3
"""What sdr_corr_profile costs against the only way to get the same numbers without it: Engine.epl_batch in chunks of 8 taps.

    python tools/corr_profile_cost.py [--package-root DIR] [--baseline-only] [--json out.json]

Workload: 32 items (8 staged C/A codes, different starts, carriers and rem_code) on a synthesised ci8 ring at 25, 10 and
4 MHz; tap counts 9, 17, 65, 129 and 1024 on a +-2 chip grid.  Warm; per configuration the medians of 25 calls by wall
clock and of 25 HIP-event brackets (sdr_prof_enable: the whole call's "call_*" scope, then the per-stage scopes).
`--package-root DIR` imports sydr_amd from DIR instead of this tree (a build of the parent commit: run with
`--baseline-only` there, in a process of its own on the same box).  Prints one JSON object; docs/notes/corr_profile.md holds
a run."""
import argparse
import json
import os
import sys
import time

import numpy as np

TAPS = (9, 17, 65, 129, 1024)
REPS = 25
SATS = ((3, 1630.0, 100.5), (7, -2381.0, 300.25), (11, 4120.0, 612.75), (14, 877.0, 17.5),
        (19, -3499.0, 900.0), (22, 2244.0, 455.5), (27, -1113.0, 250.25), (31, 3368.0, 777.0))


def median_ms(call, reps=REPS):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def event_ms(engine, call, prefix, calls_only, reps=REPS):
    """Median over `reps` calls of the summed duration of the scopes whose name starts with `prefix`."""
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--baseline-only", action="store_true", help="time the epl_batch composition alone (a library without the call)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.package_root)
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine, make_items

    e = Engine(0)
    out = dict(package_root=args.package_root, build_id=_lib.load().sdr_build_id().decode(), rows=[])
    try:
        e.code_slots(8)
        for slot, (prn, _, _) in enumerate(SATS):
            e.load_gps_code(slot, prn)
        for fs in (25e6, 10e6, 4e6):
            N = int(round(fs * 1e-3))
            cap = 8 * N // 8 * 8
            e.iq_alloc(cap, FMT_CI8)
            e.iq_synth([dict(prn=p, doppler=d, code_phase=c, phase=0.1 * k, amp=3.0) for k, (p, d, c) in enumerate(SATS)],
                       fs, 30.0, 20260009, 0, cap)
            k = np.arange(32)
            dop = np.array([SATS[i % 8][1] for i in k])
            phase = np.array([SATS[i % 8][2] for i in k])
            cstep = 1.023e6 * (1.0 + dop / 1575.42e6) / fs
            rem = np.array([0.25, -0.3, 0.9999999, 1e-12])[k // 8]
            n = np.ceil((1023 - rem) / cstep).astype(np.int64)
            start = np.ceil((1023 - phase + rem) / cstep).astype(np.int64) + (k // 8) * N
            items = make_items(k % 8, n, start, dop + 2.0, 0.1 * k, rem, cstep)
            for taps in TAPS:
                first, step = -2.0, 4.0 / (taps - 1)
                spacing = first + step * np.arange(taps)

                def composition():
                    return np.concatenate([e.epl_batch(items, spacing[j:j + 8], fs).reshape(32, -1, 2)
                                           for j in range(0, taps, 8)], axis=1)
                for _ in range(3):
                    ref = composition()
                row = dict(fs=fs, taps=taps, calls_of_composition=(taps + 7) // 8,
                           composition_wall_ms=median_ms(composition),
                           composition_kernel_ms=event_ms(e, composition, "epl_kernel", False))
                if not args.baseline_only:
                    forms = [("default", 0)] + ([("per_sample_forced", 1)] if fs == 25e6 else [])
                    for form, forced in forms:
                        e.set_option("corr_profile_per_sample", forced)

                        def profile():
                            return e.corr_profile(items, first, step, taps, fs)
                        for _ in range(3):
                            got = profile()
                        peak = np.hypot(ref[..., 0], ref[..., 1]).max(axis=1)
                        row[form] = dict(wall_ms=median_ms(profile), call_ms=event_ms(e, profile, "call_corr_profile", True),
                                         # (whichever form the library chose: the other scope is empty)
                                         kernel_ms=event_ms(e, profile, "corr_walk_kernel", False) + event_ms(e, profile, "corr_per_sample_kernel", False),
                                         upload_ms=event_ms(e, profile, "corr_items_upload", False),
                                         worst_difference=float((np.abs(got - ref).reshape(32, -1).max(axis=1) / peak).max()))
                        e.set_option("corr_profile_per_sample", 0)
                    row["ratio_wall"] = row["default"]["wall_ms"] / row["composition_wall_ms"]
                out["rows"].append(row)
    finally:
        e.close()
    text = json.dumps(out)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
