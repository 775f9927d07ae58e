#!/usr/bin/env python3
"""What sdr_iq_probe costs against the two yardsticks of docs/notes/probe.md.

    python tools/probe_cost.py [--json out.json] [--seconds 1.0]

One MI355X, one JSON line.  The window is one second at 25 MHz (25 000 000 samples), the ring exactly that long.
Streams: a ci8 ring of synthesised noise; the same ring after a 2-bit packed upload of its samples (four values per
component: every lane of a wave adds into the same few histogram counters); a ci16 ring; a cf32 ring.
Legs: moments only; moments + histogram (integer rings); moments + spectrum at nfft 1024 and 4096.
Per leg, warm: the medians of 25 calls by wall clock and of 25 HIP-event brackets (the whole call's scope, then the kernels'
scopes), and beside them
  parent_route_ms  the same answer through the only route without the call: Engine.iq_download of the window plus the NumPy
                   statement (sydr_amd/signal/probe.py), wall clock, median of 3, same box, same run;
  hbm_read_ms      one read of the window at the rate sdr_hbm_copy_rate reports on this GPU (bytes / rate)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPS, BASE_REPS = 25, 3
FS = 25e6


def median_ms(call, reps):
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of the window")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CF32, FMT_CI16, FMT_CI8, Engine
    from sydr_amd.signal import packing as pk
    from sydr_amd.signal import probe as pb

    n = int(FS * args.seconds) // 8 * 8
    rng = np.random.default_rng(20260017)
    e = Engine(0)
    out = dict(build_id=_lib.load().sdr_build_id().decode(), window_samples=n, fs=FS, reps=REPS, parent_route_reps=BASE_REPS, rows=[])
    try:
        out["hbm_copy_gbps"] = e.hbm_copy_rate(1 << 30, 10)
        e.code_slots(1)
        e.load_gps_code(0, 9)

        def measure(stream, fmt_bytes, integer):
            legs = [("moments", dict(hist=False))]
            if integer:
                legs.append(("moments_hist", dict(hist=True)))
            legs += [("moments_psd_1024", dict(hist=False, nfft=1024, fs=FS)), ("moments_psd_4096", dict(hist=False, nfft=4096, fs=FS))]
            hbm_ms = n * fmt_bytes / (out["hbm_copy_gbps"] * 1e9) * 1e3
            for leg, kw in legs:
                call = lambda: e.iq_probe(0, n, **kw)
                for _ in range(3):
                    got = call()

                def parent():
                    raw = e.iq_download(n, 0)
                    return pb.probe(raw, nfft=kw.get("nfft", 0), fs=kw.get("fs"))
                want = parent()
                row = dict(stream=stream, leg=leg, window_bytes=n * fmt_bytes, hbm_read_ms=hbm_ms,
                           wall_ms=median_ms(call, REPS), call_ms=event_ms(e, call, "call_iq_probe", True),
                           moments_kernel_ms=event_ms(e, call, "probe_moments_kernel", False),
                           psd_kernel_ms=event_ms(e, call, "probe_psd_kernel", False) if "nfft" in kw else 0.0,
                           parent_route_ms=median_ms(parent, BASE_REPS))
                row["times_hbm_read"] = row["call_ms"] / hbm_ms
                row["speedup_over_parent_route"] = row["parent_route_ms"] / row["wall_ms"]
                row["not_slower_than_parent_route"] = bool(row["wall_ms"] <= row["parent_route_ms"])
                if integer:
                    row["equal_to_statement"] = bool(got.raw() == dict(want.raw(), n_segments=got.n_segments)
                                                     and (got.hist is None or np.array_equal(got.hist, want.hist)))
                if "nfft" in kw:
                    row["psd_worst_of_peak"] = float(np.max(np.abs(got.psd - want.psd)) / want.psd.max())
                out["rows"].append(row)

        e.iq_alloc(n, FMT_CI8)
        e.iq_synth([dict(slot=0, doppler=1500.0, code_phase=10.0, amp=2.0)], FS, 25.0, 20260018, 0, n)
        measure("ci8_noise", 2, True)
        raw = e.iq_download(n, 0)
        p = pk.Packing(2)
        packed = pk.pack(pk.quantise(raw, 2, float(raw.astype(np.float64).std()), p), p)
        del raw
        e.iq_upload_packed(packed, n, p, 0)
        measure("ci8_after_2bit_packed_upload", 2, True)
        e.iq_alloc(n, FMT_CI16)
        e.iq_upload(np.clip(np.rint(rng.standard_normal(2 * n, dtype=np.float32) * 2500.0), -32768, 32767).astype(np.int16), 0)
        measure("ci16_noise", 4, True)
        e.iq_alloc(n, FMT_CF32)
        e.iq_upload(rng.standard_normal(2 * n, dtype=np.float32), 0)
        measure("cf32_noise", 8, False)
    finally:
        e.close()
    text = json.dumps(out)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
