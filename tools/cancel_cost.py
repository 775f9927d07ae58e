#!/usr/bin/env python3
"""What sdr_iq_cancel (sydr_amd/csrc/cancel.hip) costs against the only way to get the same samples without it: download the
window, subtract the replicas in NumPy (sydr_amd/signal/cancel.py: cancel_statement), upload (docs/notes/cancel.md).

    python tools/cancel_cost.py [--json out.json] [--fs 25e6] [--seconds 1.0] [--channels 1,4,8] [--reps 5] [--timeout 540]

One MI355X, one JSON line.  A ci8 ring of `seconds` at `fs` from the device's synthesiser; per channel one epoch per code period
(fs / 1000 samples), NCO state carried from epoch to epoch, amplitudes a few LSB.  For each channel count:
  kernel_ms / call_ms   the in-stream time of the kernel (scope "cancel_kernel") and of the whole call ("call_iq_cancel":
                        the item upload, the kernel), HIP events, warm, medians of --reps calls in place
  wall_ms               the host clock around the synchronous call (it ends in a stream synchronise)
  host_ms               iq_download + cancel_statement + iq_upload on the same box, once (download_ms, statement_ms, upload_ms)
  floor_ms              the window read once and written once at the rate sdr_hbm_copy_rate measures on this GPU
Nothing is asserted about any ratio.  The measuring process runs under its own `timeout`; the driver never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np


def chain(slot, n, n_epochs, start, carrier_hz, fs):
    """One channel's items, the NCO state carried from epoch to epoch (closed form: every epoch has n samples)."""
    from sydr_amd.engine import make_items
    step = 1.023e6 * (1.0 + carrier_hz / 1575.42e6) / fs
    k = np.arange(n_epochs, dtype=np.float64)
    rem_code = np.remainder(k * (n * step - 1023.0) + 0.25, 1.0)
    rem_carrier = np.remainder(-k * (carrier_hz * 2.0 * np.pi * n / fs), 2.0 * np.pi)
    return make_items(slot, n, start + np.arange(n_epochs, dtype=np.int64) * n, carrier_hz, rem_carrier, rem_code, step)


def measure(args):
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine
    from sydr_amd.signal import cancel as cn

    fs = args.fs
    n = int(round(fs * 1e-3))
    n_epochs = int(round(args.seconds * 1e3))
    W = n * n_epochs
    counts = [int(c) for c in args.channels.split(",")]
    e = Engine(0)
    try:
        e.iq_alloc((W + 7) // 8 * 8, FMT_CI8)
        e.code_slots(max(counts))
        for s in range(max(counts)):
            e.load_gps_code(s, s + 1)
        e.iq_synth([dict(prn=s + 1, doppler=-4000.0 + 1000.0 * s, code_phase=100.0 * s, phase=0.1 * s, amp=4.0) for s in range(max(counts))],
                   fs, 12.0, 20260019, 0, W)
        gbps = e.hbm_copy_rate(1 << 28, 10)
        row = dict(build_id=_lib.load().sdr_build_id().decode(), fs=fs, window_samples=W, epochs=n_epochs, reps=args.reps,
                   hbm_copy_gbps=gbps, floor_ms=2.0 * W * 2 / (gbps * 1e9) * 1e3, cases=[])
        original = e.iq_download(W, 0)
        for n_ch in counts:
            items = np.stack([chain(s, n, n_epochs, 0, -4000.0 + 1000.0 * s, fs) for s in range(n_ch)])
            amps = np.zeros((n_ch, n_epochs, 2))
            amps[..., 0], amps[..., 1] = 1.618 * 2.0, -1.0

            def call():
                return e.iq_cancel(items, amps, fs, window=(0, W))

            e.iq_upload(original, 0)
            stats = call()
            wall, kern, whole = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            for calls_only, sink, scope in ((False, kern, "cancel_kernel"), (True, whole, "call_iq_cancel")):
                e.prof_enable(True, calls_only=calls_only)
                try:
                    for _ in range(args.reps):
                        e.prof_reset()
                        call()
                        sink.append(e.prof_read(scope)[0])
                finally:
                    e.prof_enable(False)
            case = dict(channels=n_ch, stats=stats, wall_ms=float(np.median(wall)), kernel_ms=float(np.median(kern)),
                        call_ms=float(np.median(whole)))
            if n_ch <= args.host_channels:
                e.iq_upload(original, 0)
                t0 = time.perf_counter()
                raw = e.iq_download(W, 0)
                t1 = time.perf_counter()
                x = raw[0::2].astype(np.float64) + 1j * raw[1::2].astype(np.float64)
                codes = [e.read_code(s).astype(np.float64) for s in range(n_ch)]
                res = cn.cancel_statement(x, FMT_CI8, [(items[s], amps[s], codes[s]) for s in range(n_ch)], fs, 0, None)
                out = np.empty(2 * W, dtype=np.int8)
                out[0::2], out[1::2] = res.window.real, res.window.imag
                t2 = time.perf_counter()
                e.iq_upload(out, 0)
                t3 = time.perf_counter()
                case.update(download_ms=(t1 - t0) * 1e3, statement_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3, host_ms=(t3 - t0) * 1e3)
                # (the device against the statement on the same input, at the size that was timed)
                e.iq_upload(original, 0)
                call()
                case["samples_that_differ_from_the_statement"] = int(np.count_nonzero(e.iq_download(W, 0) != out))
                case["statement_stats_equal"] = res.stats == stats
            row["cases"].append(case)
        return row
    finally:
        e.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--fs", type=float, default=25e6)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--channels", default="1,4,8")
    ap.add_argument("--host-channels", type=int, default=8, help="run the host route up to this many channels")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540, help="time limit of the measuring process in seconds")
    ap.add_argument("--inner", action="store_true", help="measure in this process (what the driver starts under `timeout`)")
    args = ap.parse_args(argv)
    if args.inner:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        text = json.dumps(measure(args))
        print(text)
        if args.json:
            with open(args.json, "w") as f:
                f.write(text + "\n")
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--inner"]
    for k in ("fs", "seconds", "channels", "reps"):
        cmd += ["--" + k, str(getattr(args, k))]
    cmd += ["--host-channels", str(args.host_channels)]
    if args.json:
        cmd += ["--json", args.json]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
