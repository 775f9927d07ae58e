#!/usr/bin/env python3
"""What sdr_ddm (sydr_amd/csrc/ddm.hip) costs against the two ways a receiver had before it (docs/notes/ddm.md):

    python tools/ddm_cost.py [--json out.json] [--fs 25e6] [--items 32] [--ms 10] [--blocks 2] [--segments 8] [--taps 65]
                             [--chip-step 0.125] [--span 500] [--step 25] [--reps 5] [--timeout 540]

One MI355X, one JSON line.  A ci8 ring at `fs` from the device's synthesiser holds `items` satellites; every item is a
window of `ms` milliseconds around its satellite's state.
  (a) ddm           the call: its three kernels ("ddm_segments_kernel", "ddm_map_kernel", "ddm_peak_kernel") and the whole
                    call ("call_ddm") in stream time (HIP events, warm, medians of --reps calls), and the host clock around
                    the synchronous call without the tables (wall_ms) and with the map (wall_map_ms)
  (b) composed      the same map from what the library had: sdr_corr_profile on items x Q segment items (the segment's own
                    NCO state per item), the download of items x Q x taps complex sums, the statement's second stage in
                    NumPy -- corr_call_ms (stream), corr_wall_ms, second_stage_ms, composed_ms (host clock, all of it); the
                    largest difference between the two maps over the map's maximum is reported (map_difference)
  (c) pcps          the cold search a reacquisition cost: sdr_pcps(coh = 5, noncoh = 2, +-5 kHz by 250 Hz) for the same
                    PRNs -- call_ms (stream, "call_pcps" when the library records it) and wall_ms.  With --only-pcps
                    nothing else runs: the figure of another build (SYDR_AMD_LIB) on the same box.
Nothing is asserted about any ratio.  The measuring process runs under its own `timeout`; the driver never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np


def measure(args):
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine, make_items

    fs, n_items, B, S, T = args.fs, args.items, args.blocks, args.segments, args.taps
    Q = B * S
    n = int(round(fs * 1e-3))
    W = int(round(fs * 1e-3 * args.ms))
    first = -(T - 1) / 2 * args.chip_step
    e = Engine(0)
    try:
        cap = (W + 12 * n + 7) // 8 * 8
        e.iq_alloc(cap, FMT_CI8)
        e.code_slots(n_items)
        sats = []
        for s in range(n_items):
            e.load_gps_code(s, s + 1)
            sats.append(dict(prn=s + 1, doppler=-4000.0 + 250.0 * s + 40.0, code_phase=31.0 * s + 0.5, phase=0.1 * s, amp=4.0))
        e.iq_synth(sats, fs, 12.0, 20260020, 0, cap)
        row = dict(build_id=_lib.load().sdr_build_id().decode(), fs=fs, items=n_items, window_samples=W, blocks=B, segments=S,
                   taps=T, chip_step=args.chip_step, span_hz=args.span, step_hz=args.step, reps=args.reps)

        # ---- (c) the cold search
        def cold():
            return e.pcps(list(range(n_items)), 0, fs, 0.0, 5000.0, 250.0, coh=5, noncoh=2)
        cold()
        wall, whole = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            cold()
            wall.append((time.perf_counter() - t0) * 1e3)
        e.prof_enable(True, calls_only=True)
        try:
            for _ in range(args.reps):
                e.prof_reset()
                cold()
                whole.append(e.prof_read("call_pcps")[0])
        finally:
            e.prof_enable(False)
        row["pcps"] = dict(wall_ms=float(np.median(wall)), call_ms=float(np.median(whole)))
        if args.only_pcps:
            return row

        # every item: its satellite's state at sample s0, the code phase off by 1.5 chips, the carrier by 90 Hz
        s0 = 1000
        step = 1.023e6 / fs
        rows = [(s, W, s0, sat["doppler"] - 90.0, 0.0, (sat["code_phase"] + s0 * step * (1.0 + sat["doppler"] / 1575.42e6)) % 1023.0 + 1.5,
                 step) for s, sat in enumerate(sats)]
        items = make_items(*(np.array(col) for col in zip(*rows)))

        # ---- (a) the call
        def call(**kw):
            return e.ddm(items, fs, B, S, first, args.chip_step, T, args.span, args.step, **kw)
        res, cmap, _ = call()
        wall, wall_map = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call(want_map=False)
            t1 = time.perf_counter()
            call()
            wall.append((t1 - t0) * 1e3)
            wall_map.append((time.perf_counter() - t1) * 1e3)
        scopes = {k: [] for k in ("ddm_segments_kernel", "ddm_map_kernel", "ddm_peak_kernel", "call_ddm")}
        for calls_only in (False, True):
            e.prof_enable(True, calls_only=calls_only)
            try:
                for _ in range(args.reps):
                    e.prof_reset()
                    call(want_map=False)
                    for k in scopes:
                        if (k == "call_ddm") == calls_only:
                            scopes[k].append(e.prof_read(k)[0])
            finally:
                e.prof_enable(False)
        row["ddm"] = dict(wall_ms=float(np.median(wall)), wall_map_ms=float(np.median(wall_map)),
                          **{k + "_ms": float(np.median(v)) for k, v in scopes.items()})
        peak = res["peak_chips"] + items["rem_code"]
        row["ddm"]["worst_phase_error_chips"] = float(np.abs((peak - [(sat["code_phase"] + s0 * step * (1.0 + sat["doppler"] / 1575.42e6)) % 1023.0
                                                                      for sat in sats] + 511.5) % 1023.0 - 511.5).max())
        row["ddm"]["worst_carrier_error_hz"] = float(np.abs(res["peak_hz"] - [sat["doppler"] for sat in sats]).max())

        # ---- (b) composed from sdr_corr_profile and NumPy
        K = e.ddm_bins(args.span, args.step)
        d = (np.arange(K) - (K - 1) // 2) * args.step

        def composed(timing=None):
            t0 = time.perf_counter()
            seg, tau = [], np.zeros((n_items, Q))
            for i, (slot, _, start, f0, remc, remk, cstep) in enumerate(rows):
                for q in range(Q):
                    a, b = (q * W) // Q, ((q + 1) * W) // Q
                    seg.append((slot, b - a, start + a, f0, (remc + (-(f0 * 2.0 * np.pi * a / fs))) % (2 * np.pi), remk + float(a) * cstep, cstep))
                    tau[i, q] = (a + b - 1) / 2.0 / fs
            seg_items = make_items(*(np.array(col) for col in zip(*seg)))
            t1 = time.perf_counter()
            out = e.corr_profile(seg_items, first, args.chip_step, T, fs)
            t2 = time.perf_counter()
            z = (out[..., 0] + 1j * out[..., 1]).reshape(n_items, B, S, T)
            rot = np.exp(-2j * np.pi * d[None, None, :] * tau[:, :, None]).reshape(n_items, B, S, K)
            Z = np.einsum("ibsk,ibst->ibkt", rot, z)
            m = (np.abs(Z) ** 2).sum(axis=1)
            t3 = time.perf_counter()
            if timing is not None:
                timing.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3))
            return m
        ref = composed()
        timing, corr_call = [], []
        for _ in range(args.reps):
            composed(timing)
        e.prof_enable(True, calls_only=True)
        try:
            for _ in range(args.reps):
                e.prof_reset()
                composed()
                corr_call.append(e.prof_read("call_corr_profile")[0])
        finally:
            e.prof_enable(False)
        t = np.median(np.array(timing), axis=0)
        row["composed"] = dict(items_ms=float(t[0]), corr_wall_ms=float(t[1]), second_stage_ms=float(t[2]), composed_ms=float(t[3]),
                               corr_call_ms=float(np.median(corr_call)), segment_items=n_items * Q,
                               map_difference=float(np.abs(ref - cmap).max() / cmap.max()))
        return row
    finally:
        e.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--fs", type=float, default=25e6)
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--ms", type=float, default=10.0)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--taps", type=int, default=65)
    ap.add_argument("--chip-step", type=float, default=0.125)
    ap.add_argument("--span", type=float, default=500.0)
    ap.add_argument("--step", type=float, default=25.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-pcps", action="store_true", help="time the cold search alone (another build through SYDR_AMD_LIB)")
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
    for k in ("fs", "items", "ms", "blocks", "segments", "taps", "span", "step", "reps"):
        cmd += ["--" + k, str(getattr(args, k))]
    cmd += ["--chip-step", str(args.chip_step)]
    if args.only_pcps:
        cmd.append("--only-pcps")
    if args.json:
        cmd += ["--json", args.json]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
