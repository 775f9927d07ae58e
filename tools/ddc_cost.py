#!/usr/bin/env python3
"""What the device's down-converter (sdr_ddc_push, sydr_amd/csrc/ddc.hip) costs against the yardsticks of
docs/notes/downconvert.md.

    python tools/ddc_cost.py [--json out.json] [--seconds 1.0]

One MI355X, one JSON line.  Four legs, one second of input each, pushed in one call from page-locked memory:
  ci8_50MHz_T33_D2      ci8 at 50 MHz, 33 taps, decimation 2 -> a ci8 ring at 25 MHz
  r8_38MHz_IF_T33_D2    real int8 at 38.192 MHz, IF 9.548 MHz (fs / 4), 33 taps, decimation 2 -> ci8 at 19.096 MHz
  ci16_25MHz_mix_only   ci16 at 25 MHz, one tap, decimation 1 (mixing only) -> ci16 at 25 MHz
  ci8_50MHz_T512_D16    ci8 at 50 MHz, 512 taps, decimation 16 -> ci8 at 3.125 MHz
Per leg, warm: the medians of 25 pushes by wall clock around the synchronous call and of 25 HIP-event brackets
(sdr_prof_enable: the whole call's scope "call_ddc_push" -- copy command and kernels --, then "ddc_kernel" and
"ddc_history_kernel"), and beside them
  parent_route_ms  (a) the only route without the converter: the NumPy statement (sydr_amd/signal/downconvert.py) on the host
                   plus Engine.iq_upload of its output, wall clock, once, same box, same run;
  hbm_ms           (b) one read of the input plus one write of the output at the rate sdr_hbm_copy_rate reports in this run;
  link_copy_ms     (c) the host-link copy of the same input bytes out of the same page-locked block (one copy command and the
                   wait for it), wall clock, median of 25, same run.
Conditions (exit status 1 when one fails): no leg's push is slower than (a); for the three legs with T <= 33 the kernel's
time is no longer than (c) -- ingest is bound by the link, a converter that hides behind the copy costs the stream nothing.
The T = 512 leg is reported, not conditioned."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPS = 25


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of the input")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI16, FMT_CI8, Engine
    from sydr_amd.signal import downconvert as dc

    legs = [("ci8_50MHz_T33_D2", dc.IN_CI8, 50e6, 0.0, 33, 2, FMT_CI8, 1.0, True),
            ("r8_38MHz_IF_T33_D2", dc.IN_R8, 38.192e6, 9.548e6, 33, 2, FMT_CI8, 2.0, True),
            ("ci16_25MHz_mix_only", dc.IN_CI16, 25e6, 1.0e6, 1, 1, FMT_CI16, 1.0, True),
            ("ci8_50MHz_T512_D16", dc.IN_CI8, 50e6, 0.0, 512, 16, FMT_CI8, 1.0, False)]
    rng = np.random.default_rng(20260018)
    e = Engine(0)
    out = dict(build_id=_lib.load().sdr_build_id().decode(), seconds=args.seconds, reps=REPS, rows=[])
    ok = True
    try:
        out["hbm_copy_gbps"] = e.hbm_copy_rate(1 << 30, 10)
        for name, in_fmt, fs_in, shift, T, D, ring_fmt, gain, conditioned in legs:
            n_in = int(fs_in * args.seconds) // (64 * D) * (64 * D)      # (both rings whole granules)
            n_out = n_in // D
            per = 2 if dc.input_is_complex(in_fmt) else 1
            dtype = dc.input_dtype(in_fmt)
            amp = 100 if dtype == np.int8 else 2500
            block = e.host_alloc(per * n_in, dtype)
            block[:] = rng.integers(-amp, amp + 1, per * n_in).astype(dtype)
            in_bytes, out_bytes = block.nbytes, n_out * (2 if ring_fmt == FMT_CI8 else 4)
            cfg = dc.DownConverterConfig(in_fmt, D, dc.design_lowpass(T, 0.45 / D), dc.frequency_word(shift, fs_in), gain)
            # (c) the link: the same bytes by one copy command into a ring that takes them as they are (ci16: no sign flip behind it)
            e.iq_alloc(in_bytes // 4, FMT_CI16)
            as_i16 = block.view(np.int16)

            def link():
                e.iq_upload_queue(as_i16, 0)
                e.sync()
            for _ in range(3):
                link()
            link_ms = median_ms(link)
            e.iq_alloc(n_out, ring_fmt)
            ddc = e.ddc_create(cfg)

            def push():
                e.ddc_reset(ddc)
                e.ddc_push(ddc, block, 0)
            for _ in range(3):
                push()
            row = dict(leg=name, n_in=n_in, n_out=n_out, taps=T, decimation=D, in_bytes=in_bytes, out_bytes=out_bytes,
                       wall_ms=median_ms(push), call_ms=event_ms(e, push, "call_ddc_push", True),
                       kernel_ms=event_ms(e, push, "ddc_kernel", False), history_kernel_ms=event_ms(e, push, "ddc_history_kernel", False),
                       link_copy_ms=link_ms, hbm_ms=(in_bytes + out_bytes) / (out["hbm_copy_gbps"] * 1e9) * 1e3)
            got = e.iq_download(n_out, 0)
            e.ddc_destroy(ddc)
            print(f"{name}: device done, the statement on the host ...", file=sys.stderr, flush=True)
            # (a) the parent's only route, once: the statement on the host, then an ordinary upload of its output
            t0 = time.perf_counter()
            want = dc.statement(cfg, [block], ring_fmt)
            e.iq_upload(want, 0)
            row["parent_route_ms"] = (time.perf_counter() - t0) * 1e3
            row["equal_to_statement"] = bool(np.array_equal(got, want))
            row["speedup_over_parent_route"] = row["parent_route_ms"] / row["wall_ms"]
            row["not_slower_than_parent_route"] = bool(row["wall_ms"] <= row["parent_route_ms"])
            row["kernel_over_link_copy"] = row["kernel_ms"] / link_ms
            row["kernel_over_hbm"] = row["kernel_ms"] / row["hbm_ms"]
            row["conditioned_on_link"] = conditioned
            row["kernel_hides_behind_link_copy"] = bool(row["kernel_ms"] <= link_ms)
            ok = ok and row["not_slower_than_parent_route"] and (row["kernel_hides_behind_link_copy"] or not conditioned)
            out["rows"].append(row)
            del got, want
            e.host_free(block)
            print(f"{name}: " + json.dumps(row), file=sys.stderr, flush=True)
        out["conditions_hold"] = bool(ok)
    finally:
        e.close()
    text = json.dumps(out)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
