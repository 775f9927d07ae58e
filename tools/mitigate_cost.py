#!/usr/bin/env python3
"""What the device's pulse blanker and narrow-band excisor (sdr_ddc_mitigate, sydr_amd/csrc/mitigate.hip) cost against the
yardsticks of docs/notes/mitigate.md.

    python tools/mitigate_cost.py [--json out.json] [--seconds 1.0]

One MI355X, one JSON line.  Two legs, one second of ci8 input each (noise, a carrier wave, pulses), pushed in one call from
page-locked memory through a converter with a blanker (lead 2, hold 5) and an excisor of 1024 points:
  ci8_25MHz_identity    25 MHz through the identity converter (one tap, decimation 1) -> a ci8 ring at 25 MHz
  ci8_50MHz_T33_D2      50 MHz, 33 taps, decimation 2 -> a ci8 ring at 25 MHz
Per leg, warm: the medians of 25 pushes by wall clock around the synchronous call and of 25 HIP-event brackets
(sdr_prof_enable: the whole call's scope "call_ddc_push", then "ddc_kernel", "mit_blank_kernel", "mit_excise_kernel",
"mit_combine_kernel"), and beside them
  plain_*          the same converter WITHOUT the mitigator -- the path every other recording takes --, same run, same medians;
  statement_ms     the NumPy statements (signal/downconvert.py, then signal/mitigate.py) on the host, wall clock, once;
  counters_equal   the device's counters against the statement's (the gates of a random stream may, rarely, differ: reported).
Condition (exit status 1 when it fails): no leg's mitigated push is slower than the statement on the host."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPS = 25
NFFT, LEAD, HOLD, FACTOR, MARGIN_DB = 1024, 2, 5, 2.5, 10.0   # (the carrier wave raises the measured level: 2.5 times it catches the pulses)


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


def jammed(rng, n, block):
    """n ci8 samples into `block` (interleaved), made in pieces: noise of sigma 12, a carrier wave of amplitude 40, a pulse of
    12 samples every 40 000."""
    step = 1 << 22
    for lo in range(0, n, step):
        m = min(step, n - lo)
        x = 12.0 * (rng.standard_normal(m) + 1j * rng.standard_normal(m)) + 40.0 * np.exp(2j * np.pi * 0.0613 * (lo + np.arange(m)))
        for at in range((-lo) % 40000, m - 12, 40000):
            x[at:at + 12] += 110.0
        block[2 * lo:2 * (lo + m):2] = np.clip(np.rint(x.real), -127, 127)
        block[2 * lo + 1:2 * (lo + m):2] = np.clip(np.rint(x.imag), -127, 127)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of the input")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sydr_amd import _lib
    from sydr_amd.engine import FMT_CI8, Engine
    from sydr_amd.signal import downconvert as dc
    from sydr_amd.signal import mitigate as mt

    legs = [("ci8_25MHz_identity", 25e6, 1, 1), ("ci8_50MHz_T33_D2", 50e6, 33, 2)]
    rng = np.random.default_rng(20260019)
    e = Engine(0)
    out = dict(build_id=_lib.load().sdr_build_id().decode(), seconds=args.seconds, reps=REPS, nfft=NFFT, rows=[])
    ok = True
    try:
        for name, fs_in, T, D in legs:
            n_in = int(fs_in * args.seconds) // (64 * D) * (64 * D)
            n_out = n_in // D
            block = e.host_alloc(2 * n_in, np.int8)
            jammed(rng, n_in, block)
            cfg = dc.DownConverterConfig(dc.IN_CI8, D, dc.design_lowpass(T, 0.45 / D))
            head = dc.statement(cfg, [block[:2 * 8 * int(fs_in * 1e-3)]])                 # (8 ms, as the host layer calibrates)
            mcfg = mt.MitigationConfig(mt.blanking_level(head, FACTOR), LEAD, HOLD, NFFT, mt.excision_limits(head, NFFT, MARGIN_DB))
            e.iq_alloc(n_out, FMT_CI8)
            row = dict(leg=name, n_in=n_in, n_out=n_out, taps=T, decimation=D)
            for label, attach in (("plain_", False), ("", True)):
                ddc = e.ddc_create(cfg)
                if attach:
                    e.ddc_mitigate(ddc, mcfg)

                def push():
                    e.ddc_reset(ddc)
                    e.ddc_push(ddc, block, 0)
                for _ in range(3):
                    push()
                row[label + "wall_ms"] = median_ms(push)
                row[label + "call_ms"] = event_ms(e, push, "call_ddc_push", True)
                row[label + "ddc_kernel_ms"] = event_ms(e, push, "ddc_kernel", False)
                if attach:
                    for scope in ("mit_blank_kernel", "mit_excise_kernel", "mit_combine_kernel"):
                        row[scope + "_ms"] = event_ms(e, push, scope, False)
                    stats = e.ddc_mitigation_stats(ddc)
                    got = e.iq_download(n_out, 0)
                e.ddc_destroy(ddc)
            print(f"{name}: device done, the statements on the host ...", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            st = mt.Statement(mcfg)
            want = dc.quantise(st.push(dc.statement(cfg, [block])), dc.FMT_CI8)
            row["statement_ms"] = (time.perf_counter() - t0) * 1e3
            row["counters_equal"] = bool(stats == st.stats)
            row["ring_bytes_differing"] = int(np.count_nonzero(got != want))
            row["n_triggers"], row["n_blanked"], row["n_bins_excised"] = stats.n_triggers, stats.n_blanked, stats.n_bins_excised
            row["mitigation_ms"] = row["call_ms"] - row["plain_call_ms"]
            row["speedup_over_statement"] = row["statement_ms"] / row["wall_ms"]
            row["not_slower_than_statement"] = bool(row["wall_ms"] <= row["statement_ms"])
            ok = ok and row["not_slower_than_statement"]
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
