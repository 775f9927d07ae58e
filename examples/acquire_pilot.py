#!/usr/bin/env python3
"""Acquire a weak pilot under a secondary (overlay) code: where the zero-padded search stays below the threshold, the coherent
search under secondary-code hypotheses finds code sample, Doppler bin, overlay phase and fine carrier in one call.

    python examples/acquire_pilot.py [--fs 4e6] [--doppler 877] [--periods 40] [--amp 0.5] [--seed 4]

What runs on one MI355X:
  1. the host makes the signal -- C/A PRN 7 as the primary code under NH20 (L5-Q's Neuman-Hofman code), carrier, noise of
     sigma = 20 -- and uploads it (the device's synthesiser knows no secondary code);
  2. `Engine.pcps_signal(pad=1, noncoh=M)` adds the M periods' magnitudes: its peak ratio;
  3. `Engine.pcps_coherent` adds the M periods' complex correlations under the 20 overlay phases and 11 fine frequencies: its
     peak ratio, code sample, overlay phase and carrier, against what was planted."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sydr_amd.dsp.signalsearch import NH20                           # noqa: E402
from sydr_amd.engine import FMT_CI8, Engine                          # noqa: E402

CHIPS, CHIP_RATE, L1, SIGMA = 1023, 1.023e6, 1575.42e6, 20.0
FIRST, PHASE_AT_FIRST = 1234, 4          # a code period begins at sample FIRST and carries overlay chip PHASE_AT_FIRST


def synthesise(code, fs, doppler, n, amp, seed):
    """The code under NH20 on a carrier, in noise -> int8 IQ, interleaved."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    cstep = CHIP_RATE * (1.0 + doppler / L1) / fs
    chips = (CHIPS - FIRST * cstep) + t * cstep
    period = np.floor(chips / CHIPS).astype(np.int64) + PHASE_AT_FIRST - 1 + len(NH20)
    x = amp * code[np.floor(chips).astype(np.int64) % CHIPS] * NH20[period % len(NH20)].astype(np.float64)
    x = x * np.exp(2j * np.pi * (doppler / fs * t + 0.2)) + SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.empty(2 * n, dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return raw


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=float, default=4e6)
    ap.add_argument("--doppler", type=float, default=877.0)
    ap.add_argument("--periods", type=int, default=40)
    ap.add_argument("--amp", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=4)
    args = ap.parse_args(argv)
    fs, M = args.fs, args.periods
    N = int(np.rint(fs * CHIPS / CHIP_RATE))
    n = (M + 1) * N // 8 * 8 + 8
    coarse = 250.0 * np.round(args.doppler / 250.0)          # five coarse bins around the rounded Doppler
    e = Engine(0)
    try:
        e.code_slots(1)
        e.load_gps_code(0, 7)
        code = e.read_code(0).astype(np.float64)
        e.iq_alloc(n, FMT_CI8)
        e.iq_upload(synthesise(code, fs, args.doppler, n, args.amp, args.seed), 0)
        pb, pc, pr, _ = e.pcps_signal([0], 0, fs, coarse, 500.0, 250.0, CHIP_RATE, pad=1, noncoh=M)
        print(f"padded search, {M} periods added as magnitudes: ratio {pr[0]:.2f} at code sample {pc[0]} (planted {FIRST})")
        r = e.pcps_coherent([0], 0, NH20, 0, fs, coarse, 500.0, 250.0, CHIP_RATE, M, span_hz=125.0, step_hz=25.0)[0][0]
        print(f"coherent search under the 20 overlay phases: ratio {r['peak_ratio']:.2f} at code sample {r['peak_code']}, overlay "
              f"phase {r['sec_phase']} (planted {PHASE_AT_FIRST}), carrier {r['carrier_hz']:.0f} Hz (planted {args.doppler:.0f}), "
              f"best over any other phase {r['power'] / r['power_other']:.2f}")
    finally:
        e.close()


if __name__ == "__main__":
    main()
