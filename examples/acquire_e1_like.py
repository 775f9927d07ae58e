#!/usr/bin/env python3
"""Acquire a signal that is not GPS L1 C/A and hand it to the closed loop: a 4092-chip code with a BOC(1,1) sub-carrier whose
sign changes from one code period (4 ms) to the next under a 25-chip secondary code, as Galileo E1-C's does.

    python examples/acquire_e1_like.py [--fs 4.092e6] [--doppler 500] [--epochs 40] [--seed 7]

The codes are SEEDED STAND-INS, not Galileo's memory or secondary codes.  What runs on one MI355X:
  1. the code goes into slot 0, its half-chip (BOC-doubled) code into slot 1; the host makes the signal -- the doubled code
     under the secondary code, carrier, noise -- and uploads it (the device's synthesiser knows no secondary code);
  2. `Engine.pcps_signal` searches slot 1 at 2.046 Mcps, circular (pad = 0) and zero-padded over two periods (pad = 1), with the
     BOC side peaks inside the exclusion window -- the code boundary lies inside the window, and in every block whose two
     periods differ in sign the circular search loses its peak to the neighbouring Doppler bins (here its peak ratio is the
     lower one); the padded search sees whole periods only;
  3. `Engine.acq_secondary` takes the padded search's code sample and Doppler to the secondary code's phase and to the carrier
     on a 5 Hz grid -- what lets the prompts of several periods be added coherently;
  4. the closed loop (five taps, 4 ms epochs, one symbol per epoch) starts from the padded search's Doppler and code sample."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sydr_amd._lib import LoopCfg, TrackState                        # noqa: E402
from sydr_amd.dsp.signalsearch import boc_doubled                   # noqa: E402
from sydr_amd.engine import FMT_CI8, Engine, make_secondary_items   # noqa: E402

CHIPS, CHIP_RATE, L1 = 4092, 1.023e6, 1575.42e6
FIVE = (-1.0, -0.5, 0.0, 0.5, 1.0)                                  # half chips: VE/VL on the BOC side peaks
SEC_CHIPS, SEC_AT_FIRST = 25, 8                                     # the secondary code, the chip the period at `first` carries


def synthesise(code2, sec, fs, doppler, first, n, amp, sigma, seed):
    """The half-chip code under the secondary code on a carrier, in noise -> int8 IQ, interleaved.  A code period begins at
    sample `first`, carrying secondary chip SEC_AT_FIRST."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    cstep = 2.0 * CHIP_RATE * (1.0 + doppler / L1) / fs
    chips = (len(code2) - first * cstep) + t * cstep
    period = np.floor(chips / len(code2)).astype(np.int64) + SEC_AT_FIRST - 1
    x = amp * code2[np.floor(chips).astype(np.int64) % len(code2)] * sec[period % len(sec)] * np.exp(1j * (2.0 * np.pi * doppler / fs * t + 0.1))
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.empty(2 * n, dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return raw


def loop_coefficients(noise_bw, damping, gain):
    wn = noise_bw * 8.0 * damping / (4.0 * damping ** 2 + 1.0)
    return gain / (wn * wn), 2.0 * damping / wn


def loop_cfg(fs):
    """A Kaplan-style FLL-assisted PLL and DLL with 4 ms epochs of 8184 half chips (one symbol per epoch)."""
    cfg = LoopCfg()
    cfg.loop_kind, cfg.n_taps, cfg.fs = 1, len(FIVE), fs
    for t, s in enumerate(FIVE):
        cfg.spacing_wide[t], cfg.spacing_narrow[t] = s, 0.5 * s
    cfg.dll_tau1, cfg.dll_tau2 = loop_coefficients(2.0, 0.7, 1.0)
    cfg.dll_pdi, cfg.dll_threshold = 0.004, 10.0
    cfg.fll_bw_pullin, cfg.fll_bw_wide, cfg.fll_bw_narrow = 20.0, 10.0, 5.0
    cfg.fll_thr_wide, cfg.fll_thr_narrow = 0.3, 0.6
    cfg.pll_bw_wide, cfg.pll_bw_narrow = 15.0, 10.0
    cfg.pll_thr_wide, cfg.pll_thr_narrow = 0.3, 0.6
    cfg.epoch_chips, cfg.epochs_per_bit, cfg.epoch_seconds = 2.0 * CHIPS, 1, 4e-3
    return cfg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fs", type=float, default=4.092e6)
    ap.add_argument("--doppler", type=float, default=500.0, help="of the synthesised signal [Hz]")
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args(argv)
    fs = args.fs
    n_code = int(np.rint(fs * CHIPS / CHIP_RATE))
    n = (args.epochs + 3) * n_code // 8 * 8
    rng = np.random.default_rng(args.seed)
    code = np.where(rng.random(CHIPS) < 0.5, -1, 1).astype(np.int8)   # a stand-in, seeded
    sec = np.where(rng.random(SEC_CHIPS) < 0.5, -1, 1).astype(np.int8)   # ... and so is the secondary code
    first = n_code // 2 + 37                                         # the sample a code period starts at
    e = Engine(0)
    try:
        e.iq_alloc(n, FMT_CI8)
        e.code_slots(2, 2 * CHIPS)
        e.set_code(0, code)
        e.set_code(1, boc_doubled(code).astype(np.int8))
        e.iq_upload(synthesise(boc_doubled(code).astype(np.float64), sec.astype(np.float64), fs, args.doppler, first, n, 7.0, 14.0,
                               args.seed), 0)
        bins = np.arange(-1000.0, 1001.0, 250.0)
        excl = int(np.rint(fs / CHIP_RATE))                          # one chip = two half chips: the side peaks stay inside
        found = None
        for pad in (0, 1):
            pb, pc, pr, _ = e.pcps_signal([1], 0, fs, 0.0, 1000.0, 250.0, 2.0 * CHIP_RATE, pad=pad, excl_samples=excl, noncoh=2)
            doppler = -bins[int(pb[0])]                              # the searches mix with if_hz - bin: postAcquisitionUpdate's sign
            print(f"{'zero-padded' if pad else 'circular   '} search: Doppler {doppler:+7.1f} Hz, code sample {int(pc[0]):6d}, "
                  f"peak ratio {pr[0]:.2f}   (truth {args.doppler:+.1f} Hz, sample {first})")
            found = (doppler, int(pc[0]))
        periods = min(args.epochs, 50)
        res = e.acq_secondary(make_secondary_items(1, 0, found[1], found[0], 2.0 * CHIP_RATE), sec, fs, periods)[0]
        print(f"secondary code over {periods} periods: phase {int(res['sec_phase'])} (truth {SEC_AT_FIRST}), carrier "
              f"{res['fine_hz']:+7.1f} Hz, best phase over the next {res['power'] / res['power_other']:.1f}")
        st = TrackState()
        st.code_slot, st.current_sample = 1, found[1]
        st.carrier_hz, st.code_hz = found[0], 2.0 * CHIP_RATE
        st.code_step = st.code_hz / fs
        st.n_samples = int(np.ceil(2.0 * CHIPS / st.code_step))
        st.fll_bw, st.pll_bw, st.lock_state = 20.0, 15.0, 1          # pull-in
        states, traj, bits, done = e.track_closed_loop_ex([st], loop_cfg(fs), args.epochs, want_bits=True, epochs_per_bit=1)
        t = traj[0]
        print(f"closed loop: {int(done[0])} of {args.epochs} epochs, lock state {int(t['lock_state'][-1])}, carrier "
              f"{t['carrier_hz'][-1]:+.2f} Hz, {len(bits[0])} symbols decided")
    finally:
        e.close()


if __name__ == "__main__":
    main()
