#!/usr/bin/env python3
"""Acquire a signal that is not GPS L1 C/A and hand it to the closed loop: a 4092-chip code with a BOC(1,1) sub-carrier whose
data sign changes every code period (4 ms), as Galileo E1-B does.

    python examples/acquire_e1_like.py [--fs 4.092e6] [--doppler 500] [--epochs 40] [--seed 7]

The code is a SEEDED STAND-IN, not a Galileo memory code.  What runs on one MI355X:
  1. the code goes into slot 0, its half-chip (BOC-doubled) code into slot 1; sdr_iq_synth writes slot 0 with the sub-carrier;
  2. `Engine.pcps_signal` searches slot 1 at 2.046 Mcps, circular (pad = 0) and zero-padded over two periods (pad = 1), with the
     BOC side peaks inside the exclusion window -- the code boundary lies inside the window, and in every block whose two
     periods differ in sign the circular search loses its peak to the neighbouring Doppler bins (here its peak ratio is the
     lower one); the padded search sees whole periods only;
  3. the closed loop (five taps, 4 ms epochs, one symbol per epoch) starts from the padded search's Doppler and code sample."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sydr_amd._lib import LoopCfg, TrackState                        # noqa: E402
from sydr_amd.dsp.signalsearch import boc_doubled                   # noqa: E402
from sydr_amd.engine import FMT_CI8, Engine                         # noqa: E402

CHIPS, CHIP_RATE, L1 = 4092, 1.023e6, 1575.42e6
FIVE = (-1.0, -0.5, 0.0, 0.5, 1.0)                                  # half chips: VE/VL on the BOC side peaks


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
    code = np.where(np.random.default_rng(args.seed).random(CHIPS) < 0.5, -1, 1).astype(np.int8)   # a stand-in, seeded
    cstep = CHIP_RATE * (1.0 + args.doppler / L1) / fs
    first = n_code // 2 + 37                                         # the sample a code period starts at
    e = Engine(0)
    try:
        e.iq_alloc(n, FMT_CI8)
        e.code_slots(2, 2 * CHIPS)
        e.set_code(0, code)
        e.set_code(1, boc_doubled(code).astype(np.int8))
        e.iq_synth([dict(slot=0, boc=True, doppler=args.doppler, code_phase=CHIPS - first * cstep, phase=0.1, amp=7.0)], fs, 14.0,
                   args.seed, 0, n)
        bins = np.arange(-1000.0, 1001.0, 250.0)
        excl = int(np.rint(fs / CHIP_RATE))                          # one chip = two half chips: the side peaks stay inside
        found = None
        for pad in (0, 1):
            pb, pc, pr, _ = e.pcps_signal([1], 0, fs, 0.0, 1000.0, 250.0, 2.0 * CHIP_RATE, pad=pad, excl_samples=excl, noncoh=2)
            doppler = -bins[int(pb[0])]                              # the searches mix with if_hz - bin: postAcquisitionUpdate's sign
            print(f"{'zero-padded' if pad else 'circular   '} search: Doppler {doppler:+7.1f} Hz, code sample {int(pc[0]):6d}, "
                  f"peak ratio {pr[0]:.2f}   (truth {args.doppler:+.1f} Hz, sample {first})")
            found = (doppler, int(pc[0]))
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
