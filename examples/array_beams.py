#!/usr/bin/env python3
"""Several beams over one multi-antenna recording: the element streams side by side, and a beam made from what they show.

    python examples/array_beams.py rfsignal.ini --prn 7 [--ms 8]

`rfsignal.ini` holds the [RFSIGNAL] section of a K-element recording (`array_lanes`, INTEGRATION.md "Multi-antenna recordings"),
at least 2 * ms milliseconds long.  What runs, every beam fed by ONE push per millisecond (`ChannelManager.addBeam`,
sdr_ddc_beam_attach):
  1. beam 0, the manager's own stream, with power-inversion weights trained on the recording's first milliseconds;
  2. beams 1 .. K, the K element streams (`signal.array.element_weights`), and beam K + 1, for now element 0 once more;
  3. the first `ms` milliseconds go in; the search on beam 0 gives the satellite's carrier and code phase, and `epl_batch` at those
     parameters on the K element engines gives the per-element prompts -- the spatial signature of the signal, measured behind
     the correlator, where the signal stands above the noise and the jammer does not;
  4. `signal.array.wiener_weights(R, p)` from the elements' covariance R and those prompts p;
  5. `setBeamWeights(K + 1, w)`: from the next slab on beam K + 1 looks where the signal comes from;
  6. the next `ms` milliseconds go in, and the search on beam K + 1 is printed beside the one on beam 0 and on one element."""
import argparse
import configparser
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sydr_amd.channel.manager import ChannelManager                # noqa: E402
from sydr_amd.engine import make_items                             # noqa: E402
from sydr_amd.signal import array as ar                            # noqa: E402
from sydr_amd.signal.iqsource import RFSignal                      # noqa: E402

CODE_RATE, CODE_CHIPS = 1.023e6, 1023


def search(manager, slot, start, fs):
    """One millisecond of the manager's ring from `start` on -> (Doppler bin, code sample, ratio of the two peaks)."""
    manager._flush_pending()
    pb, pc, pr, _ = manager.engine.pcps([slot], start, fs, 0.0, 5000.0, 250.0, 1, 1)
    return int(pb[0]), int(pc[0]), float(pr[0])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config", help="an ini file with the [RFSIGNAL] section of a multi-antenna recording")
    ap.add_argument("--prn", type=int, required=True)
    ap.add_argument("--ms", type=int, default=8, help="milliseconds per half (measure, then look)")
    args = ap.parse_args(argv)
    ini = configparser.ConfigParser()
    ini.read(args.config)
    conf = dict(ini["RFSIGNAL"])
    conf.setdefault("array_mode", "power_inversion")
    sig = RFSignal(conf)
    K, fs = sig.frontEnd.config.array.n_elements, sig.samplingFrequency
    per_ms = int(fs * 1e-3)

    leader = ChannelManager(sig)                                                      # 1. (trains beam 0's weights)
    print("beam 0, power inversion:", np.round(leader.arrayWeights, 3))
    elements = [leader.addBeam(w) for w in ar.element_weights(K)]                     # 2.
    fifth = leader.addBeam(ar.unit_weights(K, 0))
    managers = [leader] + elements + [fifth]
    try:
        for m in managers:
            m.engine.code_slots(1)
            m.engine.load_gps_code(0, args.prn)
        for _ in range(args.ms):                                                      # 3. one push per millisecond feeds all K + 2 rings
            leader.addNewRFData(sig.getMilliseconds(1))
        bin0, sample0, ratio0 = search(leader, 0, 0, fs)
        doppler = -5000.0 + 250.0 * bin0
        print(f"beam 0: bin {bin0} ({doppler:+.0f} Hz), code sample {sample0}, ratio {ratio0:.2f}")
        step = CODE_RATE / fs
        n = int(np.ceil(CODE_CHIPS / step))
        starts = sample0 + 1 + np.arange(args.ms - 2) * per_ms
        items = make_items(0, n, starts, doppler, 0.0, 0.0, step)
        prompts = []
        for m in [leader] + elements:
            m._flush_pending()
            out = m.engine.epl_batch(items, (0.0,), fs)
            prompts.append(out[:, 0] + 1j * out[:, 1])
        prompts = np.array(prompts)
        # every epoch's carrier phase and data bit are beam 0's own prompt's: taken out before the epochs are added
        p = np.sum(prompts[1:] * np.conj(prompts[0] / np.abs(prompts[0])), axis=1)
        print("per-element prompts:", np.round(p / np.abs(p).max(), 3))
        R, count = leader.arrayCovariance()
        w = ar.wiener_weights(R / count, p)                                           # 4.
        w = w * np.sqrt(np.real(np.vdot(leader.arrayWeights, R @ leader.arrayWeights)) / np.real(np.vdot(w, R @ w)))
        print(f"beam {K + 1}, Wiener:", np.round(w, 3))
        leader.setBeamWeights(K + 1, w)                                               # 5.
        for _ in range(args.ms):                                                      # 6.
            leader.addNewRFData(sig.getMilliseconds(1))
        at = args.ms * per_ms
        for name, m in (("beam 0 (power inversion)", leader), ("beam 1 (element 0)", elements[0]), (f"beam {K + 1} (Wiener)", fifth)):
            b, s, r = search(m, 0, at, fs)
            print(f"{name}: bin {b}, code sample {s}, ratio {r:.2f}")
    finally:
        leader.close()


if __name__ == "__main__":
    sys.exit(main())
