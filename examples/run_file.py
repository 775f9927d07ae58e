#!/usr/bin/env python3
"""Track an IQ recording with the reference's own configuration files.

    python examples/run_file.py receiver.ini [--ms 2000] [--block 80 | --read-ahead 50] [--csv out.csv]
                                              [--profile N_TAPS] [--probe] [--search-behind PRN,PRN,...]

`receiver.ini` is the reference's receiver configuration (config/receiver.ini: [DEFAULT] nb_channels /
ms_to_process, [RFSIGNAL], [SATELLITES] include_prn, [CHANNELS] gps_l1ca = <channel ini>).  What the reference's
Receiver does around the hot path for the first stage of processing -- read the file millisecond by millisecond, give
each requested PRN a channel, acquire, track -- is done here with the drop-in ChannelManager; once every channel
tracks, blocks of `--block` ms go through the closed-loop kernel (`ChannelManager.runBlock`); with `--read-ahead N`
the loop stays the reference's own (one millisecond per iteration: `addNewRFData(getMilliseconds(1)); run()`) and the
manager tracks N ms ahead behind it (`enableReadAhead`).  Subframes the channels decode are printed as they complete
(DECODING_UPDATE; needs a decoder: by default the reference's own, where `sydr` is importable).  Navigation,
measurements, database and report stay the reference's business (feed them the packets this script prints / writes).
`--probe` looks at the front end first: the first second of the recording goes into a ring of its own length and
`Engine.iq_probe` says what it holds -- levels, rails, DC offset, I/Q imbalance, the histogram's occupied bins, the noise
floor and the bins that stand out of the spectrum -- before any channel is started.
`--search-behind 4,9,30` ends with a search for those PRNs BEHIND the tracked ones: 20 more milliseconds go through
`ChannelManager.searchBehindTracked`, which tracks them as a block, subtracts every tracked signal's replica from those
samples into a second engine (`sdr_iq_cancel`) and searches the residue over 10 non-coherent milliseconds -- a PRN 24 dB or
more under a tracked one shows there and not in a search of the samples as they came."""
import argparse
import configparser
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sydr_amd.channel.l1ca_borre import ChannelL1CA                # noqa: E402
from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan        # noqa: E402
from sydr_amd.channel.manager import ChannelManager                # noqa: E402
from sydr_amd.signal.iqsource import RFSignal                      # noqa: E402
from sydr_amd.utils.enumerations import ChannelMessage, ChannelState  # noqa: E402


def print_probe(rf):
    """The first second of the recording (or all of it, when it is shorter), probed on the device."""
    from sydr_amd.engine import FMT_CI16, FMT_CI8
    from sydr_amd.runtime import get_engine
    engine = get_engine()
    n = min(rf.totalSamples, int(rf.samplingFrequency)) // 8 * 8
    fmt = FMT_CI16 if rf.fileDataType is np.int16 else FMT_CI8
    engine.iq_alloc(n, fmt)
    if rf.packing is not None:
        engine.iq_upload_packed(rf.samples(0, n), n, rf.packing, 0)
    else:
        engine.iq_upload(rf.samples(0, n), 0)
    nfft = 1024 if n >= 1024 else 0
    r = engine.iq_probe(0, n, nfft=nfft, fs=rf.samplingFrequency if nfft else None)
    print(f"probe of the first {n} samples ({n / rf.samplingFrequency * 1e3:.0f} ms):")
    for c, name in enumerate("IQ"):
        used = np.flatnonzero(r.hist[c])
        print(f"  {name}: min {r.min[c]:.0f} max {r.max[c]:.0f} mean {r.mean[c]:+.3f} rms {r.rms[c]:.3f} (DC / rms {r.dc_offset[c]:+.4f}), "
              f"on the rails {100.0 * r.rail_fraction[c]:.3f} %, {used.size} histogram bins in use ({used[0] - 128} .. {used[-1] - 128})")
    print(f"  I/Q gain imbalance {r.iq_imbalance_db:+.3f} dB, I/Q correlation {r.iq_correlation:+.4f}")
    if nfft:
        db = r.psd_db
        print(f"  spectrum ({r.n_segments} segments of {nfft}): median {np.median(db):.2f} dB/Hz, peak {db.max():.2f} dB/Hz")
        for f, over in r.spurs(10.0)[:8]:
            print(f"    {f / 1e3:+10.1f} kHz stands {over:.1f} dB above the median bin")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("receiver_ini")
    ap.add_argument("--ms", type=int, default=None, help="milliseconds to process (default: ms_to_process)")
    ap.add_argument("--block", type=int, default=80, help="epochs per closed-loop block once all channels track (0: per-tick only)")
    ap.add_argument("--read-ahead", type=int, default=0, help="keep the per-millisecond loop and let the manager track this many ms ahead (overrides --block)")
    ap.add_argument("--csv", default=None, help="write one line per tracking epoch")
    ap.add_argument("--profile", type=int, default=0, metavar="N_TAPS",
                    help="print |correlation function| of every channel's last epoch at the end: N_TAPS taps across +-2 chips")
    ap.add_argument("--search-behind", default="", metavar="PRNS",
                    help="at the end: search these PRNs (comma separated) in 20 ms with the tracked signals cancelled")
    ap.add_argument("--probe", action="store_true", help="print what the first second of the recording holds (Engine.iq_probe) before tracking")
    args = ap.parse_args(argv)

    rcfg = configparser.ConfigParser()
    rcfg.read(args.receiver_ini)
    base = os.path.dirname(os.path.abspath(args.receiver_ini))
    chan_ini = rcfg["CHANNELS"]["gps_l1ca"]
    chan_ini = chan_ini if os.path.isabs(chan_ini) else os.path.normpath(os.path.join(base, chan_ini))
    ccfg = configparser.ConfigParser()
    ccfg.read(chan_ini)
    plugin = ChannelL1CA_Kaplan if "correlator_epl_wide" in ccfg["TRACKING"] else ChannelL1CA
    rf = RFSignal(rcfg["RFSIGNAL"])
    prns = [int(p) for p in rcfg["SATELLITES"]["include_prn"].split(",") if p.strip()]
    ms_total = args.ms or int(rcfg["DEFAULT"]["ms_to_process"])

    if args.probe:
        print_probe(rf)
    mgr = ChannelManager(rf, keepCorrelationMap=False)
    plan = getattr(rf.frontEnd, "array", None) if rf.frontEnd is not None else None
    if plan is not None:              # a multi-antenna recording ([RFSIGNAL] array_lanes): the weights its elements are combined with
        w = getattr(mgr, "arrayWeights", rf.frontEnd.config.array.weights)
        print(f"array of {len(w)} elements, {plan.mode}" + (f" over the first {plan.train_ms} ms" if plan.adaptive else "") + ": weights "
              + ", ".join(f"{v.real:+.4f}{v.imag:+.4f}j" for v in w))
    mgr.addChannel(plugin, ccfg, max(len(prns), int(rcfg["DEFAULT"].get("nb_channels", len(prns)))))
    for p in prns:
        mgr.requestTracking(p)
    if args.read_ahead:
        mgr.enableReadAhead(args.read_ahead)
        args.block = 0
    out = open(args.csv, "w") if args.csv else None
    if out:
        out.write("ms,cid,i_prompt,q_prompt,carrier_frequency,code_frequency,cn0,lock_state\n")
    ring_ms = mgr.sharedBuffer.maxSize // rf.samplesPerMs
    t0, ms, n_track = time.perf_counter(), 0, 0

    def emit(packets, ms_now):
        nonlocal n_track
        for p in packets:
            if p["type"] is ChannelMessage.ACQUISITION_UPDATE:
                print(f"[{ms_now:6d} ms] channel {p['cid']}: acquisition bin {p['frequency_idx']} code {p['code_idx']} "
                      f"ratio {p['peak_ratio']:.2f} carrier {p['carrierFrequency']:+.1f} Hz")
            elif p["type"] is ChannelMessage.DECODING_UPDATE:
                print(f"[{ms_now:6d} ms] channel {p['cid']}: subframe {p['subframe_id']} decoded, TOW {p['tow']}")
            elif p["type"] is ChannelMessage.TRACKING_UPDATE:
                n_track += 1
                if out:
                    out.write(f"{ms_now},{p['cid']},{p['i_prompt']:.3f},{p['q_prompt']:.3f},{p['carrier_frequency']:.4f},"
                              f"{p['code_frequency']:.4f},{p['cn0']:.3f},{int(p['lock_state'])}\n")

    while ms < ms_total:
        all_tracking = all(ch.channelState is ChannelState.TRACKING for ch in mgr.channels.values()
                           if ch.channelState is not ChannelState.IDLE)
        if args.block and all_tracking and ms + args.block <= ms_total and args.block < ring_ms - 2:
            for _ in range(args.block):                       # fill the ring ahead of the channels, then one launch
                mgr.addNewRFData(rf.getMilliseconds(1))
            emit(mgr.runBlock(args.block), ms + args.block)            # (as many whole epochs as the ring holds)
            ms += args.block
        else:
            mgr.addNewRFData(rf.getMilliseconds(1))
            emit(mgr.run(), ms + 1)
            ms += 1
    dt = time.perf_counter() - t0
    behind = [int(p) for p in args.search_behind.split(",") if p.strip()]
    if behind and 20 < ring_ms - 2:
        for _ in range(20):
            mgr.addNewRFData(rf.getMilliseconds(1))
        packets, rows = mgr.searchBehindTracked(behind, 20, dict(doppler_range=5000.0, doppler_step=250.0, coh=1, noncoh=10))
        emit(packets, ms + 20)
        ms += 20
        for r in rows:
            print(f"behind the tracked signals: G{r['satelliteID']:02d} bin {r['peak_bin']} ({r['doppler_hz']:+.0f} Hz) code {r['peak_code']} "
                  f"ratio {r['peak_ratio']:.2f} from sample {r['start_sample']}")
    for ch in mgr.channels.values():
        if ch.channelState is not ChannelState.IDLE:
            bits = "".join(str(int(b)) for b in getattr(ch, "navBits", [])[:40])
            print(f"channel {ch.channelID} G{ch.satelliteID:02d}: state {ch.channelState.name}, carrier {ch.carrierFrequency:+.2f} Hz, bits {bits}")
    if args.profile > 0:
        step = 4.0 / (args.profile - 1) if args.profile > 1 else 0.0
        for cid, prof in mgr.correlationProfiles(-2.0 if args.profile > 1 else 0.0, step, args.profile).items():
            mag = np.hypot(prof[:, 0], prof[:, 1])
            print(f"channel {cid} correlation profile, {args.profile} taps from {-2.0 if args.profile > 1 else 0.0:+.3f} chips "
                  f"in steps of {step:.4f}: peak {mag.max():.1f} at tap {int(mag.argmax())}")
            print("  " + " ".join(f"{v / max(mag.max(), 1e-300):.3f}" for v in mag))
    print(f"{ms} ms of signal, {n_track} tracking epochs in {dt:.2f} s = {ms * 1e-3 / dt:.2f}x real time")
    if out:
        out.close()


if __name__ == "__main__":
    main()
