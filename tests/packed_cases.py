"""Shared by tests/test_packing.py (oracle-backed engine, no GPU) and tests/test_gpu_packed.py (the device): one few-level
stream written twice -- packed, and as int8 of the same levels -- and a receiver driven over either file three ways."""
import configparser
import os

import numpy as np

from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
from sydr_amd.channel.manager import ChannelManager
from sydr_amd.signal import packing as pk
from sydr_amd.signal.iqsource import RFSignal
from sydr_amd.utils.enumerations import ChannelMessage

_EXAMPLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
KAPLAN_INI = open(os.path.join(_EXAMPLES, "channel_GPS_L1CA_kaplan.ini")).read()


def kaplan_config(noncoh=None):
    cfg = configparser.ConfigParser()
    cfg.read_string(KAPLAN_INI)
    if noncoh is not None:
        cfg["ACQUISITION"]["non_coherent_integration"] = str(noncoh)
    return cfg


def per_field_unpack(packed, bits, levels, msb_first):
    """The format's statement, field by field in plain Python (the independent check of packing.unpack)."""
    fields = 8 // bits
    out = []
    for j in range(len(packed) * fields):
        p = j % fields
        shift = bits * (fields - 1 - p) if msb_first else bits * p
        out.append(int(levels[(int(packed[j // fields]) >> shift) & ((1 << bits) - 1)]))
    return np.array(out, dtype=np.int8)


def write_both(tmp_path, raw_int8, bits, threshold, levels=None, msb_first=False, stem="iq"):
    """Quantise `raw_int8` (interleaved) to the packing's levels; write it packed and as int8 of those levels.
    -> (packed path, int8 path, packing, the few-level int8 samples)"""
    packing = pk.Packing(bits, levels, msb_first)
    few = pk.quantise(raw_int8, bits, threshold, packing)
    packed_path, plain_path = tmp_path / f"{stem}_{bits}bit.bin", tmp_path / f"{stem}_{bits}bit_as_int8.bin"
    pk.pack(few, packing).tofile(packed_path)
    few.tofile(plain_path)
    return packed_path, plain_path, packing, few


def signal(path, fs, data_size, packing=None):
    conf = dict(filepath=str(path), sampling_frequency=fs, is_complex="true", intermediate_frequency=0.0, data_size=data_size)
    if packing is not None:
        conf["sample_levels"] = ",".join(str(int(v)) for v in packing.levels)
        conf["bit_order"] = "msb" if packing.msb_first else "lsb"
    return RFSignal(conf)


def plain(p):
    """A packet as comparable plain data (arrays -> bytes)."""
    return {k: (v.tobytes(), v.shape) if isinstance(v, np.ndarray) else v for k, v in dict(p).items()}


def receive(sig, engine, prns, cfg, ms, mode, late=None, ring_ms=100, keep_map=True):
    """Drive a ChannelManager over `sig` for `ms` milliseconds.  mode: "ticks" (the reference's loop), "readahead" (the same
    loop with enableReadAhead(16)), "block" (ticks for the first 100 ms, then the rest resident and runBlock).  late:
    (tick, [prns]) -- satellites requested while the others run.  -> (ticks' packets as plain data, the manager)"""
    mgr = ChannelManager(sig, engine=engine, keepCorrelationMap=keep_map, ring_ms=ring_ms)
    mgr.addChannel(ChannelL1CA_Kaplan, cfg, len(prns) + (len(late[1]) if late else 0))
    for prn in prns:
        mgr.requestTracking(prn)
    if mode == "readahead":
        mgr.enableReadAhead(16)
    out = []
    tick_ms = ms if mode != "block" else 100
    for k in range(tick_ms):
        if late and k == late[0]:
            for prn in late[1]:
                mgr.requestTracking(prn)
        mgr.addNewRFData(sig.getMilliseconds(1))
        out.append([plain(p) for p in mgr.run()])
    if mode == "block":
        mgr.addNewRFData(sig.getMilliseconds(ms - tick_ms))
        out.append([plain(p) for p in mgr.runBlock(ms - tick_ms - 10)])
    return out, mgr


def epoch_items(fs, n_ch, total, rng):
    """E/P/L items of n_ch channels over `total` samples, epoch after epoch along each channel's own code rate (the list of
    tests/test_gpu_hostfed.py's first test).  -> (items, epochs)"""
    from sydr_amd.engine import make_items
    step = 1.023e6 * (1.0 + rng.uniform(-3e-6, 3e-6, n_ch)) / fs
    start = rng.integers(0, 2000, n_ch).astype(np.int64)
    rem = rng.uniform(0, 0.03, n_ch)
    rows = []
    while True:
        n = np.ceil((1023.0 - rem) / step).astype(np.int64)
        if (start + n).max() > total:
            break
        rows.append((n.copy(), start.copy(), rem.copy()))
        rem = rem + n * step - 1023.0
        start = start + n
    e = len(rows)
    items = make_items(np.tile(np.arange(n_ch), e), np.stack([r[0] for r in rows]).reshape(-1), np.stack([r[1] for r in rows]).reshape(-1),
                       np.tile(rng.uniform(-4000, 4000, n_ch), e), np.tile(rng.uniform(0, 6.28, n_ch), e),
                       np.stack([r[2] for r in rows]).reshape(-1), np.tile(step, e))
    return items, e


def count(ticks, kind=ChannelMessage.TRACKING_UPDATE):
    return sum(1 for t in ticks for p in t if p["type"] is kind)
