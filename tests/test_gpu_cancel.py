"""sdr_iq_cancel on the MI355X against its NumPy statement (sydr_amd/signal/cancel.py through tests/cancel_cases.py; the CPU
file tests/test_cancel.py holds the statement against the oracle): integer rings byte for byte -- every case's statement
keeps more than the derived bound from a rounding tie and from a rail, asserted first --, float rings within the derived
bound (cancel.parity_bound, docs/notes/cancel.md), the counters equal, the rest of either ring untouched."""
import ctypes as C

import numpy as np
import pytest

import cancel_cases as cc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI8, Engine, make_items
from sydr_amd.signal import cancel as cn
from test_gpu_tracking import initial_state, loop_cfg
from test_oracle_golden import BORRE_CFG

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6


def _stage(engine, image, fmt, slots):
    engine.iq_alloc(len(image) // 2, fmt)
    engine.iq_upload(image, 0)
    cc.stage_codes(engine, slots)


def _setup(engine, name, fmt, scale=1.0):
    c = cc.geometry(name)
    res, image = cc.statement(name, fmt, scale)
    _stage(engine, image, fmt, c["slots"])
    return c, res, image, cc.amps_of(name, fmt, scale)


def _expected_ring(image, res, w0):
    """The ring after the call: the image with the statement's window in it."""
    ring = cc.to_complex(image)
    ring[(w0 + np.arange(len(res.window))) % len(ring)] = res.window
    return ring


def _hold(tag, got_image, want_ring, fmt, d, inside):
    """A downloaded ring against the expected one: integer rings equal, float rings within d inside the window and equal
    outside it.  -> the worst observed fraction of d."""
    got = cc.to_complex(got_image)
    err = np.maximum(np.abs(got.real - want_ring.real), np.abs(got.imag - want_ring.imag))
    assert np.array_equal(got[~inside], want_ring[~inside], equal_nan=True), f"{tag}: samples outside the window changed"
    worst = float(err[inside].max()) / d
    print(f"{tag}: worst distance {err[inside].max():.3e} = {worst:.3f} of the bound {d:.3e}")
    if fmt in cc.RAIL:
        assert np.array_equal(got, want_ring), f"{tag}: {np.count_nonzero(got != want_ring)} samples differ"
    else:
        assert worst <= 1.0
    return worst


def _inside(cap, w0, W):
    m = np.zeros(cap, dtype=bool)
    m[(w0 + np.arange(W)) % cap] = True
    return m


def _margins(name, fmt, scale=1.0):
    tie, rail = cc.tie_and_rail_margins(name, fmt, scale)
    d = cc.bound(name, fmt, scale)
    print(f"{name} {cc.FMT_NAMES[fmt]}: tie margin {tie:.3e}, rail margin {rail:.3e}, bound {d:.3e}")
    assert tie > d and rail > d


@pytest.mark.parametrize("fmt", cc.FMTS, ids=[cc.FMT_NAMES[f] for f in cc.FMTS])
@pytest.mark.parametrize("name", cc.CASES)
def test_parity_with_the_statement(engine, name, fmt):
    if fmt in cc.RAIL:
        _margins(name, fmt)
    c, res, image, amps = _setup(engine, name, fmt)
    stats = engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"]))
    assert stats == res.stats
    _hold(f"{name} {cc.FMT_NAMES[fmt]}", engine.iq_download(c["capacity"], 0), _expected_ring(image, res, c["w0"]), fmt,
          cc.bound(name, fmt), _inside(c["capacity"], c["w0"], c["W"]))


@pytest.mark.parametrize("fmt", [FMT_CI8, FMT_CF32], ids=["ci8", "cf32"])
@pytest.mark.parametrize("name,dst_offset", [("short", 8192 - 999), ("short", 8192 - 1003), ("stagger", 24576 - 8)])
def test_another_engine_gets_what_in_place_gives(engine, name, fmt, dst_offset):
    """dst = a second engine on the device: the same bytes as in place, the source ring unchanged, the destination's other
    samples -- canaries on both sides of a window that crosses its ring's end -- untouched.  dst_offset - w0 a multiple of
    the granule (whole 16-byte stores) and not (sample by sample)."""
    c, res, image, amps = _setup(engine, name, fmt)
    dcap = 8192 if name == "short" else 24576
    canary = cc.noise_image(dcap, fmt, 7)
    other = Engine(0)
    try:
        other.iq_alloc(dcap, fmt)
        other.iq_upload(canary, 0)
        stats = engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"]), dst=other, dst_offset=dst_offset)
        assert stats == res.stats
        assert engine.iq_download(c["capacity"], 0).tobytes() == image.tobytes()          # the source is as it was
        there = other.iq_download(dcap, 0)
        assert engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"])) == res.stats
        here = cc.to_complex(engine.iq_download(c["capacity"], 0))
    finally:
        other.close()
    inside = _inside(dcap, dst_offset, c["W"])
    assert dst_offset + c["W"] > dcap
    got = cc.to_complex(there)
    assert np.array_equal(got[~inside], cc.to_complex(canary)[~inside])
    assert np.array_equal(got[(dst_offset + np.arange(c["W"])) % dcap], cc.window_of(here, c["w0"], c["W"]))


def test_a_disjoint_window_of_the_same_ring(engine):
    """dst = the engine itself: a window that shares no sample with the source's takes the result and the source stays; one
    that overlaps it is refused."""
    c = cc.geometry("short")
    res, image = cc.statement("short", FMT_CI8)
    amps = cc.amps_of("short", FMT_CI8)
    big = np.concatenate([image, cc.noise_image(8192 - c["capacity"], FMT_CI8, 11)])      # (no item wraps: the offsets stay)
    _stage(engine, big, FMT_CI8, c["slots"])
    win, there = (c["w0"], c["W"]), 5000
    with pytest.raises(_lib.SdrError) as err:
        engine.iq_cancel(c["items"], amps, c["fs"], window=win, dst=engine, dst_offset=c["w0"] + c["W"] - 1)
    assert err.value.status == INVALID
    assert engine.iq_download(8192, 0).tobytes() == big.tobytes()
    assert engine.iq_cancel(c["items"], amps, c["fs"], window=win, dst=engine, dst_offset=there) == res.stats
    want = cc.to_complex(big)
    want[there:there + c["W"]] = res.window
    assert np.array_equal(cc.to_complex(engine.iq_download(8192, 0)), want)


@pytest.mark.parametrize("fmt", [FMT_CI8, FMT_CF64], ids=["ci8", "cf64"])
def test_identical_calls_identical_bits_and_the_channel_order_is_the_statements(engine, fmt):
    c, res, image, amps = _setup(engine, "many", fmt)
    outs = []
    for _ in range(2):
        engine.iq_upload(image, 0)
        engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"]))
        outs.append(engine.iq_download(c["capacity"], 0).tobytes())
    assert outs[0] == outs[1]
    # the channels in another order against the statement fed that order
    order = np.random.default_rng(5).permutation(len(c["items"]))
    win = cc.window_of(cc.to_complex(image), c["w0"], c["W"])
    want = cn.cancel_statement(win, fmt, cc.channels_of("many", amps, order), c["fs"], c["w0"], c["capacity"])
    d = cc.bound("many", fmt)
    if fmt in cc.RAIL:
        v = np.concatenate([want.pre.real[want.covered], want.pre.imag[want.covered]])
        assert np.abs(np.abs(v - np.floor(v)) - 0.5).min() > d
    engine.iq_upload(image, 0)
    assert engine.iq_cancel(c["items"][order], amps[order], c["fs"], window=(c["w0"], c["W"])) == want.stats
    _hold("many, permuted", engine.iq_download(c["capacity"], 0), _expected_ring(image, want, c["w0"]), fmt, d,
          _inside(c["capacity"], c["w0"], c["W"]))
    if fmt == FMT_CF64:     # (the order shows: the permuted sums round differently somewhere)
        assert not np.array_equal(want.window, res.window)


def test_rails(engine):
    """ci8 with amplitudes four times the budget: components beyond +-127 are clipped and counted as the statement does."""
    _margins("stagger", FMT_CI8, cc.RAIL_SCALE)
    c, res, image, amps = _setup(engine, "stagger", FMT_CI8, cc.RAIL_SCALE)
    assert res.stats["clipped_components"] > 0
    assert engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"])) == res.stats
    _hold("rails", engine.iq_download(c["capacity"], 0), _expected_ring(image, res, c["w0"]), FMT_CI8, cc.bound("stagger", FMT_CI8, cc.RAIL_SCALE),
          _inside(c["capacity"], c["w0"], c["W"]))


def test_one_nan_stays_one_nan(engine):
    c, res, image, amps = _setup(engine, "short", FMT_CF64)
    at = (c["w0"] + 777) % c["capacity"]
    poisoned = image.copy()
    poisoned[2 * at] = np.nan
    engine.iq_upload(poisoned, 0)
    engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"]))
    got = cc.to_complex(engine.iq_download(c["capacity"], 0))
    bad = ~(np.isfinite(got.real) & np.isfinite(got.imag))
    assert np.flatnonzero(bad).tolist() == [at]
    want = _expected_ring(image, res, c["w0"])
    keep = ~bad
    assert np.abs(got[keep].real - want[keep].real).max() <= cc.bound("short", FMT_CF64)
    assert np.abs(got[at].imag - want[at].imag) <= cc.bound("short", FMT_CF64)


@pytest.mark.parametrize("fmt", [FMT_CF64, FMT_CI8], ids=["cf64", "ci8"])
def test_prompts_vanish_on_the_device(engine, fmt):
    """iq_cancel(items, amps=None) takes each epoch's prompt over n as amplitude; epl_batch of the same items on the output
    is then zero to the CPU identity test's bounds: the derived bound times n (cf64), n * sqrt(2) / 2 (an integer ring
    with no rail hit).  One channel: with more, another channel's replica leaks into the prompt."""
    nf = cc.near_far(fmt)
    fs = cc.NEAR_FAR["fs"]
    _stage(engine, nf["image"], fmt, nf["slots"])
    items = nf["items"]
    stats = engine.iq_cancel(items, None, fs)
    assert stats["samples_changed"] == 40000 and stats["clipped_components"] == 0
    prompts = engine.epl_batch(items[0], [0.0], fs)
    n = items[0]["n_samples"].astype(np.float64)
    if fmt == FMT_CF64:
        amp = float(np.abs(nf["amps_truth"]).sum(axis=-1).max())
        theta_max = float((np.abs(items["carrier_hz"]) * 2 * np.pi * n / fs + np.abs(items["rem_carrier"])).max())
        limit = cn.parity_bound(fmt, amp, theta_max, float(np.abs(cc.to_complex(nf["image"])).max()) + amp, 1) * n
    else:
        limit = n * np.sqrt(2.0) / 2.0
    worst = np.hypot(prompts[:, 0], prompts[:, 1]) / limit
    print(f"{cc.FMT_NAMES[fmt]}: prompts after cancellation at most {worst.max():.3f} of the limit")
    assert np.all(worst <= 1.0)


@pytest.mark.parametrize("fmt", [FMT_CF64, FMT_CI8], ids=["cf64", "ci8"])
def test_near_far(engine, fmt):
    """A 30 times B: sdr_pcps for B on the original ring returns a cross-correlation peak of A, on the cancelled ring B's
    (bin, code phase); the absent C's ratio drops.  The indices are the oracle's (tests/test_cancel.py asserts them there)."""
    c, nf, exp = cc.NEAR_FAR, cc.near_far(fmt), cc.near_far_expected(fmt)
    _stage(engine, nf["image"], fmt, nf["slots"])

    def search():
        pb, pc, pr, _ = engine.pcps([1, 2], 0, c["fs"], 0.0, c["R"], c["S"], c["coh"], c["noncoh"])
        return [int(pb[0]), int(pc[0])], float(pr[0]), [int(pb[1]), int(pc[1])], float(pr[1])

    b0, rb0, c0, rc0 = search()
    engine.iq_cancel(nf["items"], None, c["fs"])
    b1, rb1, c1, rc1 = search()
    print(f"{cc.FMT_NAMES[fmt]}: B before {b0} ratio {rb0:.3f}, after {b1} ratio {rb1:.3f}; C before {rc0:.3f}, after {rc1:.3f}")
    assert b0 == exp["before_b"][0] and b0 != list(nf["truth"])
    assert b1 == exp["after_b"][0] == list(nf["truth"])
    assert rb1 == pytest.approx(exp["after_b"][1], rel=1e-6)
    assert rc1 < rc0 and rc1 == pytest.approx(exp["after_c"][1], rel=1e-6)


def test_through_tracking(engine):
    """track_closed_loop on A for 20 epochs with B 28 dB under it: items_from_records of its trajectory, cancel; the device's
    output is the statement's fed the same records, and B is found where the truth puts it -- which it is not before."""
    fs, prn_a, prn_b = 4e6, 9, 23
    n = 26 * 4000
    sat_a = dict(prn=prn_a, doppler=2250.0, code_phase=417.3, phase=0.2, amp=75.0)
    sat_b = dict(prn=prn_b, doppler=-1250.0, code_phase=100.6, phase=0.7, amp=3.0)
    raw = orc.synth_iq(fs, n, [sat_a, sat_b], 1.0, 20260505)
    _stage(engine, raw, FMT_CI8, [("gps", prn_a), ("gps", prn_b)])
    pb, pc, _, _ = engine.pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)
    n0 = orc.required_samples(0.0, orc.CODE_RATE / fs)
    carrier, _, cur = orc.post_acquisition(0.0, 5000.0, 250.0, [int(pb[0]), int(pc[0])], 0, 4000, n0)
    _, traj = engine.track_closed_loop([initial_state(0, fs, carrier, cur, BORRE_CFG)], loop_cfg(0, fs, BORRE_CFG), 20)
    items, amps, (w0, W) = cn.items_from_records(traj, [0])
    assert w0 == int(traj[0]["start_sample"][0]) and W == int(traj[0]["n_samples"].sum())

    def search():
        b, k, r, _ = engine.pcps([1], w0, fs, 0.0, 5000.0, 250.0, 1, 5)
        return [int(b[0]), int(k[0])], float(r[0])

    before = search()
    x = orc.iq_to_complex(raw).astype(np.complex128)
    want = cn.cancel_statement(x[w0:w0 + W], FMT_CI8, [(items[0], amps[0], orc.gold_code(prn_a))], fs, w0, n)
    v = np.concatenate([want.pre.real, want.pre.imag])
    assert np.abs(np.abs(v - np.floor(v)) - 0.5).min() > 1e-9
    assert engine.iq_cancel(items, amps, fs) == want.stats
    got = cc.to_complex(engine.iq_download(n, 0))
    assert np.array_equal(got[w0:w0 + W], want.window) and np.array_equal(got[:w0], x[:w0]) and np.array_equal(got[w0 + W:], x[w0 + W:])
    after = search()
    step_b = orc.CODE_RATE * (1 + sat_b["doppler"] / cc.L1) / fs
    left = (-(sat_b["code_phase"] + w0 * step_b)) % 1023                      # chips until B's next code start, at w0
    truth = [int(round((-sat_b["doppler"] + 5000.0) / 250.0)), int(np.ceil(left * fs / orc.CODE_RATE))]
    print(f"B before {before}, after {after}, truth {truth}")
    assert before[0] != truth and after[0] == truth


def _raises(status, call):
    with pytest.raises(_lib.SdrError) as err:
        call()
    assert err.value.status == status, str(err.value)


def test_errors_leave_the_engine_and_the_rings_as_they_were(engine):
    c, res, image, amps = _setup(engine, "short", FMT_CI8)
    fs, win, items = c["fs"], (c["w0"], c["W"]), c["items"]
    lib, h = engine._lib, engine._h
    st = _lib.CancelStats()
    flat, a = np.ascontiguousarray(items), np.ascontiguousarray(amps)
    n_ch, n_ep = items.shape

    def raw(items_p=_lib.ptr(flat), amps_p=_lib.ptr(a), ch=n_ch, ep=n_ep, rate=fs, w0=win[0], W=win[1], dst=None, off=win[0]):
        return lib.sdr_iq_cancel(h, items_p, amps_p, ch, ep, rate, w0, W, dst, off, C.byref(st))

    assert raw(items_p=None) == INVALID and raw(amps_p=None) == INVALID
    assert raw(ch=0) == INVALID and raw(ch=65) == INVALID and raw(ep=0) == INVALID
    assert raw(rate=0.0) == INVALID and raw(rate=-1.0) == INVALID and raw(rate=float("nan")) == INVALID
    assert raw(w0=-1) == RANGE and raw(off=-1, dst=h) == RANGE
    assert raw(W=c["capacity"] + 8) == RANGE
    assert lib.sdr_iq_cancel(None, _lib.ptr(flat), _lib.ptr(a), n_ch, n_ep, fs, win[0], win[1], None, 0, None) == INVALID

    def edited(field, value, ch=1, k=2):
        its = items.copy()
        its[field][ch, k] = value
        return its

    for bad in (np.nan, np.inf):
        am = amps.copy()
        am[0, 1, 1] = bad
        _raises(INVALID, lambda: engine.iq_cancel(items, am, fs, window=win))
        for field in ("carrier_hz", "rem_carrier", "rem_code", "code_step"):
            _raises(INVALID, lambda: engine.iq_cancel(edited(field, bad), amps, fs, window=win))
    _raises(INVALID, lambda: engine.iq_cancel(edited("code_step", 0.0), amps, fs, window=win))
    _raises(INVALID, lambda: engine.iq_cancel(edited("code_step", -0.5), amps, fs, window=win))
    _raises(INVALID, lambda: engine.iq_cancel(edited("code_slot", 1), amps, fs, window=win))      # allocated, not staged
    _raises(INVALID, lambda: engine.iq_cancel(edited("code_slot", 7), amps, fs, window=win))
    _raises(INVALID, lambda: engine.iq_cancel(edited("code_slot", -1), amps, fs, window=win))
    _raises(INVALID, lambda: engine.iq_cancel(edited("start_sample", items["start_sample"][1, 1] + 61), amps, fs, window=win))   # overlaps
    swapped = items.copy()
    swapped[1, [2, 3]] = swapped[1, [3, 2]]
    _raises(INVALID, lambda: engine.iq_cancel(swapped, amps, fs, window=win))                     # does not ascend
    _raises(RANGE, lambda: engine.iq_cancel(items, amps, fs, window=(win[0], win[1] - 100)))      # an item leaves the window
    _raises(RANGE, lambda: engine.iq_cancel(items, amps, fs, window=(win[0] + 40, win[1])))       # ... in front of it
    _raises(RANGE, lambda: engine.iq_cancel(edited("start_sample", -5), amps, fs, window=win))
    _raises(UNSUPPORTED, lambda: engine.iq_cancel(edited("rem_code", 2e9), amps, fs, window=win))
    _raises(INVALID, lambda: engine.iq_cancel(items, amps, fs, window=win, dst=engine, dst_offset=win[0] + 8))   # overlapping

    other = Engine(0)
    try:
        _raises(STATE, lambda: engine.iq_cancel(items, amps, fs, window=win, dst=other, dst_offset=0))     # dst has no ring
        _raises(STATE, lambda: other.iq_cancel(items, amps, fs, window=win))
        other.iq_alloc(4096, FMT_CI8)
        _raises(STATE, lambda: other.iq_cancel(items, amps, fs, window=win))                              # no code slots
        other.iq_alloc(1024, FMT_CI8)
        _raises(RANGE, lambda: engine.iq_cancel(items, amps, fs, window=win, dst=other, dst_offset=0))     # longer than dst's ring
        other.iq_alloc(4096, FMT_CF32)
        canary = cc.noise_image(4096, FMT_CF32, 2)
        other.iq_upload(canary, 0)
        _raises(INVALID, lambda: engine.iq_cancel(items, amps, fs, window=win, dst=other, dst_offset=0))   # another format
        other.iq_alloc(4096, FMT_CI8)
        canary = cc.noise_image(4096, FMT_CI8, 3)
        other.iq_upload(canary, 0)
        _raises(RANGE, lambda: engine.iq_cancel(items, amps, fs, window=(win[0], win[1] - 100), dst=other, dst_offset=0))
        assert other.iq_download(4096, 0).tobytes() == canary.tobytes()       # a refused call wrote nothing there
    finally:
        other.close()
    # nothing was written here either, and the engine still serves a good call
    assert engine.iq_download(c["capacity"], 0).tobytes() == image.tobytes()
    assert engine.iq_cancel(items, amps, fs, window=win) == res.stats
    _hold("after the errors", engine.iq_download(c["capacity"], 0), _expected_ring(image, res, c["w0"]), FMT_CI8, cc.bound("short", FMT_CI8),
          _inside(c["capacity"], c["w0"], c["W"]))


def test_profiling_scopes(engine):
    c, res, image, amps = _setup(engine, "short", FMT_CI8)
    engine.prof_enable(True)
    try:
        engine.prof_reset()
        engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"]))
        assert engine.prof_read("cancel_kernel")[1] == 1 and engine.prof_read("cancel_items_upload")[1] == 1
        engine.prof_enable(True, calls_only=True)
        engine.prof_reset()
        engine.iq_upload(image, 0)
        engine.iq_cancel(c["items"], amps, c["fs"], window=(c["w0"], c["W"]))
        assert engine.prof_read("call_iq_cancel")[1] == 1 and engine.prof_read("cancel_")[1] == 0
    finally:
        engine.prof_enable(False)


def test_manager_searches_behind_the_tracked_channel_on_the_device(engine):
    """ChannelManager.searchBehindTracked with real engines: PRN 9 tracked at 75 LSB, PRN 23 at 3 LSB beside it (the CPU file
    runs the same scenario against the fake engine): the packets are a twin manager's runBlock packets, PRN 23 comes out at
    the truth in the second engine's ring, the tracked ring is untouched."""
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.utils.enumerations import ChannelState
    from test_host_layer import KAPLAN_INI, channel_config, drive, rf_signal
    sats = [dict(prn=9, doppler=2250.0, code_phase=417.3, phase=0.2, amp=75.0), dict(prn=23, doppler=-1250.0, code_phase=100.6, phase=0.7, amp=3.0)]
    raw = orc.synth_iq(4e6, 41 * 4000, sats, 1.0, 20260606)
    results = []
    for behind in (False, True):
        mgr = ChannelManager(rf_signal(4e6), engine=engine)
        try:
            mgr.addChannel(ChannelL1CA_Kaplan, channel_config(KAPLAN_INI), 2)
            ch = mgr.requestTracking(9)
            drive(mgr, raw, 4000, 16)
            assert ch.channelState is ChannelState.TRACKING
            mgr.addNewRFData(raw[2 * 16 * 4000:])
            if behind:
                packets, rows = mgr.searchBehindTracked([23, 30], 24, dict(doppler_range=5000.0, doppler_step=250.0, coh=1, noncoh=5))
                ring = engine.iq_download(engine.iq_capacity, 0)
                results.append(([dict(p) for p in packets], rows, ring, dict(mgr.lastCancelStats)))
            else:
                results.append(([dict(p) for p in mgr.runBlock(24)], None, engine.iq_download(engine.iq_capacity, 0), None))
        finally:
            mgr.close()
    (twin_packets, _, twin_ring, _), (packets, rows, ring, stats) = results
    assert len(packets) == len(twin_packets) == 25
    for a, b in zip(packets, twin_packets):
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert ring.tobytes() == twin_ring.tobytes()
    w0 = rows[0]["start_sample"]
    step_b = orc.CODE_RATE * (1 + sats[1]["doppler"] / cc.L1) / 4e6
    left = (-(sats[1]["code_phase"] + w0 * step_b)) % 1023
    print(f"rows {rows}, stats {stats}")
    assert (rows[0]["peak_bin"], rows[0]["peak_code"], rows[0]["doppler_hz"]) == (25, int(np.ceil(left * 4e6 / orc.CODE_RATE)), -1250.0)
    assert rows[0]["peak_ratio"] > 1.8 > rows[1]["peak_ratio"]
    assert stats["samples_written"] == stats["samples_changed"] > 24 * 3999
