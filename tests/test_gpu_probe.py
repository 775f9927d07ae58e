"""sdr_iq_probe on the device against its NumPy statement (sydr_amd/signal/probe.py): integer rings exactly (every field, the
histogram), float rings to the bound any order of fp64 additions keeps, the Welch spectrum to the project's 1e-9 of the peak;
windows at odd offsets, across the ring's end, behind queued uploads; refusals; a receiver that is probed while it runs."""
import ctypes as C

import numpy as np
import pytest

import packed_cases
import probe_cases as cases

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI16, FMT_CI8, Engine
from sydr_amd.signal import packing as pk
from sydr_amd.signal import probe as pb

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6
CAP = cases.CAP


def fill(engine, fmt, raw, cap=CAP):
    engine.iq_alloc(cap, fmt)
    engine.iq_upload(raw, 0)


# ------------------------------------------------------------------------------------------------ 1. exactness on integer rings
@pytest.mark.parametrize("fmt", [FMT_CI8, FMT_CI16])
def test_integer_rings_equal_the_statement_exactly(engine, fmt):
    rng = np.random.default_rng(100 + fmt)
    raw = cases.integer_ring(rng, fmt)
    fill(engine, fmt, raw)
    windows = cases.moment_windows(rng)
    assert len(windows) >= 40 and sum((s % CAP) + n > CAP for s, n in windows) >= 12
    for k, (start, n) in enumerate(windows):
        win = cases.window(raw, start, n, CAP)
        for shift in cases.HIST_SHIFTS[fmt]:
            want = pb.probe(win, hist_shift=shift)
            got = engine.iq_probe(start, n, hist=True, hist_shift=shift)
            assert got.raw() == want.raw(), (k, start, n, shift, got, want)        # doubles by ==
            assert np.array_equal(got.hist, want.hist), (k, start, n, shift)
            assert got.hist[0].sum() == n and got.hist[1].sum() == n
        assert engine.iq_probe(start, n, hist=False).raw() == want.raw(), (k, start, n)   # the kernel without a histogram


# ------------------------------------------------------------------------------------------------ 2. overflow
@pytest.mark.parametrize("fmt, low, sum_sq", [(FMT_CI16, -32768, float(1 << 52)), (FMT_CI8, -128, float(1 << 36))])
def test_a_ring_on_the_lower_rail_overflows_nothing(engine, fmt, low, sum_sq):
    cap = 1 << 22
    engine.iq_alloc(cap, fmt)
    engine.iq_upload(np.full(2 * cap, low, dtype=cases.NP_OF_FMT[fmt]), 0)
    for shift in cases.HIST_SHIFTS[fmt]:
        got = engine.iq_probe(3, cap, hist=True, hist_shift=shift)
        assert got.sum_sq == (sum_sq, sum_sq) and got.sum_iq == sum_sq
        assert got.sum == (float(low * cap),) * 2 and got.min == got.max == (float(low),) * 2
        assert got.n_rail == (cap, cap) and got.n_samples == cap
        assert got.hist[0][0] == cap and got.hist[1][0] == cap and got.hist.sum() == 2 * cap


# ------------------------------------------------------------------------------------------------ 3. the sign flip, few levels
@pytest.mark.parametrize("bits", [1, 2])
def test_packed_uploads_are_probed_as_their_levels(engine, bits):
    rng = np.random.default_rng(300 + bits)
    levels = rng.choice(np.arange(-127, 127), (1 << bits) - 2, replace=False).tolist() + [-128, 127] if bits > 1 else [127, -128]
    p = pk.Packing(bits, [int(v) for v in rng.permutation(levels)], msb_first=bool(bits & 1))
    packed = rng.integers(0, 256, pk.packed_bytes(p, CAP)).astype(np.uint8)
    engine.iq_alloc(CAP, FMT_CI8)
    engine.iq_upload_packed(packed, CAP, p, 0)
    raw = pk.unpack(packed, p)
    for start, n in ((0, CAP), (12345, 40001), (CAP - 77, 1000), (9, 7)):
        want = pb.probe(cases.window(raw, start, n, CAP))
        got = engine.iq_probe(start, n)
        assert got.raw() == want.raw(), (start, n, got, want)
        assert np.array_equal(got.hist, want.hist)
    assert np.count_nonzero(want.hist) <= 2 << bits
    assert np.count_nonzero(pb.probe(raw).hist[0]) == 1 << bits                     # every level of the hostile table is there


# ------------------------------------------------------------------------------------------------ 4. float rings
@pytest.mark.parametrize("fmt", [FMT_CF32, FMT_CF64])
def test_float_rings_keep_the_bound_of_any_order_of_additions(engine, fmt):
    rng = np.random.default_rng(400 + fmt)
    dt = cases.NP_OF_FMT[fmt]
    raw = (rng.standard_normal(2 * CAP) * 10.0 ** rng.uniform(-3, 3, 2 * CAP)).astype(dt)
    bad = rng.integers(0, 2 * CAP, 40)
    raw[bad[:15]] = np.nan
    raw[bad[15:30]] = np.inf
    raw[bad[30:]] = -np.inf
    raw[2 * 500:2 * 503] = np.nan                                                  # three samples with nothing finite
    fill(engine, fmt, raw)
    worst = 0.0
    for start, n in cases.moment_windows(rng) + [(500, 3)]:
        win = cases.window(raw, start, n, CAP)
        want, got = pb.probe(win), engine.iq_probe(start, n, hist=False)
        assert (got.n_samples, got.n_nonfinite, got.n_rail) == (n, want.n_nonfinite, (0, 0)) and got.hist is None
        assert np.array_equal(got.min + got.max, want.min + want.max, equal_nan=True), (start, n, got, want)    # exact
        i, q = win[0::2].astype(np.float64), win[1::2].astype(np.float64)
        ok = np.isfinite(i) & np.isfinite(q)
        i, q = i[ok], q[ok]
        terms = {"sum": (i, q), "sum_sq": (i * i, q * q)}
        for name, (ti, tq) in terms.items():
            for c, t in enumerate((ti, tq)):
                bound = n * 2.0 ** -53 * float(np.abs(t).sum())
                err = abs(getattr(got, name)[c] - getattr(want, name)[c])
                assert err <= bound, (name, c, start, n, err, bound)
                worst = max(worst, err / bound if bound else 0.0)
        bound = n * 2.0 ** -53 * float(np.abs(i * q).sum())
        assert abs(got.sum_iq - want.sum_iq) <= bound, (start, n)
    print(f"{cases.FMT_NAMES[fmt]}: sums within {worst:.3g} of the bound n * 2^-53 * sum|term|")
    lone = engine.iq_probe(500, 3, hist=False)
    assert lone.n_nonfinite == 3 and all(np.isnan(v) for v in lone.min + lone.max) and lone.sum == (0.0, 0.0)
    with pytest.raises(SdrError) as err:
        engine.iq_probe(0, 64, hist=True)
    assert err.value.status == UNSUPPORTED


# ------------------------------------------------------------------------------------------------ 5. the spectrum
@pytest.mark.parametrize("fmt", [FMT_CI8, FMT_CI16, FMT_CF32, FMT_CF64])
def test_spectrum_equals_the_statement(engine, fmt):
    rng = np.random.default_rng(500 + fmt)
    fs = 4e6
    raw = cases.noise_and_tone(rng, fmt, fs=fs)
    fill(engine, fmt, raw)
    worst = 0.0
    for k, (nfft, S, tail) in enumerate(cases.psd_cases()):
        n = (S - 1) * (nfft // 2) + nfft + tail
        start = int(rng.integers(0, CAP // 2)) * 2 + 1                             # odd
        if k % 2:
            start = CAP - int(rng.integers(1, n))                                  # across the ring's end
        want = pb.probe(cases.window(raw, start, n, CAP), nfft=nfft, fs=fs)
        got = engine.iq_probe(start, n, nfft=nfft, fs=fs, hist=False)
        assert got.n_segments == S == want.n_segments
        err = float(np.max(np.abs(got.psd - want.psd)) / want.psd.max())
        worst = max(worst, err)
        assert err <= 1e-9, (nfft, S, tail, start, err)
        assert got.spurs(20.0)[0][0] == want.spurs(20.0)[0][0]                     # the tone, in the same bin
        if fmt in (FMT_CI8, FMT_CI16):
            assert got.raw() == want.raw()
    print(f"{cases.FMT_NAMES[fmt]}: worst |psd - statement| = {worst:.3g} of the peak")


def test_a_tone_on_a_bin_peaks_there_with_its_power(engine):
    nfft, S, A, fs = 256, 5, 3.25, 2.5e6
    n = (S - 1) * (nfft // 2) + nfft
    w = pb.hann_periodic(nfft)
    expect = A * A * w.sum() ** 2 / (fs * (w * w).sum())
    for k in (37, nfft - 37):
        x = np.tile(A * np.exp(2j * np.pi * k * np.arange(nfft) / nfft), CAP // nfft)   # (the ring is a whole number of periods)
        fill(engine, FMT_CF64, x)
        for start in (0, 3 * nfft + 1, CAP - 300):
            got = engine.iq_probe(start, n, nfft=nfft, fs=fs, hist=False)
            assert int(np.argmax(got.psd)) == k, (k, start)
            assert abs(got.psd[k] - expect) <= 1e-12 * expect, (k, start, got.psd[k], expect)
            assert got.frequencies()[k] == (k if k < nfft // 2 else k - nfft) * fs / nfft


@pytest.mark.parametrize("fmt", [FMT_CF32, FMT_CF64])
def test_a_non_finite_sample_in_a_used_segment_is_reported(engine, fmt):
    rng = np.random.default_rng(550 + fmt)
    raw = cases.noise_and_tone(rng, fmt)
    nfft, start = 256, 1001
    n = 3 * 128 + 256 + 100                                                         # four segments and a tail of 100
    raw[2 * (start + 300) + 1] = np.inf                                             # inside segments 1 and 2
    raw[2 * (start + n - 5)] = np.nan                                               # in the tail no segment uses
    fill(engine, fmt, raw)
    got = engine.iq_probe(start, n, nfft=nfft, fs=1e6, hist=False)
    want = pb.probe(cases.window(raw, start, n, CAP), nfft=nfft, fs=1e6)
    assert np.isnan(got.psd).all() and np.isnan(want.psd).all()
    assert got.n_nonfinite == 2 and got.n_segments == 4 and np.isfinite(got.sum + got.sum_sq + got.min + got.max).all()
    got = engine.iq_probe(start + 400, n - 400, nfft=nfft, fs=1e6, hist=False)      # only the NaN of the tail is left
    want = pb.probe(cases.window(raw, start + 400, n - 400, CAP), nfft=nfft, fs=1e6)
    assert got.n_nonfinite == 1 and np.isfinite(got.psd).all()
    assert np.max(np.abs(got.psd - want.psd)) <= 1e-9 * want.psd.max()


# ------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("fmt", [FMT_CI8, FMT_CF32])
def test_two_identical_calls_return_identical_bytes(engine, fmt):
    rng = np.random.default_rng(600 + fmt)
    fill(engine, fmt, cases.noise_and_tone(rng, fmt))
    lib, h = engine._lib, engine._h
    outs = []
    for _ in range(2):
        res, psd = _lib.ProbeResultC(), np.zeros(1024)
        hist = np.zeros((2, 256), dtype=np.int64)
        assert lib.sdr_iq_probe(h, CAP - 4001, 60001, 0, 1024, 4e6, C.byref(res), hist.ctypes.data if fmt == FMT_CI8 else None,
                                psd.ctypes.data) == 0
        outs.append((bytes(res), hist.tobytes(), psd.tobytes()))
    assert outs[0] == outs[1]


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_the_probe_refuses_what_it_cannot_take(engine):
    lib, h = engine._lib, engine._h
    cap = 4096
    engine.iq_alloc(cap, FMT_CI16)
    res = _lib.ProbeResultC()
    C.memset(C.byref(res), 0x5A, C.sizeof(res))
    before = bytes(res)
    hist, psd = np.full((2, 256), -7, dtype=np.int64), np.full(4096, -7.0)
    hp, pp = hist.ctypes.data, psd.ctypes.data

    def refused(status, *args):
        assert lib.sdr_iq_probe(*args) == status, args
        assert lib.sdr_last_error(), args
        assert bytes(res) == before and (hist == -7).all() and (psd == -7.0).all(), args

    r = C.byref(res)
    refused(INVALID, None, 0, 64, 0, 64, 1e6, r, hp, pp)                 # no engine
    refused(INVALID, h, 0, 64, 0, 64, 1e6, None, hp, pp)                 # no result block
    refused(INVALID, h, 0, 0, 0, 64, 1e6, r, hp, pp)                     # n_samples < 1
    refused(INVALID, h, 0, 64, -1, 64, 1e6, r, hp, pp)                   # negative hist_shift
    refused(INVALID, h, 0, 64, 9, 64, 1e6, r, hp, pp)                    # ... too large for ci16
    for nfft in (0, 32, 96, 8192):
        refused(INVALID, h, 0, cap, 0, nfft, 1e6, r, hp, pp)             # nfft no power of two in 64..4096
    for fs in (0.0, -1.0, float("inf"), float("nan")):
        refused(INVALID, h, 0, 64, 0, 64, fs, r, hp, pp)
    refused(INVALID, h, 0, 63, 0, 64, 1e6, r, hp, pp)                    # n_samples < nfft
    refused(UNSUPPORTED, h, 0, (1 << 31) + 1, 0, 64, 1e6, r, hp, pp)     # n_samples > 2^31
    refused(RANGE, h, -1, 64, 0, 64, 1e6, r, hp, pp)                     # negative start_sample
    refused(RANGE, h, 0, cap + 1, 0, 64, 1e6, r, hp, pp)                 # longer than the ring
    # without a spectrum nfft and fs are not looked at; any start_sample >= 0; n up to the capacity
    assert lib.sdr_iq_probe(h, 7 * cap + 5, cap, 8, 0, 0.0, C.byref(_lib.ProbeResultC()), None, None) == 0
    engine.iq_alloc(cap, FMT_CI8)
    refused(INVALID, h, 0, 64, 1, 64, 1e6, r, hp, pp)                    # ci8 takes hist_shift 0 only
    engine.iq_alloc(cap, FMT_CF32)
    refused(UNSUPPORTED, h, 0, 64, 0, 64, 1e6, r, hp, pp)                # no histogram of a float ring
    e2 = Engine(0)
    try:
        refused(STATE, e2._h, 0, 64, 0, 64, 1e6, r, hp, pp)              # no ring
    finally:
        e2.close()


# ------------------------------------------------------------------------------------------------ 8. ordering, nothing written
def test_a_probe_sees_the_upload_queued_before_it_and_writes_nothing(engine):
    rng = np.random.default_rng(800)
    old = cases.integer_ring(rng, FMT_CI8)
    fill(engine, FMT_CI8, old)
    block = engine.host_alloc(2 * 30000, np.int8)
    try:
        block[:] = rng.integers(-128, 128, block.size).astype(np.int8)
        off = CAP - 10000                                                           # the new samples wrap
        engine.iq_upload_queue(block, off)
        got = engine.iq_probe(off - 100, 30200, nfft=256, fs=1e6)                   # no sync in between
        mirror = old.copy()
        mirror[(2 * off + np.arange(block.size)) % (2 * CAP)] = block
        want = pb.probe(cases.window(mirror, off - 100, 30200, CAP), nfft=256, fs=1e6)
        assert got.raw() == want.raw() and np.array_equal(got.hist, want.hist)
        assert np.max(np.abs(got.psd - want.psd)) <= 1e-9 * want.psd.max()
        ring = engine.iq_download(CAP, 0)
        assert np.array_equal(ring, mirror)
        engine.iq_probe(0, CAP, nfft=4096, fs=1e6)
        assert engine.iq_download(CAP, 0).tobytes() == ring.tobytes()               # byte for byte what it was
        # the profiling scopes
        engine.prof_enable(True)
        engine.prof_reset()
        engine.iq_probe(0, CAP, nfft=1024, fs=1e6)
        moments, psd = engine.prof_read("probe_moments_kernel"), engine.prof_read("probe_psd_kernel")
        engine.prof_enable(True, calls_only=True)
        engine.prof_reset()
        engine.iq_probe(0, CAP, nfft=1024, fs=1e6)
        call = engine.prof_read("call_iq_probe")
        engine.prof_enable(False)
        engine.prof_reset()
        assert moments[1] == 1 and psd[1] == 1 and call[1] == 1 and min(moments[0], psd[0], call[0]) > 0
    finally:
        engine.host_free(block)


# ------------------------------------------------------------------------------------------------ 9. a receiver is not disturbed
def test_a_receiver_that_is_probed_hands_out_the_same_packets(engine):
    """A ChannelManager at 4 MHz over two synthesised satellites (the receivers of tests/test_gpu_bank.py): once with
    probeRFData(5) every 50 ticks -- in front of run(), where the tick's slab is still only queued, and behind it -- and once
    without: every packet of every tick equal; every probe equal to the statement on the last 5 ms of the recording."""
    from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.signal.iqsource import RFSignal
    fs, n_ms = 4e6, 300
    spms = int(fs * 1e-3)
    sats = [dict(prn=5, doppler=1310.0, code_phase=211.3, phase=0.2, amp=6.0), dict(prn=17, doppler=-2740.0, code_phase=800.6, phase=0.7, amp=6.0)]
    total = n_ms * spms
    engine.iq_alloc(total, FMT_CI8)
    engine.code_slots(32)
    engine.iq_synth(sats, fs, 10.0, 9091, 0, total)
    raw = engine.iq_download(total, 0)
    cfg = packed_cases.kaplan_config()

    def receiver(probing):
        rf = RFSignal(dict(filepath="none", sampling_frequency=fs, is_complex="true", intermediate_frequency=0.0, data_size=8))
        mgr = ChannelManager(rf, engine=engine, keepCorrelationMap=False)
        mgr.addChannel(ChannelL1CA_Kaplan, cfg, 2)
        for s in sats:
            mgr.requestTracking(s["prn"])
        ticks, probes = [], []
        for k in range(n_ms):
            mgr.addNewRFData(raw[2 * k * spms:2 * (k + 1) * spms])
            if probing and k % 100 == 49:
                probes.append((k, mgr.probeRFData(5)))
            ticks.append([packed_cases.plain(p) for p in mgr.run()])
            if probing and k % 100 == 99:
                probes.append((k, mgr.probeRFData(5)))
        mgr.close()
        return ticks, probes

    plain, _ = receiver(False)
    probed, probes = receiver(True)
    assert len(probes) == 6 and packed_cases.count(plain) > 2 * 250
    for k, (a, b) in enumerate(zip(plain, probed)):
        assert a == b, k
    for k, got in probes:
        want = pb.probe(raw[2 * (k - 4) * spms:2 * (k + 1) * spms], nfft=1024, fs=fs)
        assert got.raw() == want.raw() and np.array_equal(got.hist, want.hist), k
        assert got.n_samples == 5 * spms and got.n_segments == want.n_segments
        assert np.max(np.abs(got.psd - want.psd)) <= 1e-9 * want.psd.max(), k
