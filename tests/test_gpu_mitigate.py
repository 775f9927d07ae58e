"""The device's pulse blanker and narrow-band excisor (sdr_ddc_mitigate, sydr_amd/csrc/mitigate.hip) against their NumPy
statement (sydr_amd/signal/mitigate.py): what the ring and the counters hold after a push, however the stream was cut into
pushes, wherever the window lies in the ring; the lifetime rules and the refusals; what sdr_iq_probe and sdr_pcps see of the
mitigated ring; a receiver over a jammed recording.

Tolerance (derived, not measured; docs/notes/mitigate.md): two implementations of a segment's two transforms differ by at most
B_mit = 16 log2(N) N 2^-53 max|u| per component, plus twice the converter's own gain * B (mitigate_cases.tolerance).  A gate
is a discontinuity, so every comparison first asserts of the statement alone that no bin lies within a relative 1e-9 of its
limit, no sample's power within a relative 1e-12 of the squared level and -- integer rings -- no component of y within the
tolerance of a half-integer (mitigate_cases.assert_unambiguous); then counters are equal as integers and integer rings byte for
byte.  Every test prints the worst observed error as a fraction of the tolerance."""
import ctypes as C

import numpy as np
import pytest

import downconvert_cases as dcases
import mitigate_cases as cases

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI8, FMT_CI16
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt
from sydr_amd.utils.enumerations import ChannelMessage

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -6
RING_FORMATS, RING_NAMES = dcases.RING_FORMATS, dcases.RING_NAMES


def ring_capacity(n_out: int) -> int:
    return -(-(n_out + 8) // 8) * 8


def check_ring(got: np.ndarray, y: np.ndarray, band: float, ring_fmt: int, what):
    """`got`: the downloaded window (interleaved, the ring's type); y: the statement's outputs; the gates were asserted
    unambiguous by the caller.  -> the worst error as a fraction of the tolerance (integer rings: 0, they are equal)."""
    if ring_fmt in (FMT_CI8, FMT_CI16):
        want = dc.quantise(y, ring_fmt)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
        return 0.0
    pair = dc.quantise(y, FMT_CF64)
    err = np.abs(got.astype(np.float64) - pair)
    bound = band + (2.0 ** -24 * np.abs(pair) if ring_fmt == FMT_CF32 else 0.0)
    worst = int(np.argmax(err - bound))
    ratio = float(np.max(err / bound)) if band > 0.0 else float(err.max() > 0.0)
    print(f"{what}: max |ring - y| = {err.max():.3e}, tolerance {band:.3e}, worst ratio {ratio:.3g}")
    assert np.all(err <= bound), (what, worst, err[worst], band)
    return ratio


def mitigated_converter(engine, ddc_cfg, cfg):
    ddc = engine.ddc_create(ddc_cfg)
    try:
        engine.ddc_mitigate(ddc, cfg)
    except Exception:
        engine.ddc_destroy(ddc)
        raise
    return ddc


# ------------------------------------------------------------------------------------------------ 1. ring and counters equal the statement
@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("shape", cases.CONVERTERS, ids=lambda s: f"T{s[0]}_D{s[1]}")
@pytest.mark.parametrize("nfft", cases.NFFTS, ids=lambda n: f"N{n}")
def test_ring_and_counters_equal_the_statement(engine, nfft, shape, mode):
    T, D = shape
    raw = cases.jammed()
    n_out = dc.out_count(0, cases.N_INPUTS, D)
    worst = 0.0
    for ring_fmt in RING_FORMATS:
        engine.iq_alloc(ring_capacity(n_out), ring_fmt)
        gain = cases.gain_for(T, ring_fmt)
        for name, fcw in cases.FCWS.items():
            what = (f"N{nfft}", T, D, mode, RING_NAMES[ring_fmt], name)
            ddc_cfg = cases.converter(T, D, fcw, gain)
            v = cases.converted(T, D, fcw, gain)
            cfg, y, stats = cases.mitigated(T, D, fcw, gain, nfft, mode)
            band = cases.tolerance(cfg, ddc_cfg, v, raw)
            cases.assert_unambiguous(cfg, v, y, band, ring_fmt in (FMT_CI8, FMT_CI16), what)
            assert stats.n_outputs == n_out and (mode == "excise" or stats.n_triggers > 0) and (mode == "blank" or stats.n_bins_excised > 0)
            ddc = mitigated_converter(engine, ddc_cfg, cfg)
            try:
                assert engine.ddc_delay(ddc) == cfg.delay
                assert engine.ddc_out_count(ddc, cases.N_INPUTS) == n_out
                assert engine.ddc_push(ddc, raw, 0) == n_out
                got_stats = engine.ddc_mitigation_stats(ddc)
            finally:
                engine.ddc_destroy(ddc)
            assert got_stats == stats, (what, got_stats, stats)
            worst = max(worst, check_ring(engine.iq_download(n_out, 0), y, band, ring_fmt, what))
    print(f"worst ratio to the tolerance over the case: {worst:.3g}")


@pytest.mark.parametrize("lead,hold", [(0, 0), (1024, 1024), (0, 1024), (1024, 0)])
def test_blanker_with_no_reach_and_with_the_longest(engine, lead, hold):
    """The blanker alone at the ends of its range: no state at all, and a halo of 2048 triggers around a tile of 1024."""
    n = 9001
    raw, v = cases.jammed(n), cases.converted(1, 1, 0, 1.0, n)
    cfg = mt.MitigationConfig(cases.LEVEL, lead, hold)
    st = mt.Statement(cfg)
    y = st.push(v)
    cases.assert_unambiguous(cfg, v, y, 0.0, False)
    engine.iq_alloc(ring_capacity(n), FMT_CF64)
    ddc = mitigated_converter(engine, cases.converter(1, 1, 0, 1.0), cfg)
    try:
        assert engine.ddc_delay(ddc) == lead and engine.ddc_push(ddc, raw[:2 * 4000].copy(), 0) == 4000       # (two pushes: the state is used)
        assert engine.ddc_push(ddc, raw[2 * 4000:].copy(), 4000) == n - 4000
        assert engine.ddc_mitigation_stats(ddc) == st.stats and st.stats.n_blanked >= st.stats.n_triggers > 0
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(engine.iq_download(n, 0), dc.quantise(y, FMT_CF64))          # (the identity converter: v is exact, u is v or 0)


# ------------------------------------------------------------------------------------------------ 2. the cut does not matter
@pytest.mark.parametrize("ring_fmt", [FMT_CI8, FMT_CF64], ids=lambda f: "ring_" + RING_NAMES[f])
@pytest.mark.parametrize("shape,nfft,mode", [((1, 1), 1024, "both"), ((33, 2), 64, "both"), ((1, 1), 4096, "excise"), ((33, 2), 1024, "blank")])
def test_the_ring_does_not_depend_on_how_the_stream_was_cut(engine, ring_fmt, shape, nfft, mode):
    T, D = shape
    n = 30001
    raw = cases.jammed(n)
    gain = cases.gain_for(T, ring_fmt)
    ddc_cfg = cases.converter(T, D, cases.FCWS["odd"], gain)
    cfg = cases.settings(cases.converted(T, D, ddc_cfg.fcw, gain, n), nfft, mode, gain)
    total = dc.out_count(0, n, D)
    engine.iq_alloc(ring_capacity(total), ring_fmt)
    ddc = mitigated_converter(engine, ddc_cfg, cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == total
        whole, whole_stats = engine.iq_download(total, 0), engine.ddc_mitigation_stats(ddc)
        engine.iq_upload(np.zeros(2 * engine.iq_capacity, dtype=whole.dtype), 0)
        engine.ddc_reset(ddc)
        at = 0
        lengths = [D * k for k in cases.push_lengths(nfft)]        # (in inputs: a push shorter than blank_hold, an empty one)
        for piece in cases.cut(raw, lengths, 2):
            want = engine.ddc_out_count(ddc, piece.size // 2)
            assert engine.ddc_push(ddc, np.ascontiguousarray(piece), at) == want
            at += want
        assert at == total
        pieces, pieces_stats = engine.iq_download(total, 0), engine.ddc_mitigation_stats(ddc)
    finally:
        engine.ddc_destroy(ddc)
    assert np.all(pieces == whole), np.flatnonzero(pieces != whole)[:8]
    assert pieces_stats == whole_stats, (pieces_stats, whole_stats)
    assert whole_stats.n_outputs == total and whole_stats.n_segments == mt.segments_finished(total, cfg.delay, cfg.nfft)


# ------------------------------------------------------------------------------------------------ 3. ring position
@pytest.mark.parametrize("ring_fmt", RING_FORMATS, ids=lambda f: "ring_" + RING_NAMES[f])
def test_a_window_across_the_rings_end_the_delay_and_nothing_outside(engine, ring_fmt):
    T, D, nfft, cap, n = 33, 2, 64, 4096, 6001
    raw = cases.jammed(n)
    gain = cases.gain_for(T, ring_fmt)
    ddc_cfg = cases.converter(T, D, cases.FCWS["quarter"], gain)
    v = cases.converted(T, D, ddc_cfg.fcw, gain, n)
    cfg, y, _ = cases.mitigated(T, D, ddc_cfg.fcw, gain, nfft, "both", n)
    band = cases.tolerance(cfg, ddc_cfg, v, raw)
    cases.assert_unambiguous(cfg, v, y, band, ring_fmt in (FMT_CI8, FMT_CI16))
    pattern = np.random.default_rng(cases.SEED + 3).integers(-100, 101, 2 * cap).astype(dcases.RING_DTYPE[ring_fmt])
    engine.iq_alloc(cap, ring_fmt)
    engine.iq_upload(pattern, 0)
    off = cap - 1000
    ddc = mitigated_converter(engine, ddc_cfg, cfg)
    try:
        assert engine.ddc_delay(ddc) == cfg.delay == mt.Statement(cfg).delay == nfft + cases.LEAD
        assert engine.ddc_push(ddc, raw, off) == y.size == 3001
    finally:
        engine.ddc_destroy(ddc)
    ring = engine.iq_download(cap, 0)
    inside = (2 * off + np.arange(2 * y.size)) % (2 * cap)
    outside = np.ones(2 * cap, dtype=bool)
    outside[inside] = False
    assert np.array_equal(ring[outside].view(np.uint8), pattern[outside].view(np.uint8))
    assert np.all(ring[inside][:2 * cfg.delay] == 0) and np.any(ring[inside][2 * cfg.delay:2 * cfg.delay + 16] != 0)   # format(0), then the stream
    check_ring(ring[inside], y, band, ring_fmt, "across the end")


# ------------------------------------------------------------------------------------------------ 4. state and lifetime
def _status(fn):
    with pytest.raises(SdrError) as err:
        fn()
    return err.value.status


def test_reset_two_converters_attach_and_detach(engine):
    ring_fmt, n = FMT_CF64, 9000
    raw = cases.jammed(n)
    ddc_a, ddc_b = cases.converter(1, 1, 0, 1.0), cases.converter(33, 2, cases.FCWS["odd"], dcases.GOLD)
    cfg_a = cases.settings(cases.converted(1, 1, 0, 1.0, n), 1024, "both")
    cfg_b, y_b, stats_b = cases.mitigated(33, 2, ddc_b.fcw, dcases.GOLD, 64, "excise", n)
    engine.iq_alloc(16384, ring_fmt)
    a, b, plain = mitigated_converter(engine, ddc_a, cfg_a), mitigated_converter(engine, ddc_b, cfg_b), engine.ddc_create(ddc_a)
    try:
        assert engine.ddc_push(a, raw, 0) == n
        fresh, fresh_stats = engine.iq_download(n, 0), engine.ddc_mitigation_stats(a)
        engine.ddc_push(a, raw[:2 * 777].copy(), 0)              # (more state, other counters)
        # attaching or detaching needs a converter that has seen no input
        assert _status(lambda: engine.ddc_mitigate(a, cfg_b)) == STATE and _status(lambda: engine.ddc_mitigate(a, None)) == STATE
        assert engine.ddc_delay(a) == cfg_a.delay
        engine.ddc_reset(a)
        assert engine.ddc_mitigation_stats(a) == mt.Statement(cfg_a).stats
        assert engine.ddc_push(a, raw, 0) == n
        assert np.all(engine.iq_download(n, 0) == fresh) and engine.ddc_mitigation_stats(a) == fresh_stats
        # a and b interleaved, push by push, each into its own half of the ring: each keeps its own state and counters
        engine.ddc_reset(a)
        at_a, at_b = 0, 10000
        for lo in range(0, n, 1500):
            piece = np.ascontiguousarray(raw[2 * lo:2 * (lo + 1500)])
            at_a += engine.ddc_push(a, piece, at_a)
            at_b += engine.ddc_push(b, piece, at_b)
        assert np.all(engine.iq_download(n, 0) == fresh) and engine.ddc_mitigation_stats(a) == fresh_stats
        assert at_b - 10000 == y_b.size and engine.ddc_mitigation_stats(b) == stats_b
        v_b = cases.converted(33, 2, ddc_b.fcw, dcases.GOLD, n)
        cases.assert_unambiguous(cfg_b, v_b, y_b, 0.0, False)
        check_ring(engine.iq_download(y_b.size, 10000), y_b, cases.tolerance(cfg_b, ddc_b, v_b, raw), ring_fmt, "second converter")
        # detached after a reset, the converter writes what one that never had a mitigator writes, byte for byte
        engine.ddc_reset(a)
        engine.ddc_mitigate(a, None)
        assert engine.ddc_delay(a) == 0 and _status(lambda: engine.ddc_mitigation_stats(a)) == STATE
        engine.iq_upload(np.zeros(2 * 16384), 0)
        assert engine.ddc_push(a, raw, 0) == n
        detached = engine.iq_download(n, 0)
        engine.iq_upload(np.zeros(2 * 16384), 0)
        assert engine.ddc_push(plain, raw, 0) == n
        assert np.array_equal(detached.view(np.uint8), engine.iq_download(n, 0).view(np.uint8))
    finally:
        for h in (a, b, plain):
            engine.ddc_destroy(h)


def test_push_queue_equals_push(engine):
    ring_fmt, n = FMT_CI16, 30001
    raw = cases.jammed(n)
    gain = cases.gain_for(33, ring_fmt)
    ddc_cfg = cases.converter(33, 2, cases.FCWS["odd"], gain)
    cfg = cases.settings(cases.converted(33, 2, ddc_cfg.fcw, gain, n), 1024, "both", gain)
    engine.iq_alloc(16384, ring_fmt)
    ddc = mitigated_converter(engine, ddc_cfg, cfg)
    try:
        n_out = engine.ddc_push(ddc, raw, 0)
        want, want_stats = engine.iq_download(n_out, 0), engine.ddc_mitigation_stats(ddc)
        engine.iq_upload(np.zeros(2 * 16384, dtype=np.int16), 0)
        engine.ddc_reset(ddc)
        src = raw.copy()
        at = 0
        for lo in range(0, n, 7001):                      # several pushes in flight behind each other, no wait between them
            at += engine.ddc_push_queue(ddc, src[2 * lo:2 * (lo + 7001)], at)
        engine.sync()
        assert at == n_out
        assert np.array_equal(engine.iq_download(n_out, 0), want) and engine.ddc_mitigation_stats(ddc) == want_stats
    finally:
        engine.ddc_destroy(ddc)


def _mitigate_raw(engine, ddc, nfft=0, lead=0, hold=0, flags=0, level=0.0, limit=None):
    arr = (C.c_double * max(len(limit), 1))(*limit) if limit is not None else None
    cfg = _lib.MitCfg(nfft, lead, hold, flags, level, C.cast(arr, C.POINTER(C.c_double)) if arr is not None else None)
    return _lib.load().sdr_ddc_mitigate(engine._h, ddc.handle, C.byref(cfg))


def test_refusals_leave_ring_state_and_counters_as_they_were(engine):
    ring_fmt, n, cap = FMT_CI8, 5000, 8192
    raw = cases.jammed(n)
    ddc_cfg = cases.converter(1, 1, 0, 1.0)
    cfg, y, stats = cases.mitigated(1, 1, 0, 1.0, 64, "both", n)
    engine.iq_alloc(cap, ring_fmt)
    ddc = mitigated_converter(engine, ddc_cfg, cfg)
    bare = engine.ddc_create(ddc_cfg)
    try:
        ok = [1.0] * 64
        for kw in (dict(nfft=32, limit=[1.0] * 32), dict(nfft=8192, limit=[1.0] * 8192), dict(nfft=96, limit=[1.0] * 96), dict(nfft=-64, limit=ok),
                   dict(nfft=64, limit=ok, lead=1025, level=1.0), dict(nfft=64, limit=ok, hold=1025, level=1.0), dict(nfft=64, limit=ok, lead=-1),
                   dict(nfft=64, limit=ok, hold=-1), dict(nfft=64, limit=[1.0] * 63 + [-1.0]), dict(nfft=64, limit=[float("nan")] + [1.0] * 63),
                   dict(nfft=64, limit=ok, level=-1.0), dict(nfft=64, limit=ok, level=float("nan")), dict(nfft=64), dict(nfft=64, limit=ok, flags=1),
                   dict(), dict(lead=3, hold=3)):
            assert _mitigate_raw(engine, bare, **kw) == INVALID, kw
            assert _mitigate_raw(engine, ddc, **kw) == INVALID, kw
            assert engine.ddc_delay(bare) == 0 and engine.ddc_delay(ddc) == cfg.delay
        assert _mitigate_raw(engine, bare, nfft=64, limit=[float("inf")] * 64, lead=1024, hold=1024, level=1.0) == 0
        assert engine.ddc_delay(bare) == 64 + 1024
        # a refused attachment in the middle of a stream: ring, state and counters go on as if it had not been tried
        half = 2 * 2500
        engine.ddc_push(ddc, raw[:half].copy(), 0)
        before, before_stats = engine.iq_download(cap, 0), engine.ddc_mitigation_stats(ddc)
        assert _status(lambda: engine.ddc_mitigate(ddc, cfg)) == STATE and _mitigate_raw(engine, ddc, nfft=32, limit=[1.0] * 32) != 0
        assert _status(lambda: engine.ddc_push(ddc, raw[half:].copy(), cap)) == -5          # SDR_ERR_RANGE: nothing pushed
        assert np.array_equal(engine.iq_download(cap, 0), before) and engine.ddc_mitigation_stats(ddc) == before_stats
        engine.ddc_push(ddc, raw[half:].copy(), 2500)
        assert engine.ddc_mitigation_stats(ddc) == stats
        assert np.array_equal(engine.iq_download(n, 0), dc.quantise(y, ring_fmt))
    finally:
        engine.ddc_destroy(ddc)
        engine.ddc_destroy(bare)


# ------------------------------------------------------------------------------------------------ 5. the probe sees it
def test_the_probe_sees_the_carrier_wave_gone(engine):
    """sdr_iq_probe's Welch spectrum (1024 points) of the ring: the carrier wave stands more than 30 dB over the median bin
    when the recording is uploaded as it is, and no bin within 3 bins of it is more than 6 dB over the median of the
    mitigated ring's spectrum."""
    n, nfft = cases.N_INPUTS, 1024
    raw = cases.jammed()
    cfg, y, _ = cases.mitigated(1, 1, 0, 1.0, nfft, "both")
    engine.iq_alloc(ring_capacity(n), FMT_CI8)
    near = (int(round(cases.CW_CYCLES * nfft)) + np.arange(-3, 4)) % nfft

    def excess_db(first, count):
        psd = engine.iq_probe(first, count, nfft=nfft, fs=1.0, hist=False).psd
        return 10.0 * np.log10(psd[near].max() / np.median(psd))

    engine.iq_upload(raw, 0)
    before = excess_db(0, n)
    ddc = mitigated_converter(engine, cases.converter(1, 1, 0, 1.0), cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == n
    finally:
        engine.ddc_destroy(ddc)
    after = excess_db(cfg.delay, n - cfg.delay)
    print(f"carrier wave over the median bin: {before:.1f} dB before, {after:.1f} dB after")
    assert before > 30.0 and after < 6.0, (before, after)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_search_over_the_mitigated_ring(engine):
    """The acquisition case of tests/test_mitigate.py on the device: the jammed stream through the identity converter and an
    excisor of 1024 points, sdr_pcps one millisecond behind the delay: the oracle's peak sample, bin and ratio (1e-9) on the
    statement's output -- which are the clean stream's."""
    from oracle import sydr_oracle as orc
    clean, jam = cases.acquisition_streams()
    cfg, want_ring = cases.acquisition_mitigated()
    n_code = orc.samples_per_code(cases.ACQ_FS)
    engine.iq_alloc(ring_capacity(cases.ACQ_MS * n_code), FMT_CI8)
    ddc = mitigated_converter(engine, dc.DownConverterConfig(dc.IN_CI8), cfg)
    try:
        assert engine.ddc_push(ddc, jam, 0) == cases.ACQ_MS * n_code
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(engine.iq_download(cases.ACQ_MS * n_code, 0), want_ring)
    engine.code_slots(1)
    engine.load_gps_code(0, cases.ACQ_PRN)
    pb, pc, pr, _ = engine.pcps([0], cfg.delay, cases.ACQ_FS, 0.0, 5000.0, 250.0, 1, 1)
    peak, ratio = cases.acquire(want_ring, cfg.delay)
    assert [int(pb[0]), int(pc[0])] == peak and abs(pr[0] - ratio) <= 1e-9 * ratio, (pb, pc, pr, peak, ratio)
    assert peak == cases.acquire(clean)[0] and ratio > 2.0


def test_receiver_over_the_jammed_recording(engine, tmp_path):
    """A ChannelManager over the jammed file with the mitigation keys set hands out the packets of a manager over the
    statement's output stored as an ordinary complex int8 recording, bit for bit."""
    import packed_cases
    sig, plain_sig, out = cases.write_jammed_and_mitigated(tmp_path)
    ms, prn = cases.REC_MS, dcases.SATELLITE["prn"]
    assert sig.frontEnd.mitigation.nfft == 1024 and sig.frontEnd.mitigation.blanking and sig.frontEnd.delay == 1024 + 2
    cfg = packed_cases.kaplan_config()
    got, mgr = packed_cases.receive(sig, engine, prns=[prn], cfg=cfg, ms=ms, mode="ticks")
    stats = mgr.mitigationStats()
    mgr.close()
    want, want_mgr = packed_cases.receive(plain_sig, engine, prns=[prn], cfg=cfg, ms=ms, mode="ticks")
    assert want_mgr.mitigationStats() is None
    want_mgr.close()
    st = mt.Statement(sig.frontEnd.mitigation)
    st.push(dc.statement(sig.frontEnd.config, [cases.jammed_recording()]))
    assert stats == st.stats and stats.n_bins_excised > 0
    assert len(got) == len(want) == ms
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, k
    assert packed_cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 1 and packed_cases.count(got) > 40
