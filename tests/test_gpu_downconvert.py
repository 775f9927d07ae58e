"""The device-resident down-converter (sdr_ddc_*, sydr_amd/csrc/ddc.hip) against its NumPy statement
(sydr_amd/signal/downconvert.py): what the ring holds after a push, however the stream was cut into pushes, wherever the
window lies in the ring; the refusals; and everything downstream of the ring over a converted real recording.

Tolerance (derived, not measured): B = (T + 16) * 2^-53 * sum|h| * max|x| is what any order of T fp64 products and sums
keeps, plus a few ulp for the phasor.  cf64 rings: |ring - v| <= gain * B; cf32 rings: + 2^-24 * |v|; integer rings: the
test first asserts that NO component of the statement lies within gain * B of a half-integer, then demands byte equality."""
import ctypes as C

import numpy as np
import pytest

import downconvert_cases as cases

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI8, FMT_CI16, Engine
from sydr_amd.signal import downconvert as dc
from sydr_amd.utils.enumerations import ChannelMessage

pytestmark = pytest.mark.gpu

INVALID, RANGE, STATE = -1, -5, -6


def ring_capacity(n_out: int) -> int:
    return -(-(n_out + 8) // 8) * 8


def check_ring(got: np.ndarray, v: np.ndarray, cfg, ring_fmt: int, x_max: float, what):
    """`got`: the downloaded window (interleaved, the ring's type); v: the statement's outputs."""
    band = dc.tolerance(cfg, x_max)
    if ring_fmt in (FMT_CI8, FMT_CI16):
        assert dc.ambiguous(v, band) == 0, ("statement output near a rounding tie", what)
        want = dc.quantise(v, ring_fmt)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
        return
    pair = dc.quantise(v, FMT_CF64)
    err = np.abs(got.astype(np.float64) - pair)
    bound = band + (2.0 ** -24 * np.abs(pair) if ring_fmt == FMT_CF32 else 0.0)
    worst = int(np.argmax(err - bound))
    print(f"{what}: max |ring - v| = {err.max():.3e}, bound {band:.3e}")
    assert np.all(err <= bound), (what, worst, err[worst], band)


# ------------------------------------------------------------------------------------------------ 1. ring equals statement
@pytest.mark.parametrize("shape", cases.SHAPES, ids=lambda s: f"T{s[0]}_D{s[1]}")
@pytest.mark.parametrize("ring_fmt", cases.RING_FORMATS, ids=lambda f: "ring_" + cases.RING_NAMES[f])
@pytest.mark.parametrize("in_fmt", cases.IN_FORMATS, ids=lambda f: "in_" + cases.IN_NAMES[f])
def test_ring_equals_the_statement(engine, in_fmt, ring_fmt, shape):
    T, D = shape
    raw = cases.stream(in_fmt)
    x_max = cases.max_abs(in_fmt, raw)
    n_out = dc.out_count(0, cases.N_INPUTS, D)
    engine.iq_alloc(ring_capacity(n_out), ring_fmt)
    for name, fcw in cases.FCWS.items():
        gain = cases.gain_for(in_fmt, ring_fmt)
        cfg = cases.config(in_fmt, T, D, fcw, gain)
        v = cases.reference(in_fmt, T, D, fcw, gain)
        ddc = engine.ddc_create(cfg)
        try:
            assert engine.ddc_out_count(ddc, cases.N_INPUTS) == n_out == v.size
            assert engine.ddc_push(ddc, raw, 0) == n_out
        finally:
            engine.ddc_destroy(ddc)
        check_ring(engine.iq_download(n_out, 0), v, cfg, ring_fmt, x_max, (cases.IN_NAMES[in_fmt], cases.RING_NAMES[ring_fmt], T, D, name))


# ------------------------------------------------------------------------------------------------ 2. chunk invariance
CHUNKED = [(dc.IN_R8, FMT_CF64, 33, 2), (dc.IN_CI16, FMT_CF64, 17, 3), (dc.IN_CI8, FMT_CF64, 512, 16), (dc.IN_R16, FMT_CF32, 65, 5),
           (dc.IN_R16, FMT_CI16, 33, 2), (dc.IN_CI8, FMT_CI8, 17, 3), (dc.IN_R8, FMT_CF64, 1, 1), (dc.IN_CI16, FMT_CF64, 2, 1),
           (dc.IN_R8, FMT_CF64, 3, 64)]


@pytest.mark.parametrize("in_fmt,ring_fmt,T,D", CHUNKED)
def test_the_ring_does_not_depend_on_how_the_stream_was_cut(engine, in_fmt, ring_fmt, T, D):
    n = 20001
    raw = cases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, T, D, cases.FCWS["odd"], cases.gain_for(in_fmt, ring_fmt))
    total = dc.out_count(0, n, D)
    engine.iq_alloc(ring_capacity(total), ring_fmt)
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == total
        whole = engine.iq_download(total, 0)
        engine.iq_upload(np.zeros(2 * engine.iq_capacity, dtype=whole.dtype), 0)
        engine.ddc_reset(ddc)
        st = dc.Statement(cfg)
        at = 0
        for piece in cases.cut(raw, in_fmt, cases.push_lengths(T)):
            n_in = piece.size // (2 if dc.input_is_complex(in_fmt) else 1)
            want = st.out_count(n_in)
            assert engine.ddc_out_count(ddc, n_in) == want
            assert engine.ddc_push(ddc, np.ascontiguousarray(piece), at) == want == st.push(piece).size
            at += want
        assert at == total
        pieces = engine.iq_download(total, 0)
    finally:
        engine.ddc_destroy(ddc)
    assert np.all(pieces == whole), np.flatnonzero(pieces != whole)[:8]
    check_ring(whole, cases.reference(in_fmt, T, D, cfg.fcw, cfg.gain, n), cfg, ring_fmt, cases.max_abs(in_fmt, raw), "one push")


# ------------------------------------------------------------------------------------------------ 3. a window across the ring's end
@pytest.mark.parametrize("ring_fmt", cases.RING_FORMATS, ids=lambda f: "ring_" + cases.RING_NAMES[f])
def test_a_window_across_the_rings_end_and_nothing_outside_it(engine, ring_fmt):
    in_fmt, T, D, cap, n = dc.IN_R8, 33, 2, 4096, 6001
    raw = cases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, T, D, cases.FCWS["quarter"], cases.gain_for(in_fmt, ring_fmt))
    v = cases.reference(in_fmt, T, D, cfg.fcw, cfg.gain, n)
    rng = np.random.default_rng(cases.SEED + 3)
    pattern = rng.integers(-100, 101, 2 * cap).astype(cases.RING_DTYPE[ring_fmt])
    engine.iq_alloc(cap, ring_fmt)
    engine.iq_upload(pattern, 0)
    off = cap - 1000
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, raw, off) == v.size == 3001
    finally:
        engine.ddc_destroy(ddc)
    ring = engine.iq_download(cap, 0)
    inside = (2 * off + np.arange(2 * v.size)) % (2 * cap)
    outside = np.ones(2 * cap, dtype=bool)
    outside[inside] = False
    assert np.array_equal(ring[outside].view(np.uint8), pattern[outside].view(np.uint8))
    check_ring(ring[inside], v, cfg, ring_fmt, cases.max_abs(in_fmt, raw), "across the end")


# ------------------------------------------------------------------------------------------------ 4. reset, two converters
def test_reset_and_two_converters_on_one_engine(engine):
    in_fmt, ring_fmt, n = dc.IN_CI8, FMT_CF64, 5000
    raw, other = cases.stream(in_fmt, n), cases.stream(dc.IN_R16, n)
    cfg = cases.config(in_fmt, 33, 2, cases.FCWS["odd"], cases.GOLD)
    cfg_b = cases.config(dc.IN_R16, 17, 3, cases.FCWS["quarter"], cases.GOLD)
    engine.iq_alloc(8192, ring_fmt)
    a, b = engine.ddc_create(cfg), engine.ddc_create(cfg_b)
    try:
        n_a = engine.ddc_push(a, raw, 0)
        fresh = engine.iq_download(n_a, 0)
        engine.ddc_push(a, raw[:2 * 777], 0)             # (more history, another index)
        engine.ddc_reset(a)
        assert engine.ddc_push(a, raw, 0) == n_a
        assert np.all(engine.iq_download(n_a, 0) == fresh)
        # a and b interleaved, push by push, each into its own half of the ring: what each leaves is its own stream's statement
        engine.ddc_reset(a)
        at_a, at_b = 0, 4096
        for lo in range(0, n, 1250):
            at_a += engine.ddc_push(a, np.ascontiguousarray(raw[2 * lo:2 * (lo + 1250)]), at_a)
            at_b += engine.ddc_push(b, np.ascontiguousarray(other[lo:lo + 1250]), at_b)
        assert np.all(engine.iq_download(n_a, 0) == fresh)
        v_b = cases.reference(dc.IN_R16, 17, 3, cfg_b.fcw, cfg_b.gain, n)
        assert at_b - 4096 == v_b.size
        check_ring(engine.iq_download(v_b.size, 4096), v_b, cfg_b, ring_fmt, cases.max_abs(dc.IN_R16, other), "second converter")
    finally:
        engine.ddc_destroy(a)
        engine.ddc_destroy(b)


# ------------------------------------------------------------------------------------------------ 5. push_queue
@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page_locked"])
def test_push_queue_equals_push(engine, page_locked):
    in_fmt, ring_fmt, n = dc.IN_R16, FMT_CI16, 30001
    raw = cases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, 33, 2, cases.FCWS["odd"], cases.GOLD)
    engine.iq_alloc(16384, ring_fmt)
    ddc = engine.ddc_create(cfg)
    block = engine.host_alloc(n, np.int16) if page_locked else None
    try:
        n_out = engine.ddc_push(ddc, raw, 0)
        want = engine.iq_download(n_out, 0)
        engine.iq_upload(np.zeros(2 * 16384, dtype=np.int16), 0)
        engine.ddc_reset(ddc)
        src = block if page_locked else raw.copy()
        src[:] = raw
        at = 0
        for lo in range(0, n, 7001):                      # several pushes in flight behind each other, no wait between them
            at += engine.ddc_push_queue(ddc, src[lo:lo + 7001], at)
        engine.sync()
        assert at == n_out
        assert np.array_equal(engine.iq_download(n_out, 0), want)
    finally:
        engine.ddc_destroy(ddc)
        if block is not None:
            engine.host_free(block)


# ------------------------------------------------------------------------------------------------ 6. refusals
def _status(fn):
    with pytest.raises(SdrError) as err:
        fn()
    return err.value.status


def _create_raw(engine, in_fmt=0, D=1, taps=(1.0,), n_taps=None, flags=0, gain=1.0):
    t = (C.c_double * max(len(taps), 1))(*taps)
    cfg = _lib.DdcCfg(in_fmt, D, len(taps) if n_taps is None else n_taps, flags, 0, gain, C.cast(t, C.POINTER(C.c_double)))
    h = C.c_void_p()
    rc = _lib.load().sdr_ddc_create(engine._h, C.byref(cfg), C.byref(h))
    if rc == 0:
        _lib.load().sdr_ddc_destroy(engine._h, h)
    return rc, h.value


def test_refusals_leave_the_ring_as_it_was(engine):
    cap = 1024
    engine.iq_alloc(cap, FMT_CI16)
    pattern = np.random.default_rng(cases.SEED + 6).integers(-3000, 3000, 2 * cap).astype(np.int16)
    engine.iq_upload(pattern, 0)
    for kw in (dict(D=0), dict(D=65), dict(D=-1), dict(n_taps=0), dict(taps=(0.001,) * 513), dict(taps=(1.0, float("nan"))),
               dict(taps=(float("inf"),)), dict(gain=float("nan")), dict(gain=float("-inf")), dict(in_fmt=4), dict(in_fmt=-1),
               dict(flags=1)):
        rc, handle = _create_raw(engine, **kw)
        assert rc == INVALID and not handle, kw
    assert _create_raw(engine, D=64, taps=(0.001,) * 512)[0] == 0
    ddc = engine.ddc_create(cases.config(dc.IN_R8, 3, 2, 0, 1.0))
    raw = cases.stream(dc.IN_R8, 5000)
    try:
        assert _status(lambda: engine.ddc_push(ddc, raw, 0)) == RANGE                  # 2500 outputs, a ring of 1024
        assert _status(lambda: engine.ddc_push(ddc, raw[:100].copy(), cap)) == RANGE
        assert _status(lambda: engine.ddc_push(ddc, raw[:100].copy(), -1)) == RANGE
        assert _status(lambda: engine.ddc_push_queue(ddc, raw, 0)) == RANGE
        assert engine.ddc_out_count(ddc, 5000) == 2500                                # (a refused push has not advanced the converter)
        assert engine.ddc_push(ddc, raw[:0].copy(), 0) == 0                           # n_in = 0 succeeds and writes nothing
        assert np.array_equal(engine.iq_download(cap, 0), pattern)
    finally:
        engine.ddc_destroy(ddc)
    bare = Engine(0)                                                                   # no ring allocated
    try:
        ddc = bare.ddc_create(cases.config(dc.IN_R8, 3, 2, 0, 1.0))
        assert _status(lambda: bare.ddc_push(ddc, raw[:100].copy(), 0)) == STATE
        bare.ddc_destroy(ddc)
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------ 7. pass-through
@pytest.mark.parametrize("in_fmt,ring_fmt", [(dc.IN_R8, FMT_CI8), (dc.IN_R16, FMT_CI16)])
def test_pass_through_of_a_real_recording_equals_an_upload_of_r_0(engine, in_fmt, ring_fmt):
    n, cap = 10007, 16384
    rng = np.random.default_rng(cases.SEED + 7)
    lim = 127 if in_fmt == dc.IN_R8 else 32767
    raw = rng.integers(-lim, lim + 1, n).astype(dc.input_dtype(in_fmt))
    pair = np.zeros(2 * n, dtype=raw.dtype)
    pair[0::2] = raw
    engine.iq_alloc(cap, ring_fmt)
    engine.iq_upload(pair, 5)
    want = engine.iq_download(cap, 0)
    engine.iq_alloc(cap, ring_fmt)
    ddc = engine.ddc_create(dc.DownConverterConfig(in_fmt))
    try:
        assert engine.ddc_push(ddc, raw, 5) == n
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(engine.iq_download(cap, 0), want)


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_search_and_receiver_over_the_converted_real_recording(engine, tmp_path):
    """The 60 ms real int8 recording of tests/test_downconvert.py (8.184 MHz, IF 2.046 MHz, one C/A satellite) through the
    device's converter: sdr_pcps on the converted ring finds what the oracle finds on the statement's output -- peak sample,
    bin, ratio to 1e-12 --, and a ChannelManager over the real file hands out the packets of a manager over the statement's
    output stored as an ordinary complex int8 recording, bit for bit."""
    from oracle import sydr_oracle as orc
    import packed_cases
    sig, conv_sig, converted = cases.write_real_and_converted(tmp_path)
    raw, ms, fs, prn = cases.real_if_recording(), cases.REAL_MS, cases.FS_REAL / 2, cases.SATELLITE["prn"]
    n = orc.samples_per_code(fs)
    engine.iq_alloc(ms * n, FMT_CI8)
    ddc = engine.ddc_create(sig.frontEnd.config)
    try:
        assert engine.ddc_push(ddc, raw, 0) == ms * n
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(engine.iq_download(ms * n, 0), converted)
    engine.code_slots(1)
    engine.load_gps_code(0, prn)
    pb, pc, pr, _ = engine.pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)
    rf = orc.iq_to_complex(converted[:2 * n].astype(np.float64)).reshape(1, -1)
    cmap = orc.pcps_map(rf, 0.0, fs, orc.code_spectrum(orc.gold_code(prn), fs), 5000.0, 250.0, n)
    peak, ratio = orc.two_peak_compare(cmap, n, round(fs / orc.CODE_RATE))
    assert [int(pb[0]), int(pc[0])] == peak and abs(pr[0] - ratio) <= 1e-12 * ratio, (pb, pc, pr, peak, ratio)
    cfg = packed_cases.kaplan_config()
    got, mgr = packed_cases.receive(sig, engine, prns=[prn], cfg=cfg, ms=ms, mode="ticks")
    ring_fmt, ring_size = mgr.sharedBuffer.fmt, mgr.sharedBuffer.maxSize
    mgr.close()
    want, want_mgr = packed_cases.receive(conv_sig, engine, prns=[prn], cfg=cfg, ms=ms, mode="ticks")
    want_mgr.close()
    assert ring_fmt == FMT_CI8 and ring_size == 100 * n
    assert len(got) == len(want) == ms
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, k
    assert packed_cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 1 and packed_cases.count(got) > 40
