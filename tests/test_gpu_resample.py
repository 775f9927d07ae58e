"""The device's rational resampler (sdr_ddc_create_rational, sydr_amd/csrc/resample.hip) against its NumPy statement
(sydr_amd/signal/downconvert.py with `interpolation`): what the ring holds after a push, however the stream was cut into
pushes, wherever the window lies in the ring; interpolation = 1 against sdr_ddc_create; with a mitigator; the refusals; and
everything downstream of the ring over a 16.368 MHz recording converted to 12 MHz.

Tolerance (derived, not measured): B = (Tp + 16) * 2^-53 * max_p sum_k |h[p + k L]| * max|x|, Tp = ceil(T / L), is what any order
of a phase's fp64 products and sums keeps, plus a few ulp for the phasor.  cf64 rings: |ring - v| <= gain * B, and exactly equal
where the phasor is exact (fcw zero or fs / 4: the device forms the statement's products in the statement's order); cf32 rings:
+ 2^-24 * |v|; integer rings: the test first asserts that NO component of the statement lies within gain * B of a half-integer,
then demands byte equality."""
import ctypes as C

import numpy as np
import pytest

import downconvert_cases as dcases
import mitigate_cases as mcases
import resample_cases as cases

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI8, FMT_CI16
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt
from sydr_amd.utils.enumerations import ChannelMessage

pytestmark = pytest.mark.gpu

INVALID, RANGE = -1, -5
IN_NAMES, RING_NAMES = dcases.IN_NAMES, dcases.RING_NAMES


def ring_capacity(n_out: int) -> int:
    return -(-(n_out + 8) // 8) * 8


def per_sample(in_fmt: int) -> int:
    return 2 if dc.input_is_complex(in_fmt) else 1


def check_ring(got: np.ndarray, v: np.ndarray, cfg, ring_fmt: int, x_max: float, what, exact: bool = False) -> float:
    """`got`: the downloaded window (interleaved, the ring's type); v: the statement's outputs.  exact: a cf64 ring has to equal
    the statement (the phasor is exact).  -> the worst error as a fraction of the bound (integer rings: 0, they are equal)."""
    band = dc.tolerance(cfg, x_max)
    if ring_fmt in (FMT_CI8, FMT_CI16):
        assert dc.ambiguous(v, band) == 0, ("statement output near a rounding tie", what)
        want = dc.quantise(v, ring_fmt)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])
        return 0.0
    pair = dc.quantise(v, FMT_CF64)
    err = np.abs(got.astype(np.float64) - pair)
    bound = band + (2.0 ** -24 * np.abs(pair) if ring_fmt == FMT_CF32 else 0.0)
    worst = int(np.argmax(err - bound))
    ratio = float(np.max(err / bound))
    print(f"{what}: max |ring - v| = {err.max():.3e}, bound {band:.3e}, worst fraction of the bound {ratio:.3g}")
    assert np.all(err <= bound), (what, worst, err[worst], band)
    if exact and ring_fmt == FMT_CF64:
        assert got.tobytes() == pair.tobytes(), (what, "an exact phasor, yet the ring differs from the statement")
    return ratio


def run_case(engine, shape, in_fmt, ring_fmt):
    """One push of the shared stream through (L, M, T) for every frequency word -> the worst fraction of the bound."""
    L, M, T = shape
    raw = dcases.stream(in_fmt)
    x_max = dcases.max_abs(in_fmt, raw)
    n_out = dc.out_count(0, cases.N_INPUTS, M, L)
    engine.iq_alloc(ring_capacity(n_out), ring_fmt)
    worst = 0.0
    for name, fcw in cases.FCWS.items():
        gain = dcases.gain_for(in_fmt, ring_fmt)
        cfg = cases.config(in_fmt, L, M, T, fcw, gain)
        v = cases.reference(in_fmt, L, M, T, fcw, gain)
        ddc = engine.ddc_create(cfg)
        try:
            assert engine.ddc_out_count(ddc, cases.N_INPUTS) == n_out == v.size
            assert engine.ddc_push(ddc, raw, 0) == n_out
        finally:
            engine.ddc_destroy(ddc)
        what = (IN_NAMES[in_fmt], RING_NAMES[ring_fmt], L, M, T, name)
        worst = max(worst, check_ring(engine.iq_download(n_out, 0), v, cfg, ring_fmt, x_max, what, exact=name in ("zero", "quarter")))
    return worst


# ------------------------------------------------------------------------------------------------ 1. ring equals statement
@pytest.mark.parametrize("shape", cases.SMALL, ids=cases.shape_id)
@pytest.mark.parametrize("ring_fmt", dcases.RING_FORMATS, ids=lambda f: "ring_" + RING_NAMES[f])
@pytest.mark.parametrize("in_fmt", dcases.IN_FORMATS, ids=lambda f: "in_" + IN_NAMES[f])
def test_ring_equals_the_statement(engine, in_fmt, ring_fmt, shape):
    print(f"worst fraction of the bound over the case: {run_case(engine, shape, in_fmt, ring_fmt):.3g}")


@pytest.mark.parametrize("ring_fmt", [FMT_CI16, FMT_CF64], ids=lambda f: "ring_" + RING_NAMES[f])
@pytest.mark.parametrize("shape", cases.EDGES, ids=cases.shape_id)
def test_ring_equals_the_statement_at_the_ends_of_the_domain(engine, shape, ring_fmt):
    """L = 1024 with two taps per phase; M = 64 L; the longest prototype with Tp = 512 (4.5 million outputs)."""
    print(f"worst fraction of the bound over the case: {run_case(engine, shape, dc.IN_CI16, ring_fmt):.3g}")


# ------------------------------------------------------------------------------------------------ 2. interpolation = 1
@pytest.mark.parametrize("T,D", [(33, 2), (3, 64)])
def test_interpolation_one_is_sdr_ddc_create(engine, T, D):
    in_fmt, n = dc.IN_CI8, cases.N_INPUTS
    raw = dcases.stream(in_fmt)
    lib = _lib.load()
    for ring_fmt in (FMT_CF64, FMT_CI8):
        cfg = dcases.config(in_fmt, T, D, cases.FCWS["odd"], dcases.gain_for(in_fmt, ring_fmt))
        n_out = dc.out_count(0, n, D)
        engine.iq_alloc(ring_capacity(n_out), ring_fmt)
        plain = engine.ddc_create(cfg)
        try:
            assert engine.ddc_push(plain, raw, 0) == n_out
        finally:
            engine.ddc_destroy(plain)
        want = engine.iq_download(engine.iq_capacity, 0)
        engine.iq_upload(np.zeros(2 * engine.iq_capacity, dtype=want.dtype), 0)
        taps = np.ascontiguousarray(cfg.taps)
        c = _lib.DdcCfg(in_fmt, D, T, 0, cfg.fcw, cfg.gain, taps.ctypes.data_as(C.POINTER(C.c_double)))
        h = C.c_void_p()
        assert lib.sdr_ddc_create_rational(engine._h, C.byref(c), 1, C.byref(h)) == 0 and h.value
        try:
            n_got = C.c_int64(0)
            engine.prof_enable(True)
            engine.prof_reset()
            assert lib.sdr_ddc_out_count(h, n) == n_out
            assert lib.sdr_ddc_push(engine._h, h, raw.ctypes.data, n, 0, C.byref(n_got)) == 0 and n_got.value == n_out
            scopes = {name: engine.prof_read(name)[1] for name in ("ddc_kernel", "ddc_history_kernel", "resample_kernel")}
        finally:
            engine.prof_enable(False)
            lib.sdr_ddc_destroy(engine._h, h)
        assert scopes == dict(ddc_kernel=1, ddc_history_kernel=1, resample_kernel=0), scopes
        assert engine.iq_download(engine.iq_capacity, 0).tobytes() == want.tobytes()
    # ... and the resampler's own scopes with L > 1
    cfg = cases.config(in_fmt, 3, 2, 7, 0, 1.0)
    engine.iq_alloc(ring_capacity(dc.out_count(0, n, 2, 3)), FMT_CI8)
    ddc = engine.ddc_create(cfg)
    try:
        engine.prof_enable(True)
        engine.prof_reset()
        engine.ddc_push(ddc, raw, 0)
        scopes = {name: engine.prof_read(name)[1] for name in ("ddc_kernel", "ddc_history_kernel", "resample_kernel")}
        engine.prof_enable(True, calls_only=True)
        engine.prof_reset()
        engine.ddc_push(ddc, raw, 0)
        assert engine.prof_read("call_ddc_push")[1] == 1
    finally:
        engine.prof_enable(False)
        engine.ddc_destroy(ddc)
    assert scopes == dict(ddc_kernel=0, ddc_history_kernel=1, resample_kernel=1), scopes       # (the history kernel is shared)


# ------------------------------------------------------------------------------------------------ 3. chunk invariance
@pytest.mark.parametrize("in_fmt,ring_fmt", [(dc.IN_CI8, FMT_CF64), (dc.IN_R16, FMT_CF64), (dc.IN_CI16, FMT_CI16), (dc.IN_R8, FMT_CF32)],
                         ids=lambda f: str(f))
@pytest.mark.parametrize("shape", [(5, 4, 43), (250, 341, 1500)], ids=cases.shape_id)
def test_the_ring_does_not_depend_on_how_the_stream_was_cut(engine, shape, in_fmt, ring_fmt):
    L, M, T = shape
    n = 20001
    raw = dcases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, L, M, T, cases.FCWS["odd"], dcases.gain_for(in_fmt, ring_fmt))
    total = dc.out_count(0, n, M, L)
    engine.iq_alloc(ring_capacity(total), ring_fmt)
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == total
        whole = engine.iq_download(total, 0)
        engine.iq_upload(np.zeros(2 * engine.iq_capacity, dtype=whole.dtype), 0)
        engine.ddc_reset(ddc)
        st = dc.Statement(cfg)
        at = 0
        for piece in dcases.cut(raw, in_fmt, cases.push_lengths(cfg.phase_taps)):
            n_in = piece.size // per_sample(in_fmt)
            want = st.out_count(n_in)
            assert engine.ddc_out_count(ddc, n_in) == want                       # sdr_ddc_out_count before each push equals *n_out
            assert engine.ddc_push(ddc, np.ascontiguousarray(piece), at) == want == st.push(piece).size
            at += want
        assert at == total
        pieces = engine.iq_download(total, 0)
    finally:
        engine.ddc_destroy(ddc)
    assert np.all(pieces == whole), np.flatnonzero(pieces != whole)[:8]
    check_ring(whole, cases.reference(in_fmt, L, M, T, cfg.fcw, cfg.gain, n), cfg, ring_fmt, dcases.max_abs(in_fmt, raw), "one push")


# ------------------------------------------------------------------------------------------------ 4. a window across the ring's end
@pytest.mark.parametrize("ring_fmt", dcases.RING_FORMATS, ids=lambda f: "ring_" + RING_NAMES[f])
def test_a_window_across_the_rings_end_and_nothing_outside_it(engine, ring_fmt):
    in_fmt, (L, M, T), cap, n = dc.IN_R8, (5, 4, 43), 8192, 6001
    raw = dcases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, L, M, T, cases.FCWS["quarter"], dcases.gain_for(in_fmt, ring_fmt))
    v = cases.reference(in_fmt, L, M, T, cfg.fcw, cfg.gain, n)
    rng = np.random.default_rng(cases.SEED + 3)
    pattern = rng.integers(-100, 101, 2 * cap).astype(dcases.RING_DTYPE[ring_fmt])
    engine.iq_alloc(cap, ring_fmt)
    engine.iq_upload(pattern, 0)
    off = cap - 1000
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, raw, off) == v.size == 7502
    finally:
        engine.ddc_destroy(ddc)
    ring = engine.iq_download(cap, 0)
    inside = (2 * off + np.arange(2 * v.size)) % (2 * cap)
    outside = np.ones(2 * cap, dtype=bool)
    outside[inside] = False
    assert outside.sum() == 2 * (cap - v.size)
    assert np.array_equal(ring[outside].view(np.uint8), pattern[outside].view(np.uint8))
    check_ring(ring[inside], v, cfg, ring_fmt, dcases.max_abs(in_fmt, raw), "across the end", exact=True)


# ------------------------------------------------------------------------------------------------ 5. reset, two converters
def test_reset_and_a_rational_beside_an_integer_converter(engine):
    in_fmt, ring_fmt, n = dc.IN_CI8, FMT_CF64, 5000
    raw, other = dcases.stream(in_fmt, n), dcases.stream(dc.IN_R16, n)
    cfg = cases.config(in_fmt, 5, 4, 43, cases.FCWS["odd"], dcases.GOLD)
    cfg_b = dcases.config(dc.IN_R16, 17, 3, cases.FCWS["quarter"], dcases.GOLD)
    engine.iq_alloc(16384, ring_fmt)
    a, b = engine.ddc_create(cfg), engine.ddc_create(cfg_b)
    try:
        n_a = engine.ddc_push(a, raw, 0)
        assert n_a == 6250
        fresh = engine.iq_download(n_a, 0)
        engine.ddc_push(a, raw[:2 * 777], 0)             # (more history, another index, another phase)
        engine.ddc_reset(a)
        assert engine.ddc_out_count(a, n) == n_a
        assert engine.ddc_push(a, raw, 0) == n_a
        assert np.all(engine.iq_download(n_a, 0) == fresh)
        # a and b interleaved, push by push, each into its own half of the ring: what each leaves is its own stream's statement
        engine.ddc_reset(a)
        at_a, at_b = 0, 8192
        for lo in range(0, n, 1250):
            at_a += engine.ddc_push(a, np.ascontiguousarray(raw[2 * lo:2 * (lo + 1250)]), at_a)
            at_b += engine.ddc_push(b, np.ascontiguousarray(other[lo:lo + 1250]), at_b)
        assert at_a == n_a and np.all(engine.iq_download(n_a, 0) == fresh)
        check_ring(fresh, cases.reference(in_fmt, 5, 4, 43, cfg.fcw, cfg.gain, n), cfg, ring_fmt, dcases.max_abs(in_fmt, raw), "rational converter")
        v_b = dcases.reference(dc.IN_R16, 17, 3, cfg_b.fcw, cfg_b.gain, n)
        assert at_b - 8192 == v_b.size
        got_b = engine.iq_download(v_b.size, 8192)
        assert got_b.tobytes() == dc.quantise(v_b, FMT_CF64).tobytes()            # (fs / 4: the integer converter is exact there)
    finally:
        engine.ddc_destroy(a)
        engine.ddc_destroy(b)


# ------------------------------------------------------------------------------------------------ 6. push_queue
@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page_locked"])
def test_push_queue_equals_push(engine, page_locked):
    in_fmt, ring_fmt, n = dc.IN_R16, FMT_CI16, 30001
    raw = dcases.stream(in_fmt, n)
    cfg = cases.config(in_fmt, 250, 341, 1500, cases.FCWS["odd"], dcases.GOLD)
    engine.iq_alloc(32768, ring_fmt)
    ddc = engine.ddc_create(cfg)
    block = engine.host_alloc(n, np.int16) if page_locked else None
    try:
        n_out = engine.ddc_push(ddc, raw, 0)
        assert n_out == dc.out_count(0, n, 341, 250)
        want = engine.iq_download(n_out, 0)
        engine.iq_upload(np.zeros(2 * 32768, dtype=np.int16), 0)
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


# ------------------------------------------------------------------------------------------------ 7. with a mitigator
MIT_SHAPE, MIT_NFFT = (3, 2, 49), 256


@pytest.mark.parametrize("ring_fmt", dcases.RING_FORMATS, ids=lambda f: "ring_" + RING_NAMES[f])
def test_with_a_blanker_and_an_excisor(engine, ring_fmt):
    """A blanker and a 256-point excisor on the stream v_m of a (3, 2, 49) resampler: counters and integer rings equal
    mitigate.Statement over the rational statement's output, float rings within the mitigator's derived bound
    (mitigate_cases.tolerance), and neither depends on how the stream was cut."""
    L, M, T = MIT_SHAPE
    raw = mcases.jammed()
    n = mcases.N_INPUTS
    gain = dcases.gain_for(dc.IN_CI8, ring_fmt)
    ddc_cfg = cases.config(dc.IN_CI8, L, M, T, cases.FCWS["odd"], gain)
    v = dc.statement(ddc_cfg, [raw])
    cfg = mcases.settings(v, MIT_NFFT, "both", gain)
    st = mt.Statement(cfg)
    y = st.push(v)
    band = mcases.tolerance(cfg, ddc_cfg, v, raw)
    mcases.assert_unambiguous(cfg, v, y, band, ring_fmt in (FMT_CI8, FMT_CI16), RING_NAMES[ring_fmt])
    n_out = dc.out_count(0, n, M, L)
    assert st.stats.n_outputs == n_out == y.size and st.stats.n_triggers > 0 and st.stats.n_bins_excised > 0
    engine.iq_alloc(ring_capacity(n_out), ring_fmt)
    ddc = engine.ddc_create(ddc_cfg)
    try:
        engine.ddc_mitigate(ddc, cfg)
        assert engine.ddc_delay(ddc) == cfg.delay
        assert engine.ddc_out_count(ddc, n) == n_out
        assert engine.ddc_push(ddc, raw, 0) == n_out
        whole, whole_stats = engine.iq_download(n_out, 0), engine.ddc_mitigation_stats(ddc)
        engine.iq_upload(np.zeros(2 * engine.iq_capacity, dtype=whole.dtype), 0)
        engine.ddc_reset(ddc)
        at = 0
        for piece in mcases.cut(raw, mcases.push_lengths(MIT_NFFT), 2):
            want = engine.ddc_out_count(ddc, piece.size // 2)
            assert engine.ddc_push(ddc, np.ascontiguousarray(piece), at) == want
            at += want
        assert at == n_out
        pieces, pieces_stats = engine.iq_download(n_out, 0), engine.ddc_mitigation_stats(ddc)
    finally:
        engine.ddc_destroy(ddc)
    assert whole_stats == st.stats, (whole_stats, st.stats)
    assert pieces_stats == whole_stats and np.all(pieces == whole)
    if ring_fmt in (FMT_CI8, FMT_CI16):
        want = dc.quantise(y, ring_fmt)
        assert np.array_equal(whole, want), np.flatnonzero(whole != want)[:8]
    else:
        pair = dc.quantise(y, FMT_CF64)
        err = np.abs(whole.astype(np.float64) - pair)
        bound = band + (2.0 ** -24 * np.abs(pair) if ring_fmt == FMT_CF32 else 0.0)
        print(f"max |ring - y| = {err.max():.3e}, tolerance {band:.3e}, worst fraction {float(np.max(err / bound)):.3g}")
        assert np.all(err <= bound)


# ------------------------------------------------------------------------------------------------ 8. refusals
def _status(fn):
    with pytest.raises(SdrError) as err:
        fn()
    return err.value.status


def _create_raw(engine, L, in_fmt=2, M=1, taps=(1.0,), n_taps=None, flags=0, gain=1.0, null_taps=False):
    t = (C.c_double * max(len(taps), 1))(*taps)
    cfg = _lib.DdcCfg(in_fmt, M, len(taps) if n_taps is None else n_taps, flags, 0, gain, None if null_taps else C.cast(t, C.POINTER(C.c_double)))
    h = C.c_void_p()
    rc = _lib.load().sdr_ddc_create_rational(engine._h, C.byref(cfg), L, C.byref(h))
    if rc == 0:
        _lib.load().sdr_ddc_destroy(engine._h, h)
    return rc, h.value


def test_refusals_leave_the_ring_and_the_converter_as_they_were(engine):
    cap = 2048
    engine.iq_alloc(cap, FMT_CI16)
    pattern = np.random.default_rng(cases.SEED + 6).integers(-3000, 3000, 2 * cap).astype(np.int16)
    engine.iq_upload(pattern, 0)
    small = (0.001,)
    for kw in (dict(L=0), dict(L=-1), dict(L=1025), dict(L=2, M=0), dict(L=2, M=-4), dict(L=1024, M=1025), dict(L=2, M=129),       # M > 64 L
               dict(L=2, n_taps=0), dict(L=1024, taps=small * 32769), dict(L=63, taps=small * (63 * 512 + 1)),                       # Tp = 513
               dict(L=2, taps=(1.0, float("nan"))), dict(L=2, taps=(float("inf"),)), dict(L=2, gain=float("nan")), dict(L=2, in_fmt=4),
               dict(L=2, in_fmt=-1), dict(L=2, flags=1), dict(L=2, null_taps=True),
               dict(L=1, M=65), dict(L=1, taps=small * 513)):                                                                        # L = 1: sdr_ddc_create's limits
        rc, handle = _create_raw(engine, **kw)
        assert rc == INVALID and not handle, kw
    lib = _lib.load()
    assert lib.sdr_ddc_create_rational(engine._h, None, 2, C.byref(C.c_void_p())) == INVALID
    for kw in (dict(L=1024, M=1024, taps=small * 2048), dict(L=16, M=1024, taps=small * 512), dict(L=64, taps=small * 32768),
               dict(L=63, taps=small * (63 * 512)), dict(L=1, M=64, taps=small * 512)):
        assert _create_raw(engine, **kw)[0] == 0, kw
    cfg = cases.config(dc.IN_R8, 3, 2, 7, 0, dcases.GOLD * 24.0)
    ddc = engine.ddc_create(cfg)
    raw = dcases.stream(dc.IN_R8, 5000)
    try:
        assert engine.ddc_push(ddc, raw[:1000].copy(), 0) == 1500                                # (the converter has a history and an index)
        before = engine.iq_download(cap, 0)
        assert _status(lambda: engine.ddc_push(ddc, raw, 0)) == RANGE                            # 7500 outputs, a ring of 2048
        assert _status(lambda: engine.ddc_push(ddc, raw[:100].copy(), cap)) == RANGE
        assert _status(lambda: engine.ddc_push(ddc, raw[:100].copy(), -1)) == RANGE
        assert _status(lambda: engine.ddc_push_queue(ddc, raw, 0)) == RANGE
        # (N + n_in) * L at 2^62: refused in host arithmetic before anything is copied (the pointer is never read)
        huge, n_got = (1 << 62) // 3, C.c_int64(-7)
        assert lib.sdr_ddc_push(engine._h, ddc.handle, raw.ctypes.data, huge, 0, C.byref(n_got)) == RANGE and n_got.value == -7
        assert lib.sdr_ddc_out_count(ddc.handle, huge) == RANGE
        assert lib.sdr_ddc_push(engine._h, ddc.handle, raw.ctypes.data, -1, 0, None) == INVALID
        assert lib.sdr_ddc_push(engine._h, ddc.handle, None, 10, 0, None) == INVALID
        assert engine.ddc_push(ddc, raw[:0].copy(), 0) == 0                                      # n_in = 0 succeeds and writes nothing
        assert np.array_equal(engine.iq_download(cap, 0), before)
        # the converter is where it was: the next push continues the stream
        assert engine.ddc_out_count(ddc, 1001) == dc.out_count(1000, 1001, 2, 3) == 1502
        assert engine.ddc_push(ddc, raw[1000:1200].copy(), 0) == 300
        v = dc.statement(cfg, [raw[:1200]])
        check_ring(engine.iq_download(300, 0), v[1500:], cfg, FMT_CI16, dcases.max_abs(dc.IN_R8, raw), "after the refusals")
        assert np.array_equal(engine.iq_download(cap - 300, 300), before[2 * 300:])
    finally:
        engine.ddc_destroy(ddc)


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_search_and_receiver_over_a_16368_kHz_recording_at_12_MHz(engine, tmp_path):
    """A 60 ms complex int8 recording at 16.368 MHz with one C/A satellite, through the device's resampler (250 / 341, the
    default prototype of 5457 taps, gain 2) into a 12 MHz ring: the ring equals the statement; sdr_pcps on it finds what the
    oracle finds on the statement's output -- peak sample, bin, ratio to 1e-12 --, the satellite sits where it was synthesised
    plus the group delay (T - 1) / (2 M) = 8 output samples; and a ChannelManager over the 16.368 MHz file with the key hands out
    the packets of a manager over the statement's output stored as an ordinary complex int8 recording at 12 MHz, bit for bit."""
    from oracle import sydr_oracle as orc
    import packed_cases
    sig, conv_sig, converted = cases.write_recording_and_converted(tmp_path)
    raw, ms, fs, prn = cases.recording(), cases.REC_MS, cases.FS_RING, cases.SATELLITE["prn"]
    n = orc.samples_per_code(fs)
    assert n == 12000 and sig.samplesPerMs == n and converted.size == 2 * ms * n
    fe_cfg = sig.frontEnd.config
    assert dc.ambiguous(dc.statement(fe_cfg, [raw]), dc.tolerance(fe_cfg, dcases.max_abs(dc.IN_CI8, raw))) == 0
    engine.iq_alloc(ms * n, FMT_CI8)
    ddc = engine.ddc_create(fe_cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == ms * n
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(engine.iq_download(ms * n, 0), converted)
    engine.code_slots(1)
    engine.load_gps_code(0, prn)
    pb, pc, pr, _ = engine.pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)
    code = orc.gold_code(prn)
    rf = orc.iq_to_complex(converted[:2 * n].astype(np.float64)).reshape(1, -1)
    cmap = orc.pcps_map(rf, 0.0, fs, orc.code_spectrum(code, fs), 5000.0, 250.0, n)
    peak, ratio = orc.two_peak_compare(cmap, n, round(fs / orc.CODE_RATE))
    assert [int(pb[0]), int(pc[0])] == peak and abs(pr[0] - ratio) <= 1e-12 * ratio, (pb, pc, pr, peak, ratio)
    # where the satellite was synthesised: the same satellite synthesised at the ring's rate, plus the group delay
    delay = (fe_cfg.n_taps - 1) / (2.0 * cases.REC_M)
    assert delay == 8.0 == sig.frontEnd.groupDelay * cases.REC_L / cases.REC_M
    direct = orc.iq_to_complex(orc.synth_iq(fs, n, [cases.SATELLITE], 0.0, 1).astype(np.float64)).reshape(1, -1)
    peak0, _ = orc.two_peak_compare(orc.pcps_map(direct, 0.0, fs, orc.code_spectrum(code, fs), 5000.0, 250.0, n), n, round(fs / orc.CODE_RATE))
    assert peak[0] == peak0[0] and abs(peak[1] - (peak0[1] + delay)) <= 1 and ratio > 3.0, (peak, peak0, ratio)
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
