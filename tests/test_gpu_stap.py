"""Space-time weights of the device's array down-converter (sdr_ddc_create_stap: T frames of K elements combined where ddc_kernel /
resample_kernel load their inputs, the raw tail carried across pushes; sdr_ddc_stap_weights; sdr_ddc_stap_covariance).

Against existing code paths every comparison demands equal ring bytes: T = 1 against the array converter, a unit weight at tap t0
against the layout's converter on the stream with t0 zero frames prepended.  Against the NumPy statement
(sydr_amd/signal/stap.py) general weights are held bit for bit with fcw = 0 and within the converter's own derived bound
(`check_ring`, evaluated with the combined inputs) with a mixer.  The lag covariance of integer fields equals the statement's;
of float32 fields it lies within 2 n 2^-52 sum(|..| + |..|) per lag."""
import ctypes as C

import numpy as np
import pytest

import array_cases as cases
import downconvert_cases as dcases
import ddc_layout_cases as lcases
import stap_cases as scases
from test_gpu_downconvert import check_ring

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI8, FMT_CI16
from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt
from sydr_amd.signal import stap
from sydr_amd.utils.enumerations import ChannelMessage

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -6
CAPACITY = lcases.ring_capacity(2 * cases.N_FRAMES)
RINGS = dcases.RING_FORMATS
SCOPES = ("ddc_kernel", "resample_kernel", "ddc_history_kernel", "ddc_array_cov_kernel", "ddc_stap_cov_kernel", "call_ddc_push")


def push_all(engine, cfg, raw, n_out):
    return lcases.push_all(engine, cfg, raw, n_out)


def assert_same_bytes(got, want, what):
    bad = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (what, bad.size, bad[:5])
    assert np.any(want != 0), what


def geometry_of(name, msb=False):
    return (cases.packed_layout(name, msb), cases.PACKED[name][3]) if name in cases.PACKED else cases.GEOMETRIES[name]


# ------------------------------------------------------------------------------------------------ 1. launch identity
@pytest.mark.parametrize("name", list(cases.GEOMETRIES))
def test_one_tap_gives_the_ring_of_the_array_converter(engine, name):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    w = cases.general_weights(K)
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        gain = cases.gain_for(layout, ring_fmt, K)
        for shape in cases.SHAPES:
            n_out = lcases.out_total(shape, cases.N_FRAMES)
            got = push_all(engine, cases.config(shape, cases.FCWS["odd"], gain, layout, scases.geometry(lanes, 1, w.reshape(1, K))), raw, n_out)
            want = push_all(engine, cases.config(shape, cases.FCWS["odd"], gain, layout, ar.ArrayGeometry(lanes, w)), raw, n_out)
            assert_same_bytes(got, want, (dcases.RING_NAMES[ring_fmt], shape))


def test_converters_of_the_older_constructors_make_the_launches_they_made(engine):
    """sdr_prof_read launch counts of one push: a converter of sdr_ddc_create, _rational, _layout and _array makes one converter
    kernel, one history kernel (none without a filter), with MEASURE one "ddc_array_cov_kernel" pass and never a
    "ddc_stap_cov_kernel" one; a space-time converter makes the converter kernel, the history kernel -- for its raw tail also
    without a filter when T > 1 -- and with MEASURE one lag pass under its own scope."""
    layout, lanes = cases.GEOMETRIES["K3_int8_complex"]
    raw = cases.stream(layout)
    plain = cases.combined_integers(raw, layout, lanes, cases.quarter_weights(3))
    engine.iq_alloc(CAPACITY, FMT_CI16)
    element = ar.element_layout(layout, 2)
    # (cfg, data, converter kernel, history launches, array passes, lag passes)
    made = [(cases.config((33, 2), 0, 1.0), plain, "ddc_kernel", 1, 0, 0), (cases.config((1, 1), 0, 1.0), plain, "ddc_kernel", 0, 0, 0),
            (cases.config((3, 2, 7), 0, 1.0), plain, "resample_kernel", 1, 0, 0),
            (cases.config((33, 2), 0, 1.0, element), raw, "ddc_kernel", 1, 0, 0), (cases.config((3, 2, 7), 0, 1.0, element), raw, "resample_kernel", 1, 0, 0),
            (cases.config((33, 2), 0, 1.0, layout, ar.ArrayGeometry(lanes)), raw, "ddc_kernel", 1, 0, 0),
            (cases.config((1, 1), 0, 1.0, layout, ar.ArrayGeometry(lanes, measure=True)), raw, "ddc_kernel", 0, 1, 0),
            (cases.config((3, 2, 7), 0, 1.0, layout, ar.ArrayGeometry(lanes, measure=True)), raw, "resample_kernel", 1, 1, 0),
            (cases.config((33, 2), 0, 1.0, layout, scases.geometry(lanes, 1)), raw, "ddc_kernel", 1, 0, 0),
            (cases.config((1, 1), 0, 1.0, layout, scases.geometry(lanes, 1)), raw, "ddc_kernel", 0, 0, 0),
            (cases.config((1, 1), 0, 1.0, layout, scases.geometry(lanes, 5, measure=True)), raw, "ddc_kernel", 1, 0, 1),
            (cases.config((3, 2, 7), 0, 1.0, layout, scases.geometry(lanes, 8, measure=True)), raw, "resample_kernel", 1, 0, 1)]
    engine.prof_enable(True)
    try:
        for cfg, data, kernel, hist, cov, lag in made:
            ddc = engine.ddc_create(cfg)
            try:
                engine.prof_reset()
                engine.ddc_push(ddc, data, 0)
                engine.sync()
                counts = {name: engine.prof_read(name)[1] for name in SCOPES}
            finally:
                engine.ddc_destroy(ddc)
            other = "resample_kernel" if kernel == "ddc_kernel" else "ddc_kernel"
            assert counts[kernel] == 1 and counts[other] == 0, (kernel, counts)
            assert (counts["ddc_history_kernel"], counts["ddc_array_cov_kernel"], counts["ddc_stap_cov_kernel"]) == (hist, cov, lag), (kernel, counts)
            assert engine.prof_read("")[1] == sum(counts.values()), counts
    finally:
        engine.prof_enable(False)


# ------------------------------------------------------------------------------------------------ 2. a delayed unit weight
DELAYED = ["K3_int8_complex", "K4_2bit_complex", "K3_int16_complex_swapped", "K3_1bit_complex_6bit_frame", "K8_4bit_complex_68bit_frame"]


@pytest.mark.parametrize("name", DELAYED)
def test_a_unit_weight_at_one_tap_gives_the_layout_converter_on_the_delayed_stream(engine, name):
    """e_a at tap t0: the ring of sdr_ddc_create_layout at lanes[a] on the stream with t0 zero frames prepended (a packed stream
    is unpacked to int8 for that: no packed code need mean zero)."""
    layout, lanes = geometry_of(name)
    n = cases.frames(cases.N_FRAMES, layout)
    raw, K = cases.stream(layout, n), len(lanes)
    plain, plain_layout = cases.unpacked(raw, layout) if layout.field == dc.FIELD_PACKED else (raw, layout)
    for ring_fmt in (FMT_CI8, FMT_CI16, FMT_CF64):
        engine.iq_alloc(CAPACITY, ring_fmt)
        gain = lcases.gain_for(plain_layout, ring_fmt) * (8.0 if layout.field == dc.FIELD_PACKED else 1.0)
        for shape in cases.FILTERED:
            n_out = lcases.out_total(shape, n)
            for T in (2, 8):
                for t0 in (0, T - 1):
                    for a in (0, K - 1):
                        cfg = cases.config(shape, cases.FCWS["odd"], gain, layout, scases.geometry(lanes, T, stap.unit_weights(T, K, a, t0)))
                        want_cfg = cases.config(shape, cases.FCWS["odd"], gain, ar.element_layout(plain_layout, lanes[a]))
                        want = push_all(engine, want_cfg, scases.delayed(plain, plain_layout, t0, n), n_out)
                        assert_same_bytes(push_all(engine, cfg, raw, n_out), want, (dcases.RING_NAMES[ring_fmt], shape, T, t0, a))


# ------------------------------------------------------------------------------------------------ 3. general weights against the statement
GENERAL = [("K2_int8_real", 3), ("K2_int8_real", 8), ("K8_int8_complex", 3), ("K8_int8_complex", 8)]


@pytest.mark.parametrize("name,T", GENERAL)
def test_general_weights_without_a_mixer_equal_the_statement_bit_for_bit(engine, name, T):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.SHAPES:
            cfg = cases.config(shape, 0, cases.gain_for(layout, ring_fmt, K), layout, scases.geometry(lanes, T, scases.general_weights(T, K)))
            want = stap.statement(cfg, [raw], ring_fmt)
            assert_same_bytes(push_all(engine, cfg, raw, want.size // 2), want, (dcases.RING_NAMES[ring_fmt], shape))


@pytest.mark.parametrize("name,T", GENERAL)
def test_general_weights_with_a_mixer_are_held_as_the_converter_is(engine, name, T):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.FILTERED:
            cfg = cases.config(shape, cases.FCWS["odd"], cases.gain_for(layout, ring_fmt, K), layout, scases.geometry(lanes, T, scases.general_weights(T, K)))
            v = stap.statement(cfg, [raw])
            check_ring(push_all(engine, cfg, raw, v.size), v, cfg, ring_fmt, scases.x_max(cfg, raw), (name, T, dcases.RING_NAMES[ring_fmt], shape))


def test_float32_elements_against_the_statement(engine):
    layout, lanes, T = dc.InputLayout(dc.FIELD_FLOAT32, 0, 6, 0, True), (4, 0, 2), 3
    raw = lcases.fractional(True, 3 * cases.N_FRAMES)
    geometry = scases.geometry(lanes, T, scases.general_weights(T, 3))
    for ring_fmt in (FMT_CF64, FMT_CF32):
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.SHAPES:
            cfg = cases.config(shape, 0, 1000.0, layout, geometry)
            want = stap.statement(cfg, [raw], ring_fmt)
            assert_same_bytes(push_all(engine, cfg, raw, want.size // 2), want, (dcases.RING_NAMES[ring_fmt], shape))
            cfg = cases.config(shape, cases.FCWS["odd"], 1000.0, layout, geometry)
            v = stap.statement(cfg, [raw])
            check_ring(push_all(engine, cfg, raw, v.size), v, cfg, ring_fmt, scases.x_max(cfg, raw), ("float32", dcases.RING_NAMES[ring_fmt], shape))


# ------------------------------------------------------------------------------------------------ 4. the cut, the weights, the lag covariance
CUTS = [("K3_int8_complex", (33, 2)), ("K3_1bit_complex_6bit_frame", (3, 2, 7)), ("K3_int16_complex_swapped", (1, 1)), ("K8_4bit_complex_68bit_frame", (33, 2))]


@pytest.mark.parametrize("name,shape", CUTS, ids=lambda v: v if isinstance(v, str) else lcases.shape_id(v))
def test_ring_and_lag_covariance_do_not_depend_on_the_cut(engine, name, shape):
    """T = 8.  A first push of one frame (one group of a packed layout), pushes shorter than T - 1 = 7 frames at the start and in
    the middle, a push of 2100 frames whose tile boundaries (1024 outputs of the integer converter) lie inside tap spans, against
    three pushes cut at the weight changes alone.  The weights change twice, 4 frames apart: inputs behind the second change
    still reach over frames that were pushed before the first.  The lag covariance is read and cleared at the first change: the
    lags of the next inputs still see the frames before it.  Integer fields: the covariance equals the statement's."""
    T = 8
    layout, lanes = geometry_of(name)
    group = layout.frame_group
    n = cases.frames(cases.N_FRAMES, layout)
    raw, K = cases.stream(layout, n), len(lanes)
    marks = (1000, 1004)
    weights = {0: scases.general_weights(T, K, 0), marks[0]: scases.general_weights(T, K, 1), marks[1]: scases.general_weights(T, K, 2)}
    total = lcases.out_total(shape, n)
    cfg = cases.config(shape, cases.FCWS["odd"], lcases.gain_for(layout, FMT_CF64) * (8.0 if layout.field == dc.FIELD_PACKED else 1.0), layout,
                       scases.geometry(lanes, T, weights[0], measure=True))
    small = [1, 1, 2, 3, 5, 2100, 1, 4, 6, 2, 0, 40, 3]
    assert group < T - 1 and any(0 < -(-v // group) * group < T - 1 for v in small[6:])
    engine.iq_alloc(lcases.ring_capacity(total), FMT_CF64)
    rings, covs, st = [], [], stap.Statement(cfg)
    want_covs = []
    ddc = engine.ddc_create(cfg)
    try:
        for lengths in ([], small):
            engine.iq_upload(np.zeros(2 * lcases.ring_capacity(total)), 0)
            engine.ddc_reset(ddc)
            engine.ddc_stap_weights(ddc, weights[0])                          # (a reset keeps the weights: those of the last run)
            st.reset()
            st.set_weights(weights[0])
            at, parts, read = 0, [], []
            for first, count in cases.cut_with_marks(lengths, marks, n, group):
                if first in marks and count > 0:
                    engine.ddc_stap_weights(ddc, weights[first])
                    st.set_weights(weights[first])
                    if first == marks[0]:
                        read.append(engine.ddc_stap_covariance(ddc, clear=True))
                        want_covs.append(st.read_covariance(True))
                part = cases.piece(raw, layout, first, count)
                want = st.out_count(count)
                assert engine.ddc_out_count(ddc, count) == want
                assert engine.ddc_push(ddc, part, at) == want
                parts.append(st.push(part))
                at += want
            assert at == total
            rings.append(engine.iq_download(total, 0))
            read.append(engine.ddc_stap_covariance(ddc))
            want_covs.append(st.read_covariance())
            covs.append(read)
            v = np.concatenate(parts)
    finally:
        engine.ddc_destroy(ddc)
    assert_same_bytes(rings[1], rings[0], "pieces against three pushes")
    x_max = max(scases.x_max(cases.config(shape, 0, 1.0, layout, scases.geometry(lanes, T, w)), raw) for w in weights.values())
    check_ring(rings[0], v, cfg, FMT_CF64, x_max, (name, shape))
    assert not np.array_equal(v, stap.statement(cfg, [raw]))                       # (the changes are in the ring)
    for run in range(2):
        for k in range(2):
            (got_C, got_n), (want_C, want_n) = covs[run][k], want_covs[2 * run + k]
            assert got_n == want_n == (marks[0], n - marks[0])[k] and got_C.shape == (T, K, K)
            assert np.array_equal(got_C, want_C) and np.any(want_C[T - 1] != 0), (run, k)
    # the lags behind the clearing read saw the frames before it: not what a stream that begins there gives
    fresh = stap.Statement(cfg)
    fresh.push(cases.piece(raw, layout, marks[0], n - marks[0]))
    assert not np.array_equal(fresh.read_covariance()[0][1:], want_covs[1][0][1:]) and np.array_equal(fresh.read_covariance()[0][0], want_covs[1][0][0])


@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page_locked"])
def test_push_queue_equals_push(engine, page_locked):
    layout, lanes, T = cases.packed_layout("K4_2bit_complex", False), cases.PACKED["K4_2bit_complex"][3], 5
    n, ring_fmt, shape = cases.N_FRAMES, FMT_CI16, (33, 2)
    raw = cases.stream(layout, n)
    w = [scases.general_weights(T, 4, s) for s in range(3)]
    cfg = cases.config(shape, cases.FCWS["odd"], 48.0 * dcases.GOLD, layout, scases.geometry(lanes, T, w[0], measure=True))
    engine.iq_alloc(CAPACITY, ring_fmt)
    ddc = engine.ddc_create(cfg)
    block = engine.host_alloc(raw.size, np.uint8) if page_locked else None
    try:
        step = 1000
        at = 0
        for k, lo in enumerate(range(0, n, step)):
            engine.ddc_stap_weights(ddc, w[k])
            at += engine.ddc_push(ddc, cases.piece(raw, layout, lo, step), at)
        want, want_cov = engine.iq_download(at, 0), engine.ddc_stap_covariance(ddc)
        engine.iq_upload(np.zeros(2 * CAPACITY, dtype=np.int16), 0)
        engine.ddc_reset(ddc)
        src = block if page_locked else raw.copy()
        src[:] = raw
        got_n, per = 0, layout.bytes_for(step)
        for k in range(n // step):                            # several pushes in flight, the weights changed between them without a wait
            engine.ddc_stap_weights(ddc, w[k])
            got_n += engine.ddc_push_queue(ddc, src[k * per:(k + 1) * per], got_n)
        engine.sync()
        assert got_n == at == lcases.out_total(shape, n)
        assert_same_bytes(engine.iq_download(at, 0), want, "queued")
        got_cov = engine.ddc_stap_covariance(ddc)
        assert got_cov[1] == want_cov[1] == n and np.array_equal(got_cov[0], want_cov[0])
        st = stap.Statement(cfg)
        st.push(raw)
        assert np.array_equal(want_cov[0], st.read_covariance()[0])
    finally:
        engine.ddc_destroy(ddc)
        if block is not None:
            engine.host_free(block)


# ------------------------------------------------------------------------------------------------ 5. the lag covariance
def test_lag_covariance_of_int16_rails_is_beyond_any_int32_partial(engine):
    """Every component of every element -32768 over 70 000 frames: every entry of C[tau] is 2^31 (70 000 - tau), imaginary part 0."""
    layout, lanes, n, T = dc.InputLayout(dc.FIELD_INT16, 0, 6, 0, True), (4, 0, 2), 70000, 3
    raw = np.full(6 * n, -32768, dtype=np.int16)
    cfg = cases.config((1, 1), 0, 2.0 ** -18, layout, scases.geometry(lanes, T, measure=True))
    engine.iq_alloc(lcases.ring_capacity(n), FMT_CI16)
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == n
        got_C, got_n = engine.ddc_stap_covariance(ddc)
    finally:
        engine.ddc_destroy(ddc)
    assert got_n == n and 2 ** 31 * (n - T + 1) > 2 ** 47
    for tau in range(T):
        assert np.array_equal(got_C[tau], np.full((3, 3), float(2 ** 31 * (n - tau)) + 0j)), tau
    sr, si = ar.elements(raw, layout, lanes)
    zeros = np.zeros((3, T - 1))
    want = stap.lag_covariance(np.concatenate([zeros, sr], axis=1), np.concatenate([zeros, si], axis=1), T, True)
    assert np.array_equal(got_C, want)


def test_lag_covariance_of_float32_fields_within_the_derived_bound_and_reproducible(engine):
    layout, lanes, T = dc.InputLayout(dc.FIELD_FLOAT32, 0, 6, 0, True), (4, 0, 2), 4
    raw = lcases.fractional(True, 3 * cases.N_FRAMES)
    cfg = cases.config((3, 2), 0, 1.0, layout, scases.geometry(lanes, T, measure=True))
    engine.iq_alloc(CAPACITY, FMT_CF64)
    runs = []
    for _ in range(2):
        ddc = engine.ddc_create(cfg)
        try:
            engine.ddc_push(ddc, cases.piece(raw, layout, 0, 1001), 0)
            engine.ddc_push(ddc, cases.piece(raw, layout, 1001, 2), 0)
            engine.ddc_push(ddc, cases.piece(raw, layout, 1003, cases.N_FRAMES - 1003), 0)
            runs.append(engine.ddc_stap_covariance(ddc))
        finally:
            engine.ddc_destroy(ddc)
    (Cd, n), (C2, n2) = runs
    assert n == n2 == cases.N_FRAMES and np.array_equal(Cd.view(np.uint64), C2.view(np.uint64))      # the same pushes, the same bits
    sr, si = ar.elements(raw, layout, lanes)
    zeros = np.zeros((3, T - 1))
    sr, si = np.concatenate([zeros, sr], axis=1), np.concatenate([zeros, si], axis=1)
    want = stap.lag_covariance(sr, si, T, False)
    bound_re, bound_im = stap.lag_covariance_bound(sr, si, T)
    err_re, err_im = np.abs(Cd.real - want.real), np.abs(Cd.imag - want.imag)
    print(f"max |C - statement|: re {err_re.max():.3e} (bound {bound_re.min():.3e}), im {err_im.max():.3e} (bound {bound_im.min():.3e})")
    assert np.all(err_re <= bound_re) and np.all(err_im <= bound_im) and np.all(Cd[0].diagonal().imag == 0) and np.any(Cd[T - 1].imag != 0)


# ------------------------------------------------------------------------------------------------ 6. refusals
def _create_raw(engine, layout, array, n_taps, w, D=1, taps=(1.0,), L=1):
    t = (C.c_double * len(taps))(*taps)
    cfg = _lib.DdcCfg(77, D, len(taps), 0, 0, 1.0, C.cast(t, C.POINTER(C.c_double)))
    h = C.c_void_p()
    wa = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    rc = _lib.load().sdr_ddc_create_stap(engine._h, C.byref(cfg), L, C.byref(layout) if layout is not None else None,
                                         C.byref(array) if array is not None else None, n_taps,
                                         wa.ctypes.data_as(C.POINTER(C.c_double)) if wa is not None else None, C.byref(h))
    if rc == 0:
        _lib.load().sdr_ddc_destroy(engine._h, h)
    return rc, h.value


def _array(K, lanes, flags=0):
    c = _lib.DdcArray(K, flags)
    for a, lane in enumerate(lanes):
        c.lanes[a] = lane
    for a in range(8):
        c.weights[a][0] = c.weights[a][1] = float("nan")              # (the array's own weights are not read)
    return c


def test_refusals_leave_the_ring_and_the_converter_as_they_were(engine):
    cap = 4096
    engine.iq_alloc(cap, FMT_CI16)
    pattern = np.random.default_rng(scases.SEED + 6).integers(-3000, 3000, 2 * cap).astype(np.int16)
    engine.iq_upload(pattern, 0)
    lib = _lib.load()
    real4, cplx4 = _lib.DdcLayout(0, 0, 4, 0, 0, 0), _lib.DdcLayout(0, 0, 4, 0, 1, 0)
    nan, inf = float("nan"), float("inf")
    ones = [1.0] * 128
    # every cause of sdr_ddc_create_array ...
    for layout, array in ((real4, _array(1, (0,))), (real4, _array(0, ())), (real4, _array(9, range(8))), (real4, _array(-1, ())),
                          (real4, _array(2, (0, 0))), (real4, _array(3, (1, 2, 1))), (real4, _array(2, (0, 4))), (real4, _array(2, (-1, 0))),
                          (cplx4, _array(2, (0, 3))), (cplx4, _array(2, (3, 0))), (real4, _array(2, (0, 1), 2)), (real4, _array(2, (0, 1), 3)),
                          (real4, _array(2, (0, 1), -1)), (_lib.DdcLayout(0, 0, 65, 0, 0, 0), _array(2, (0, 1))),
                          (_lib.DdcLayout(3, 3, 4, 0, 0, 0), _array(2, (0, 1))), (None, _array(2, (0, 1))), (real4, None)):
        rc, handle = _create_raw(engine, layout, array, 3, ones)
        assert rc == INVALID and not handle
    good = _array(2, (3, 0), 1)
    for T in (1, 8):
        assert _create_raw(engine, real4, good, T, ones)[0] == 0
    # ... the taps, the weights ...
    for T in (0, -1, 9, 64):
        assert _create_raw(engine, real4, good, T, ones)[0] == INVALID, T
    assert _create_raw(engine, real4, good, 3, None)[0] == INVALID
    for at, bad in ((0, nan), (5, inf), (11, -inf)):
        w = [1.0] * 12
        w[at] = bad
        assert _create_raw(engine, real4, good, 3, w)[0] == INVALID, at
    assert _create_raw(engine, real4, good, 3, [1.0] * 12 + [nan])[0] == 0                # (weights past [T][K][2] are not read)
    for kw in (dict(D=0), dict(D=65), dict(taps=(1.0, nan)), dict(L=0), dict(L=1025), dict(L=2, D=129)):
        assert _create_raw(engine, real4, good, 3, ones, **kw)[0] == INVALID, kw
    h = C.c_void_p()
    cfg = _lib.DdcCfg(0, 1, 1, 0, 0, 1.0, C.cast((C.c_double * 1)(1.0), C.POINTER(C.c_double)))
    wp = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    assert lib.sdr_ddc_create_stap(engine._h, None, 1, C.byref(real4), C.byref(good), 3, wp(ones), C.byref(h)) == INVALID
    assert lib.sdr_ddc_create_stap(engine._h, C.byref(cfg), 1, C.byref(real4), C.byref(good), 3, wp(ones), None) == INVALID

    layout, lanes, T = cases.packed_layout("K3_1bit_complex_6bit_frame", False), (4, 0, 2), 4
    raw = cases.stream(layout, 2000)
    w = scases.general_weights(T, 3)
    Cb, n = np.zeros(2 * T * 9), C.c_int64(-7)
    Cp, np_ = Cb.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)
    for shape in ((3, 2), (3, 2, 7)):
        quiet = engine.ddc_create(cases.config(shape, 0, 1.0, layout, scases.geometry(lanes, T, w)))
        plain_array = engine.ddc_create(cases.config(shape, 0, 1.0, layout, ar.ArrayGeometry(lanes, measure=True)))
        other = engine.ddc_create(cases.config(shape, 0, 1.0, ar.element_layout(layout, 0)))
        cfg = cases.config(shape, cases.FCWS["odd"], 24.0 * dcases.GOLD, layout, scases.geometry(lanes, T, w, measure=True))
        ddc = engine.ddc_create(cfg)
        try:
            # the two STAP calls on converters that sdr_ddc_create_stap did not make, the two array calls on one it made
            for d in (other, plain_array):
                assert lib.sdr_ddc_stap_weights(engine._h, d.handle, wp([1.0] * 24)) == INVALID
                assert lib.sdr_ddc_stap_covariance(engine._h, d.handle, Cp, np_, 1) == INVALID
            assert lib.sdr_ddc_array_weights(engine._h, ddc.handle, wp([1.0] * 6)) == INVALID
            assert lib.sdr_ddc_array_covariance(engine._h, ddc.handle, Cp, np_, 1) == INVALID
            assert lib.sdr_ddc_stap_covariance(engine._h, quiet.handle, Cp, np_, 1) == STATE
            assert lib.sdr_ddc_stap_weights(engine._h, ddc.handle, None) == INVALID and lib.sdr_ddc_stap_weights(engine._h, None, wp([1.0] * 24)) == INVALID
            assert lib.sdr_ddc_stap_covariance(engine._h, ddc.handle, None, np_, 0) == INVALID and lib.sdr_ddc_stap_covariance(engine._h, ddc.handle, Cp, None, 0) == INVALID
            for at, bad in ((2, nan), (23, -inf)):
                v = [0.5] * 24
                v[at] = bad
                assert lib.sdr_ddc_stap_weights(engine._h, ddc.handle, wp(v)) == INVALID
            assert n.value == -7 and not np.any(Cb)
            # pushes that are not whole bytes (6-bit frames, whole every 4)
            n_out = C.c_int64(-7)
            for call in (lib.sdr_ddc_push, lib.sdr_ddc_push_queue):
                for n_in in (1, 2, 3, 1999):
                    assert call(engine._h, ddc.handle, raw.ctypes.data, n_in, 0, C.byref(n_out)) == INVALID and n_out.value == -7
            assert np.array_equal(engine.iq_download(cap, 0), pattern)
            got_C, got_n = engine.ddc_stap_covariance(ddc)
            assert got_n == 0 and not np.any(got_C)
            # ... and the pushes give what they would have given, with the weights the converter was made with, the tail untouched
            got_n = engine.ddc_push(ddc, raw[:layout.bytes_for(4)], 0)
            got_n += engine.ddc_push(ddc, raw[layout.bytes_for(4):], got_n)
            got = engine.iq_download(got_n, 0)
            st = stap.Statement(cfg)
            want = st.push(raw)
            check_ring(got, want, cfg, FMT_CI16, scases.x_max(cfg, raw), ("after the refusals", shape))
            got_C, got_count = engine.ddc_stap_covariance(ddc)
            want_C, want_count = st.read_covariance()
            assert got_count == want_count == 2000 and np.array_equal(got_C, want_C)
        finally:
            for d in (ddc, quiet, other, plain_array):
                engine.ddc_destroy(d)
        engine.iq_upload(pattern, 0)


# ------------------------------------------------------------------------------------------------ 7. a mitigator behind it
@pytest.mark.parametrize("ring_fmt", [FMT_CI8, FMT_CF64], ids=["ring_ci8", "ring_cf64"])
def test_a_mitigator_behind_a_space_time_converter(engine, ring_fmt):
    """int8 elements with weights in {+-1, +-i} at tap 1 of 2, a blanker and a 64-point excisor behind them: the ring and the
    counters of the IN_CI16 converter with the same mitigator on the host-combined integers, one zero input prepended."""
    layout, lanes = cases.GEOMETRIES["K3_int8_complex"]
    raw = cases.stream(layout)
    q = cases.quarter_weights(3, 1)
    plain = cases.combined_integers(raw, layout, lanes, q)
    plain = np.ascontiguousarray(np.concatenate([np.zeros(2, dtype=plain.dtype), plain])[:plain.size])
    w = np.zeros((2, 3), dtype=np.complex128)
    w[1] = q
    shape, gain = (33, 2), dcases.GOLD / 4.0
    new_cfg, old_cfg = cases.config(shape, cases.FCWS["odd"], gain, layout, scases.geometry(lanes, 2, w)), cases.config(shape, cases.FCWS["odd"], gain)
    v = dc.statement(old_cfg, [plain])
    mit = mt.MitigationConfig(float(np.quantile(np.abs(v), 0.99)), 2, 5, 64, mt.excision_limits(v[:1024], 64, 3.0))
    n_out = v.size
    engine.iq_alloc(lcases.ring_capacity(n_out), ring_fmt)
    results = []
    for cfg, data, per in ((new_cfg, raw, layout.stride), (old_cfg, plain, 2)):
        ddc = engine.ddc_create(cfg)
        try:
            engine.ddc_mitigate(ddc, mit)
            assert engine.ddc_delay(ddc) == 64 + 2                              # (the filter's own: the reference tap is the host's to add)
            half = 1400 * per                                                 # (two pushes: the mitigator's state and the tail are carried)
            assert engine.ddc_push(ddc, data[:half], 0) + engine.ddc_push(ddc, data[half:], 700) == n_out
            results.append((engine.iq_download(n_out, 0), engine.ddc_mitigation_stats(ddc)))
        finally:
            engine.ddc_destroy(ddc)
    (got, got_stats), (want, want_stats) = results
    assert_same_bytes(got, want, "mitigated")
    assert got_stats == want_stats and want_stats.n_triggers > 0 and want_stats.n_outputs == n_out


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_two_partial_band_jammers_need_the_time_taps(engine, tmp_path):
    """stap_cases.two_jammers (2 elements, int16, 4 MHz; two 0.5 MHz jammers from different directions, each 20 dB above an
    element's noise) through ChannelManager with the [RFSIGNAL] keys.  On element 0 alone and with array_taps = 1 power inversion
    -- one spatial null against two directions -- the acquisition misses the satellite's bin or sample or falls under the plugin's
    ratio threshold of 1.5; with array_taps = 5 it finds bin 13 within a sample of 2826 + 2 (the reference tap) with a ratio above
    1.5 (tests/test_stap.py has the oracle's figures).  In the two array runs the device's ring equals the statement's byte for
    byte, the trained weights are the host's solve of the statement's (lag) covariance, and the live converter's covariance over
    the 8 ms equals the statement's."""
    import packed_cases
    from sydr_amd.signal.iqsource import RFSignal
    raw, ms, per_ms = scases.two_jammers(), scases.E2E_MS, int(scases.E2E_FS * 1e-3)
    path = tmp_path / "stap.bin"
    raw.tofile(path)
    train = cases.piece(raw, scases.E2E_LAYOUT, 0, scases.E2E_TRAIN_MS * per_ms)
    runs = (("element0", {}, 1), ("taps1", dict(array_mode="power_inversion", array_train_ms=scases.E2E_TRAIN_MS, array_taps=1), 1),
            ("taps5", dict(array_mode="power_inversion", array_train_ms=scases.E2E_TRAIN_MS, array_taps=scases.E2E_TAPS), scases.E2E_TAPS))
    found = {}
    for mode, more, T in runs:
        sig = RFSignal(scases.e2e_conf(path, **more))
        got, mgr = packed_cases.receive(sig, engine, prns=[scases.E2E_PRN], cfg=packed_cases.kaplan_config(), ms=ms, mode="ticks")
        try:
            ring = engine.iq_download(ms * per_ms, 0)
            weights = getattr(mgr, "arrayWeights", sig.frontEnd.config.array.weights)
            cov, delay = mgr.arrayCovariance(), mgr.arrayDelay
        finally:
            mgr.close()
        acq = [p for tick in got for p in tick if p["type"] is ChannelMessage.ACQUISITION_UPDATE]
        assert len(acq) == 1
        found[mode] = ([int(acq[0]["frequency_idx"]), int(acq[0]["code_idx"])], float(acq[0]["peak_ratio"]))
        print(mode, found[mode], "weights", weights)
        if mode == "element0":
            assert cov is None and delay == 0
            continue
        weights = np.asarray(weights)
        st = stap.Statement(scases.e2e_config(T, None, True))
        st.push(train)
        want_C, want_n = st.read_covariance()
        if T == 1:
            assert weights.shape == (2,) and delay == 0 and np.array_equal(weights, ar.power_inversion(want_C[0], want_n))
        else:
            assert weights.shape == (T, 2) and delay == (T - 1) // 2 and np.array_equal(weights, stap.power_inversion(want_C, want_n))
        st = stap.Statement(scases.e2e_config(T, weights.reshape(T, 2), True))
        assert np.array_equal(ring, dc.quantise(st.push(raw), FMT_CI16)) and np.any(ring != 0), mode
        whole_C, whole_n = st.read_covariance()
        assert cov[1] == whole_n == ms * per_ms and np.array_equal(np.asarray(cov[0]).reshape(T, 2, 2), whole_C)
    truth = [13, 2826]
    for mode in ("element0", "taps1"):
        assert found[mode][1] < 1.5 or found[mode][0] != truth, found
    peak, ratio = found["taps5"]
    assert peak[0] == 13 and abs(peak[1] - (2826 + 2)) <= 1 and ratio > 1.5, found
