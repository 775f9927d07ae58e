"""Antenna arrays of the device's down-converter (sdr_ddc_create_array: the K elements of a frame decoded and combined where
ddc_kernel / resample_kernel load their inputs; sdr_ddc_array_weights; sdr_ddc_array_covariance).

Against existing code paths every comparison demands equal ring bytes, in every ring format: a unit weight against the layout's
converter at that lane, weights in {+-1, +-i} on int8 elements against IN_CI16 on the host-combined integers, a packed array
against the INT8 array on the unpacked bytes.  Against the NumPy statement (sydr_amd/signal/array.py) general complex weights
are held bit for bit with fcw = 0 (no phasor: the same products and sums in the same order) and within the converter's own
derived bound `dc.tolerance`, evaluated with the combined inputs, with a mixer.  The covariance of integer fields equals the
statement's; of float32 fields it lies within 2 n 2^-52 sum(|..| + |..|) (derived: n terms of two products in any order)."""
import ctypes as C

import numpy as np
import pytest

import array_cases as cases
import downconvert_cases as dcases
import ddc_layout_cases as lcases
from test_gpu_downconvert import check_ring

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI8, FMT_CI16, Engine, array_struct, layout_struct
from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt
from sydr_amd.utils.enumerations import ChannelMessage

pytestmark = pytest.mark.gpu

INVALID, RANGE, STATE = -1, -5, -6
CAPACITY = lcases.ring_capacity(2 * cases.N_FRAMES)
RINGS = dcases.RING_FORMATS


def push_all(engine, cfg, raw, n_out):
    return lcases.push_all(engine, cfg, raw, n_out)


def assert_same_bytes(got, want, what):
    bad = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (what, bad.size, bad[:5])
    assert np.any(want != 0), what


# ------------------------------------------------------------------------------------------------ 1. against existing code paths
@pytest.mark.parametrize("name", list(cases.GEOMETRIES))
def test_a_unit_weight_gives_the_ring_of_the_layout_converter_at_that_lane(engine, name):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        gain = lcases.gain_for(layout, ring_fmt)
        for shape in cases.SHAPES:
            n_out = lcases.out_total(shape, cases.N_FRAMES)
            for a, lane in enumerate(lanes):
                cfg = cases.config(shape, cases.FCWS["odd"], gain, layout, ar.ArrayGeometry(lanes, ar.unit_weights(K, a)))
                want_cfg = cases.config(shape, cases.FCWS["odd"], gain, ar.element_layout(layout, lane))
                assert_same_bytes(push_all(engine, cfg, raw, n_out), push_all(engine, want_cfg, raw, n_out), (dcases.RING_NAMES[ring_fmt], shape, a))


@pytest.mark.parametrize("name", cases.INT8_GEOMETRIES)
def test_quarter_turn_weights_on_int8_give_the_ring_of_ci16_on_the_combined_integers(engine, name):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        gain = cases.gain_for(layout, ring_fmt, K)
        for shape in cases.FILTERED:
            n_out = lcases.out_total(shape, cases.N_FRAMES)
            for turn in (0, 1, 3):
                w = cases.quarter_weights(K, turn)
                got = push_all(engine, cases.config(shape, cases.FCWS["odd"], gain, layout, ar.ArrayGeometry(lanes, w)), raw, n_out)
                want = push_all(engine, cases.config(shape, cases.FCWS["odd"], gain), cases.combined_integers(raw, layout, lanes, w), n_out)
                assert_same_bytes(got, want, (dcases.RING_NAMES[ring_fmt], shape, turn))


@pytest.mark.parametrize("msb", [False, True], ids=["lsb", "msb"])
@pytest.mark.parametrize("name", list(cases.PACKED))
def test_a_packed_array_gives_the_ring_of_the_int8_array_on_the_unpacked_bytes(engine, name, msb):
    layout, lanes = cases.packed_layout(name, msb), cases.PACKED[name][3]
    n = cases.frames(cases.N_FRAMES, layout)
    raw = cases.stream(layout, n)
    plain, plain_layout = cases.unpacked(raw, layout)
    assert len(np.unique(plain)) == 1 << layout.bits and plain.size == n * layout.stride
    geometry = ar.ArrayGeometry(lanes, cases.general_weights(len(lanes)))
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        gain = dcases.GOLD * (8.0 if ring_fmt != FMT_CI8 else 4.0)
        for shape in cases.SHAPES:
            n_out = lcases.out_total(shape, n)
            got = push_all(engine, cases.config(shape, cases.FCWS["odd"], gain, layout, geometry), raw, n_out)
            want = push_all(engine, cases.config(shape, cases.FCWS["odd"], gain, plain_layout, geometry), plain, n_out)
            assert_same_bytes(got, want, (dcases.RING_NAMES[ring_fmt], shape))


# ------------------------------------------------------------------------------------------------ 2. against the statement
@pytest.mark.parametrize("name", list(cases.GEOMETRIES))
def test_general_weights_without_a_mixer_equal_the_statement_bit_for_bit(engine, name):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.SHAPES:
            cfg = cases.config(shape, 0, cases.gain_for(layout, ring_fmt, K), layout, ar.ArrayGeometry(lanes, cases.general_weights(K)))
            want = ar.statement(cfg, [raw], ring_fmt)
            got = push_all(engine, cfg, raw, want.size // 2)
            assert_same_bytes(got, want, (dcases.RING_NAMES[ring_fmt], shape))


@pytest.mark.parametrize("name", list(cases.GEOMETRIES))
def test_general_weights_with_a_mixer_are_held_as_the_converter_is(engine, name):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    for ring_fmt in RINGS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.SHAPES:
            for fcw_name in ("quarter", "odd"):
                cfg = cases.config(shape, cases.FCWS[fcw_name], cases.gain_for(layout, ring_fmt, K), layout, ar.ArrayGeometry(lanes, cases.general_weights(K)))
                v = ar.statement(cfg, [raw])
                got = push_all(engine, cfg, raw, v.size)
                check_ring(got, v, cfg, ring_fmt, cases.x_max(cfg, raw), (name, dcases.RING_NAMES[ring_fmt], shape, fcw_name))


def test_float32_elements_against_the_statement(engine):
    layout, lanes = dc.InputLayout(dc.FIELD_FLOAT32, 0, 6, 0, True), (4, 0, 2)
    raw = lcases.fractional(True, 3 * cases.N_FRAMES)
    geometry = ar.ArrayGeometry(lanes, cases.general_weights(3))
    for ring_fmt in (FMT_CF64, FMT_CF32):
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.SHAPES:
            cfg = cases.config(shape, 0, 1000.0, layout, geometry)
            want = ar.statement(cfg, [raw], ring_fmt)
            assert_same_bytes(push_all(engine, cfg, raw, want.size // 2), want, (dcases.RING_NAMES[ring_fmt], shape))
            cfg = cases.config(shape, cases.FCWS["odd"], 1000.0, layout, geometry)
            v = ar.statement(cfg, [raw])
            check_ring(push_all(engine, cfg, raw, v.size), v, cfg, ring_fmt, cases.x_max(cfg, raw), ("float32", dcases.RING_NAMES[ring_fmt], shape))


# ------------------------------------------------------------------------------------------------ 3. the cut and the weights
CUTS = [("K3_int8_complex", (33, 2)), ("K8_int8_real", (3, 2, 7)), ("K3_int16_complex_swapped", (512, 16)), ("K3_1bit_complex_6bit_frame", (33, 2)),
        ("K2_int8_real", (250, 341, 1500))]


@pytest.mark.parametrize("name,shape", CUTS, ids=lambda v: v if isinstance(v, str) else lcases.shape_id(v))
def test_the_ring_does_not_depend_on_the_cut_with_weights_changed_at_fixed_inputs(engine, name, shape):
    """Pushes of 1 frame, of fewer frames than Tp - 1 and of the input-layout tests' lengths (1, 2, 3, Tp - 2, Tp - 1, Tp, 0, Tp + 1,
    4097 rounded to whole bytes) against three pushes cut at the weight changes alone; the weights change twice, the second time
    while inputs combined with the first and the second vector are both still in the filter's history."""
    layout, lanes = (cases.packed_layout(name, False), cases.PACKED[name][3]) if name in cases.PACKED else cases.GEOMETRIES[name]
    group = layout.frame_group
    n = cases.frames(2 * cases.N_FRAMES, layout)
    raw, K, Tp = cases.stream(layout, n), len(lanes), lcases.phase_taps(shape)
    marks = (1000, 1008)
    weights = {0: cases.general_weights(K, 0), marks[0]: cases.general_weights(K, 1), marks[1]: cases.general_weights(K, 2)}
    total = lcases.out_total(shape, n)
    cfg = cases.config(shape, cases.FCWS["odd"], lcases.gain_for(layout, FMT_CF64), layout, ar.ArrayGeometry(lanes, weights[0]))
    small = [1, 1, 2, 1] + ([Tp - 2] if Tp > 2 else []) + lcases.rounded_lengths(Tp, group) + [900, 1, 1, 3]
    assert 0 in small and (Tp <= 2 or any(0 < v < Tp - 1 for v in small))
    engine.iq_alloc(lcases.ring_capacity(total), FMT_CF64)
    rings, st = [], ar.Statement(cfg)
    ddc = engine.ddc_create(cfg)
    try:
        for lengths in ([], small):
            engine.iq_upload(np.zeros(2 * lcases.ring_capacity(total)), 0)
            engine.ddc_reset(ddc)
            engine.ddc_array_weights(ddc, weights[0])                          # (a reset keeps the weights: those of the last run)
            st.reset()
            at = 0
            for first, count in cases.cut_with_marks(lengths, marks, n, group):
                if first in marks and count > 0:
                    engine.ddc_array_weights(ddc, weights[first])
                want = st.out_count(count)
                assert engine.ddc_out_count(ddc, count) == want
                assert engine.ddc_push(ddc, cases.piece(raw, layout, first, count), at) == want
                st.n_seen += count
                at += want
            assert at == total
            rings.append(engine.iq_download(total, 0))
    finally:
        engine.ddc_destroy(ddc)
    assert_same_bytes(rings[1], rings[0], "pieces against three pushes")
    v = ar.statement(cfg, [cases.piece(raw, layout, 0, marks[0]), cases.piece(raw, layout, marks[0], marks[1] - marks[0]), cases.piece(raw, layout, marks[1], n - marks[1])],
                     weights_at={1: weights[marks[0]], 2: weights[marks[1]]})
    x_max = max(cases.x_max(cfg, raw, w) for w in weights.values())
    check_ring(rings[0], v, cfg, FMT_CF64, x_max, (name, shape))
    assert not np.array_equal(v, ar.statement(cfg, [raw]))                       # (the changes are in the ring)


@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page_locked"])
def test_push_queue_equals_push(engine, page_locked):
    layout, lanes = cases.packed_layout("K4_2bit_complex", False), cases.PACKED["K4_2bit_complex"][3]
    n, ring_fmt, shape = cases.N_FRAMES, FMT_CI16, (33, 2)
    raw = cases.stream(layout, n)
    w = [cases.general_weights(4, s) for s in range(3)]
    cfg = cases.config(shape, cases.FCWS["odd"], 24.0 * dcases.GOLD, layout, ar.ArrayGeometry(lanes, w[0], measure=True))
    engine.iq_alloc(CAPACITY, ring_fmt)
    ddc = engine.ddc_create(cfg)
    block = engine.host_alloc(raw.size, np.uint8) if page_locked else None
    try:
        step = 1000
        at = 0
        for k, lo in enumerate(range(0, n, step)):
            engine.ddc_array_weights(ddc, w[k])
            at += engine.ddc_push(ddc, cases.piece(raw, layout, lo, step), at)
        want, want_cov = engine.iq_download(at, 0), engine.ddc_array_covariance(ddc)
        engine.iq_upload(np.zeros(2 * CAPACITY, dtype=np.int16), 0)
        engine.ddc_reset(ddc)
        src = block if page_locked else raw.copy()
        src[:] = raw
        got_n, per = 0, layout.bytes_for(step)
        for k in range(n // step):                            # several pushes in flight, the weights changed between them without a wait
            engine.ddc_array_weights(ddc, w[k])
            got_n += engine.ddc_push_queue(ddc, src[k * per:(k + 1) * per], got_n)
        engine.sync()
        assert got_n == at == lcases.out_total(shape, n)
        assert_same_bytes(engine.iq_download(at, 0), want, "queued")
        got_cov = engine.ddc_array_covariance(ddc)
        assert got_cov[1] == want_cov[1] == n and np.array_equal(got_cov[0], want_cov[0])
    finally:
        engine.ddc_destroy(ddc)
        if block is not None:
            engine.host_free(block)


@pytest.mark.parametrize("ring_fmt", [FMT_CI8, FMT_CF64], ids=["ring_ci8", "ring_cf64"])
def test_a_mitigator_behind_an_array(engine, ring_fmt):
    """int8 elements with weights in {+-1, +-i}, a blanker and a 64-point excisor behind them: the ring and the counters of the
    IN_CI16 converter with the same mitigator on the host-combined integers."""
    layout, lanes = cases.GEOMETRIES["K3_int8_complex"]
    raw = cases.stream(layout)
    w = cases.quarter_weights(3, 1)
    plain = cases.combined_integers(raw, layout, lanes, w)
    shape, gain = (33, 2), dcases.GOLD / 4.0
    new_cfg, old_cfg = cases.config(shape, cases.FCWS["odd"], gain, layout, ar.ArrayGeometry(lanes, w)), cases.config(shape, cases.FCWS["odd"], gain)
    v = dc.statement(old_cfg, [plain])
    mit = mt.MitigationConfig(float(np.quantile(np.abs(v), 0.99)), 2, 5, 64, mt.excision_limits(v[:1024], 64, 3.0))
    n_out = v.size
    engine.iq_alloc(lcases.ring_capacity(n_out), ring_fmt)
    results = []
    for cfg, data, per in ((new_cfg, raw, layout.stride), (old_cfg, plain, 2)):
        ddc = engine.ddc_create(cfg)
        try:
            engine.ddc_mitigate(ddc, mit)
            assert engine.ddc_delay(ddc) == 64 + 2
            half = 1400 * per                                                 # (two pushes: the mitigator's state is carried)
            assert engine.ddc_push(ddc, data[:half], 0) + engine.ddc_push(ddc, data[half:], 700) == n_out
            results.append((engine.iq_download(n_out, 0), engine.ddc_mitigation_stats(ddc)))
        finally:
            engine.ddc_destroy(ddc)
    (got, got_stats), (want, want_stats) = results
    assert_same_bytes(got, want, "mitigated")
    assert got_stats == want_stats and want_stats.n_triggers > 0 and want_stats.n_outputs == n_out


# ------------------------------------------------------------------------------------------------ 4. refusals
def _create_raw(engine, layout, array, D=1, taps=(1.0,), L=1):
    t = (C.c_double * len(taps))(*taps)
    cfg = _lib.DdcCfg(77, D, len(taps), 0, 0, 1.0, C.cast(t, C.POINTER(C.c_double)))
    h = C.c_void_p()
    rc = _lib.load().sdr_ddc_create_array(engine._h, C.byref(cfg), L, C.byref(layout) if layout is not None else None,
                                          C.byref(array) if array is not None else None, C.byref(h))
    if rc == 0:
        _lib.load().sdr_ddc_destroy(engine._h, h)
    return rc, h.value


def _array(K, lanes, flags=0, weights=None):
    c = _lib.DdcArray(K, flags)
    for a, lane in enumerate(lanes):
        c.lanes[a] = lane
    for a, w in enumerate(weights if weights is not None else [1.0] * 8):
        c.weights[a][0], c.weights[a][1] = complex(w).real, complex(w).imag
    return c


def test_refusals_leave_the_ring_and_the_converter_as_they_were(engine):
    cap = 4096
    engine.iq_alloc(cap, FMT_CI16)
    pattern = np.random.default_rng(cases.SEED + 6).integers(-3000, 3000, 2 * cap).astype(np.int16)
    engine.iq_upload(pattern, 0)
    lib = _lib.load()
    real4, cplx4 = _lib.DdcLayout(0, 0, 4, 0, 0, 0), _lib.DdcLayout(0, 0, 4, 0, 1, 0)
    nan, inf = float("nan"), float("inf")
    for layout, array in ((real4, _array(1, (0,))), (real4, _array(0, ())), (real4, _array(9, range(8))), (real4, _array(-1, ())),
                          (real4, _array(2, (0, 0))), (real4, _array(3, (1, 2, 1))), (real4, _array(2, (0, 4))), (real4, _array(2, (-1, 0))),
                          (cplx4, _array(2, (0, 3))), (cplx4, _array(2, (3, 0))), (real4, _array(2, (0, 1), 2)), (real4, _array(2, (0, 1), 3)),
                          (real4, _array(2, (0, 1), -1)), (real4, _array(2, (0, 1), 0, [1.0, nan])), (real4, _array(2, (0, 1), 0, [complex(0, inf), 1.0])),
                          (real4, _array(2, (0, 1), 0, [1.0, -inf])), (_lib.DdcLayout(0, 0, 65, 0, 0, 0), _array(2, (0, 1))),
                          (_lib.DdcLayout(3, 3, 4, 0, 0, 0), _array(2, (0, 1))), (None, _array(2, (0, 1))), (real4, None)):
        rc, handle = _create_raw(engine, layout, array)
        assert rc == INVALID and not handle
    good = _array(2, (3, 0), 1, [1.0, 1j, nan, inf])                              # (weights past K are not read)
    assert _create_raw(engine, real4, good)[0] == 0
    assert _create_raw(engine, _lib.DdcLayout(0, 0, 4, 99, 0, 0), good)[0] == 0          # (layout->lane is not read)
    for kw in (dict(D=0), dict(D=65), dict(taps=(1.0, nan)), dict(L=0), dict(L=1025), dict(L=2, D=129)):
        assert _create_raw(engine, real4, good, **kw)[0] == INVALID, kw
    h = C.c_void_p()
    cfg = _lib.DdcCfg(0, 1, 1, 0, 0, 1.0, C.cast((C.c_double * 1)(1.0), C.POINTER(C.c_double)))
    assert lib.sdr_ddc_create_array(engine._h, None, 1, C.byref(real4), C.byref(good), C.byref(h)) == INVALID
    assert lib.sdr_ddc_create_array(engine._h, C.byref(cfg), 1, C.byref(real4), C.byref(good), None) == INVALID

    layout, lanes = cases.packed_layout("K3_1bit_complex_6bit_frame", False), (4, 0, 2)
    raw = cases.stream(layout, 2000)
    w = cases.general_weights(3)
    R, n = np.zeros(18), C.c_int64(-7)
    Rp, np_ = R.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)
    wp = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    for shape in ((3, 2), (3, 2, 7)):
        quiet = engine.ddc_create(cases.config(shape, 0, 1.0, layout, ar.ArrayGeometry(lanes, w)))
        other = engine.ddc_create(cases.config(shape, 0, 1.0, ar.element_layout(layout, 0)))
        cfg = cases.config(shape, cases.FCWS["odd"], 24.0 * dcases.GOLD, layout, ar.ArrayGeometry(lanes, w, measure=True))
        ddc = engine.ddc_create(cfg)
        try:
            # the two new calls: a converter without an array, a converter without MEASURE, NULLs, weights that are not finite
            assert lib.sdr_ddc_array_weights(engine._h, other.handle, wp([1.0, 0.0] * 3)) == INVALID
            assert lib.sdr_ddc_array_covariance(engine._h, other.handle, Rp, np_, 0) == INVALID
            assert lib.sdr_ddc_array_covariance(engine._h, quiet.handle, Rp, np_, 1) == STATE
            assert lib.sdr_ddc_array_weights(engine._h, ddc.handle, None) == INVALID and lib.sdr_ddc_array_weights(engine._h, None, wp([1.0] * 6)) == INVALID
            assert lib.sdr_ddc_array_covariance(engine._h, ddc.handle, None, np_, 0) == INVALID and lib.sdr_ddc_array_covariance(engine._h, ddc.handle, Rp, None, 0) == INVALID
            for bad in ([1.0, 0.0, nan, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0, 0.0, -inf]):
                assert lib.sdr_ddc_array_weights(engine._h, ddc.handle, wp(bad)) == INVALID
            assert n.value == -7 and not np.any(R)
            # pushes: not whole bytes (K = 3 complex 1-bit: 6-bit frames, whole every 4), the ring's limits
            n_out = C.c_int64(-7)
            for call in (lib.sdr_ddc_push, lib.sdr_ddc_push_queue):
                for n_in in (1, 2, 3, 1999):
                    assert call(engine._h, ddc.handle, raw.ctypes.data, n_in, 0, C.byref(n_out)) == INVALID and n_out.value == -7
                assert call(engine._h, ddc.handle, raw.ctypes.data, -4, 0, C.byref(n_out)) == INVALID
                assert call(engine._h, ddc.handle, None, 4, 0, C.byref(n_out)) == INVALID
            for bad in (raw[:1000].view(np.int8), raw[:1000], raw[:1501][::2]):                  # (1000 bytes: 1333.3 frames)
                with pytest.raises(ValueError):
                    engine.ddc_push(ddc, bad, 0)
            with pytest.raises(SdrError) as err:
                engine.ddc_push(ddc, cases.stream(layout, 16000), 0)                               # more outputs than the ring holds
            assert err.value.status == RANGE
            with pytest.raises(SdrError) as err:
                engine.ddc_push(ddc, raw[:300].copy(), cap)
            assert err.value.status == RANGE
            assert engine.ddc_push(ddc, raw[:0].copy(), 0) == 0
            assert engine.ddc_out_count(ddc, 2000) == lcases.out_total(shape, 2000)
            assert np.array_equal(engine.iq_download(cap, 0), pattern)
            got_R, got_n = engine.ddc_array_covariance(ddc)
            assert got_n == 0 and not np.any(got_R)
            # ... and the next push gives what it would have given, with the weights it was made with
            got_n = engine.ddc_push(ddc, raw, 0)
            got = engine.iq_download(got_n, 0)
            want = ar.statement(cfg, [raw])
            check_ring(got, want, cfg, FMT_CI16, cases.x_max(cfg, raw), ("after the refusals", shape))
            got_R, got_count = engine.ddc_array_covariance(ddc)
            want_R, want_count = ar.covariance(raw, layout, lanes)
            assert got_count == want_count == 2000 and np.array_equal(got_R, want_R)
        finally:
            for d in (ddc, quiet, other):
                engine.ddc_destroy(d)
        engine.iq_upload(pattern, 0)
    bare = Engine(0)                                                                      # no ring allocated
    try:
        ddc = bare.ddc_create(cases.config((3, 2), 0, 1.0, layout, ar.ArrayGeometry(lanes, w)))
        with pytest.raises(SdrError) as err:
            bare.ddc_push(ddc, raw, 0)
        assert err.value.status == STATE
        bare.ddc_destroy(ddc)
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------ 5. the covariance
COV_GEOMETRIES = ["K2_int8_real", "K3_int16_complex_swapped", "K8_int8_complex"]


@pytest.mark.parametrize("name", COV_GEOMETRIES + ["K3_1bit_complex_6bit_frame", "K8_4bit_complex_68bit_frame"])
def test_covariance_of_integer_fields_equals_the_statement(engine, name):
    """n = 1, 63, 64, 65 and 1000 frames (a lane takes the frames 256 apart: lanes without a frame, one wave, a second wave's first
    lane), accumulated across pushes, read with and without `clear`, and across a reset."""
    layout, lanes = (cases.packed_layout(name, True), cases.PACKED[name][3]) if name in cases.PACKED else cases.GEOMETRIES[name]
    group = layout.frame_group
    counts = [cases.frames(v, layout) for v in (1, 63, 64, 65, 1000)]
    raw = cases.stream(layout, sum(counts))
    cfg = cases.config((3, 2), 0, 1.0, layout, ar.ArrayGeometry(lanes, measure=True))
    engine.iq_alloc(CAPACITY, FMT_CF64)
    ddc = engine.ddc_create(cfg)
    try:
        at, total_R, total_n = 0, 0, 0
        for k, count in enumerate(counts):
            part = cases.piece(raw, layout, at, count)
            engine.ddc_push(ddc, part, 0)
            want_R, want_n = ar.covariance(part, layout, lanes)
            total_R, total_n = total_R + want_R, total_n + want_n
            got_R, got_n = engine.ddc_array_covariance(ddc)                   # (without clear: the sums go on)
            assert got_n == total_n and np.array_equal(got_R, total_R), (name, count)
            assert got_R.dtype == np.complex128 and np.array_equal(got_R, got_R.conj().T)
            at += count
        whole_R, whole_n = ar.covariance(raw, layout, lanes)
        assert np.array_equal(total_R, whole_R) and total_n == whole_n == sum(counts)
        got_R, got_n = engine.ddc_array_covariance(ddc, clear=True)
        assert got_n == whole_n and np.array_equal(got_R, whole_R)
        got_R, got_n = engine.ddc_array_covariance(ddc)
        assert got_n == 0 and not np.any(got_R)
        engine.ddc_push(ddc, cases.piece(raw, layout, 0, counts[4]), 0)
        engine.ddc_reset(ddc)                                                 # a reset zeroes it too
        got_R, got_n = engine.ddc_array_covariance(ddc)
        assert got_n == 0 and not np.any(got_R)
        part = cases.piece(raw, layout, group, counts[3])
        engine.ddc_push(ddc, part, 0)
        want_R, want_n = ar.covariance(part, layout, lanes)
        got_R, got_n = engine.ddc_array_covariance(ddc)
        assert got_n == want_n and np.array_equal(got_R, want_R) and np.any(want_R != 0)
    finally:
        engine.ddc_destroy(ddc)


def test_covariance_of_int16_rails_is_beyond_any_int32_partial(engine):
    """Every component of every element -32768 over 70 000 frames: every entry of R is 2^31 * 70 000 (and its imaginary part 0)."""
    layout, lanes, n = dc.InputLayout(dc.FIELD_INT16, 0, 6, 0, True), (4, 0, 2), 70000
    raw = np.full(6 * n, -32768, dtype=np.int16)
    cfg = cases.config((1, 1), 0, 2.0 ** -16, layout, ar.ArrayGeometry(lanes, measure=True))
    engine.iq_alloc(lcases.ring_capacity(n), FMT_CI16)
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == n
        got_R, got_n = engine.ddc_array_covariance(ddc)
    finally:
        engine.ddc_destroy(ddc)
    assert got_n == n and np.array_equal(got_R, np.full((3, 3), float(2 ** 31 * n) + 0j)) and 2 ** 31 * n > 2 ** 47
    want_R, _ = ar.covariance(raw, layout, lanes)
    assert np.array_equal(got_R, want_R)


def test_covariance_of_float32_fields_within_the_derived_bound_and_reproducible(engine):
    layout, lanes = dc.InputLayout(dc.FIELD_FLOAT32, 0, 6, 0, True), (4, 0, 2)
    raw = lcases.fractional(True, 3 * cases.N_FRAMES)
    cfg = cases.config((3, 2), 0, 1.0, layout, ar.ArrayGeometry(lanes, measure=True))
    engine.iq_alloc(CAPACITY, FMT_CF64)
    runs = []
    for _ in range(2):
        ddc = engine.ddc_create(cfg)
        try:
            engine.ddc_push(ddc, cases.piece(raw, layout, 0, 1001), 0)
            engine.ddc_push(ddc, cases.piece(raw, layout, 1001, cases.N_FRAMES - 1001), 0)
            runs.append(engine.ddc_array_covariance(ddc))
        finally:
            engine.ddc_destroy(ddc)
    (R, n), (R2, n2) = runs
    assert n == n2 == cases.N_FRAMES and np.array_equal(R.view(np.uint64), R2.view(np.uint64))      # the same pushes, the same bits
    want_R, want_n = ar.covariance(raw, layout, lanes)
    bound_re, bound_im = ar.covariance_bound(raw, layout, lanes)
    err_re, err_im = np.abs(R.real - want_R.real), np.abs(R.imag - want_R.imag)
    print(f"max |R - statement|: re {err_re.max():.3e} (bound {bound_re.min():.3e}), im {err_im.max():.3e} (bound {bound_im.min():.3e})")
    assert np.all(err_re <= bound_re) and np.all(err_im <= bound_im) and np.all(R.diagonal().imag == 0) and np.any(R.imag != 0)


# ------------------------------------------------------------------------------------------------ 6. the old constructors
def test_converters_of_the_old_constructors_make_the_launches_they_made(engine):
    """sdr_prof_read launch counts of one push of a converter of sdr_ddc_create, _rational and _layout: one converter kernel, one
    history kernel, no covariance pass -- and of an array converter the same plus, with MEASURE alone, one covariance pass."""
    layout, lanes = cases.GEOMETRIES["K3_int8_complex"]
    raw = cases.stream(layout)
    plain = cases.combined_integers(raw, layout, lanes, cases.quarter_weights(3))
    engine.iq_alloc(CAPACITY, FMT_CI16)
    element = ar.element_layout(layout, 2)
    made = [(cases.config((33, 2), 0, 1.0), plain, "ddc_kernel", 0), (cases.config((3, 2, 7), 0, 1.0), plain, "resample_kernel", 0),
            (cases.config((33, 2), 0, 1.0, element), raw, "ddc_kernel", 0), (cases.config((3, 2, 7), 0, 1.0, element), raw, "resample_kernel", 0),
            (cases.config((33, 2), 0, 1.0, layout, ar.ArrayGeometry(lanes)), raw, "ddc_kernel", 0),
            (cases.config((3, 2, 7), 0, 1.0, layout, ar.ArrayGeometry(lanes, measure=True)), raw, "resample_kernel", 1)]
    engine.prof_enable(True)
    try:
        for cfg, data, kernel, cov in made:
            ddc = engine.ddc_create(cfg)
            try:
                engine.prof_reset()
                engine.ddc_push(ddc, data, 0)
                engine.sync()
                counts = {name: engine.prof_read(name)[1] for name in ("ddc_kernel", "resample_kernel", "ddc_history_kernel", "ddc_array_cov_kernel", "call_ddc_push")}
            finally:
                engine.ddc_destroy(ddc)
            other = "resample_kernel" if kernel == "ddc_kernel" else "ddc_kernel"
            assert counts[kernel] == 1 and counts[other] == 0 and counts["ddc_history_kernel"] == 1 and counts["ddc_array_cov_kernel"] == cov, (kernel, counts)
            assert engine.prof_read("")[1] == counts[kernel] + counts["ddc_history_kernel"] + counts["ddc_array_cov_kernel"] + counts["call_ddc_push"], counts
    finally:
        engine.prof_enable(False)


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_a_jammed_recording_is_acquired_through_the_array_and_not_on_one_element(engine, tmp_path):
    """array_cases.jammed_recording (4 elements, int16, 4 MHz; jammer 20 dB above an element's noise) through ChannelManager with
    the [RFSIGNAL] keys.  On element 0 alone (fixed weights e_0) the acquisition falls under the plugin's ratio threshold at a wrong
    bin and code phase (the oracle on the statement's ring: [23, 579], ratio 1.454); with array_mode = power_inversion over the first
    2 ms it finds bin 13, sample 2826 with ratio 5.777 (the oracle on the statement's ring: tests/test_array.py).  Either way the
    device's ring equals the statement's byte for byte, and the trained weights are the host's solve of the statement's covariance."""
    import packed_cases
    from sydr_amd.signal.iqsource import RFSignal
    raw, ms, per_ms = cases.jammed_recording(), cases.E2E_MS, int(cases.E2E_FS * 1e-3)
    path = tmp_path / "array.bin"
    raw.tofile(path)
    R, n = ar.covariance(cases.piece(raw, cases.E2E_LAYOUT, 0, cases.E2E_TRAIN_MS * per_ms), cases.E2E_LAYOUT, cases.E2E_LANES)
    want_w = ar.power_inversion(R, n)
    found = {}
    for mode, more in (("element0", {}), ("power_inversion", dict(array_mode="power_inversion", array_train_ms=cases.E2E_TRAIN_MS))):
        sig = RFSignal(cases.e2e_conf(path, **more))
        got, mgr = packed_cases.receive(sig, engine, prns=[cases.E2E_PRN], cfg=packed_cases.kaplan_config(), ms=ms, mode="ticks")
        try:
            ring = engine.iq_download(ms * per_ms, 0)
            weights = getattr(mgr, "arrayWeights", sig.frontEnd.config.array.weights)
            cov = mgr.arrayCovariance()
        finally:
            mgr.close()
        acq = [p for tick in got for p in tick if p["type"] is ChannelMessage.ACQUISITION_UPDATE]
        assert len(acq) == 1
        found[mode] = ([int(acq[0]["frequency_idx"]), int(acq[0]["code_idx"])], float(acq[0]["peak_ratio"]))
        print(mode, found[mode], "weights", weights)
        cfg = RFSignal(cases.e2e_conf(path)).frontEnd.config
        cfg.array.weights = weights
        assert np.array_equal(ring, ar.statement(cfg, [raw], FMT_CI16)) and np.any(ring != 0), mode
        if mode == "power_inversion":
            assert np.array_equal(weights, want_w)
            whole_R, whole_n = ar.covariance(raw, cases.E2E_LAYOUT, cases.E2E_LANES)
            assert cov[1] == whole_n == ms * per_ms and np.array_equal(cov[0], whole_R)
            gain = abs(np.vdot(weights, cases.E2E_JAMMER_DIRECTION)) ** 2 / abs(weights[0]) ** 2
            print(f"output gain towards the jammer over the reference element's: {10 * np.log10(gain):.1f} dB")
        else:
            assert cov is None
    truth = [13, 2826]
    assert found["element0"][1] < 1.5 and found["element0"][0] != truth, found
    assert found["power_inversion"][0] == truth and found["power_inversion"][1] > 4.0, found
