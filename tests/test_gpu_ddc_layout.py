"""Input layouts of the device's down-converter (sdr_ddc_create_layout; packed, float32 and interleaved recordings decoded where
ddc_kernel / resample_kernel load their inputs) against the converter of the four old formats on the host-decoded stream.

Every such comparison demands equality of every ring byte: behind the decode it is the same arithmetic on the same doubles, so
no tie condition is needed.  Only the fractional float32 streams, which no old format holds, are held to the NumPy statement
within `dc.tolerance` (derived, not measured: (Tp + 16) * 2^-53 * sum|h| * max|x| * gain, plus 2^-24 |v| on a cf32 ring)."""
import ctypes as C

import numpy as np
import pytest

import downconvert_cases as dcases
import ddc_layout_cases as cases
from test_gpu_downconvert import check_ring

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI8, FMT_CI16, Engine, layout_struct
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt
from sydr_amd.signal import packing as pk
from sydr_amd.utils.enumerations import ChannelMessage

pytestmark = pytest.mark.gpu

INVALID, RANGE, STATE = -1, -5, -6
RING_DTYPE = dcases.RING_DTYPE
CAPACITY = cases.ring_capacity(2 * cases.N_FRAMES)              # (every shape's outputs of N_FRAMES inputs: 3 / 2 of them at most)


def same_ring(engine, layout, raw, shape, fcw, ring_fmt, what, plain=None):
    """The layout's converter on `raw` against the old-format converter on the decoded stream: equal ring bytes.  -> the ring"""
    n = layout.frames_in(raw.nbytes)
    n_out = cases.out_total(shape, n)
    gain = cases.gain_for(layout, ring_fmt)
    plain = cases.decoded(raw, layout) if plain is None else plain
    got = cases.push_all(engine, cases.config(shape, fcw, gain, layout=layout), raw, n_out)
    want = cases.push_all(engine, cases.config(shape, fcw, gain, cases.old_format(layout)), plain, n_out)
    bad = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (what, bad.size, bad[:5])
    assert np.any(want != 0), what
    return got


# ------------------------------------------------------------------------------------------------ 1. packed inputs
PACKED = [(bits, cplx, msb, None) for bits in (1, 2, 4) for cplx in (False, True) for msb in (False, True)]
PACKED += [(2, False, False, cases.ODD_TABLE), (2, True, True, cases.ODD_TABLE)]


@pytest.mark.parametrize("bits,cplx,msb,levels", PACKED,
                         ids=[f"{b}bit_{'complex' if c else 'real'}_{'msb' if m else 'lsb'}{'_table' if t else ''}" for b, c, m, t in PACKED])
def test_packed_input_gives_the_ring_of_the_unpacked_bytes(engine, bits, cplx, msb, levels):
    layout = cases.packed_layout(bits, cplx, msb, levels)
    raw = cases.stream(layout)
    plain = cases.decoded(raw, layout)
    f = pk.unpack(raw, pk.Packing(bits, levels, msb))
    assert np.array_equal(plain, f) and len(np.unique(f)) == 1 << bits            # (the stream IS unpack's, every level in it)
    rings = [FMT_CI8, FMT_CF64] + ([FMT_CI16] if (bits, cplx, msb) == (2, False, False) else []) + ([FMT_CF32] if (bits, cplx, msb) == (4, True, True) else [])
    for ring_fmt in rings:
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.SHAPES:
            for name, fcw in cases.FCWS.items():
                same_ring(engine, layout, raw, shape, fcw, ring_fmt, (dcases.RING_NAMES[ring_fmt], shape, name), plain)


# ------------------------------------------------------------------------------------------------ 2. frames
FRAME_SHAPES = [(1, 1), (33, 2), (3, 2, 7)]


@pytest.mark.parametrize("lane", [0, 2])
@pytest.mark.parametrize("swap", [False, True], ids=["iq", "qi"])
def test_one_of_two_complex_streams_of_an_int16_file(engine, lane, swap):
    layout = dc.InputLayout(dc.FIELD_INT16, 0, 4, lane, True, swap)
    raw = cases.stream(layout)
    a, b = raw[lane::4], raw[lane + 1::4]
    plain = np.empty(2 * cases.N_FRAMES, dtype=np.int16)                            # (de-interleaved here, not by `decode`)
    plain[0::2], plain[1::2] = (b, a) if swap else (a, b)
    for ring_fmt in (FMT_CI16, FMT_CF64):
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in FRAME_SHAPES:
            same_ring(engine, layout, raw, shape, cases.FCWS["odd"], ring_fmt, (dcases.RING_NAMES[ring_fmt], shape), plain)


FRAMES = [cases.packed_layout(2, stride=4, lane=0), cases.packed_layout(2, stride=4, lane=3), cases.packed_layout(2, complex=True, stride=4, lane=1, swap_iq=True),
          cases.packed_layout(1, stride=3, lane=1), cases.packed_layout(1, stride=3, lane=1, msb_first=True),
          cases.packed_layout(4, complex=True, stride=3, lane=1), cases.packed_layout(4, complex=True, stride=3, lane=1, msb_first=True),
          dc.InputLayout(dc.FIELD_INT8, 0, 3, 2), dc.InputLayout(dc.FIELD_FLOAT32, 0, 3, 1, True), dc.InputLayout(dc.FIELD_INT16, 0, 3, 1, True)]


@pytest.mark.parametrize("layout", FRAMES, ids=repr)
def test_frames_wider_than_the_stream_and_frames_that_are_not_whole_bytes(engine, layout):
    """2-bit stride 4 (a byte is one frame); 1-bit stride 3 lane 1 real and 4-bit stride 3 lane 1 complex (frames straddle
    bytes; I in the high nibble of one byte, Q in the low nibble of the next); int16 and float32 pairs at odd field indices."""
    raw = cases.stream(layout)
    for ring_fmt in (FMT_CI8, FMT_CF64):
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in FRAME_SHAPES:
            same_ring(engine, layout, raw, shape, cases.FCWS["odd"], ring_fmt, (dcases.RING_NAMES[ring_fmt], shape))


@pytest.mark.parametrize("field,cplx", [(dc.FIELD_INT8, False), (dc.FIELD_INT16, False), (dc.FIELD_INT8, True), (dc.FIELD_INT16, True)])
def test_the_four_plain_layouts_are_the_four_old_formats(engine, field, cplx):
    layout = dc.InputLayout(field, complex=cplx)
    raw = cases.stream(layout)
    for ring_fmt in dcases.RING_FORMATS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in FRAME_SHAPES:
            same_ring(engine, layout, raw, shape, cases.FCWS["odd"], ring_fmt, (dcases.RING_NAMES[ring_fmt], shape), raw)     # the SAME array


# ------------------------------------------------------------------------------------------------ 3. float32
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_integer_valued_float32_gives_the_ring_of_int16(engine, cplx):
    layout = dc.InputLayout(dc.FIELD_FLOAT32, complex=cplx)
    raw = cases.stream(layout)
    plain = raw.astype(np.int16)
    assert np.array_equal(plain.astype(np.float32), raw)
    for ring_fmt in dcases.RING_FORMATS:
        engine.iq_alloc(CAPACITY, ring_fmt)
        for shape in cases.SHAPES:
            same_ring(engine, layout, raw, shape, cases.FCWS["odd"], ring_fmt, (dcases.RING_NAMES[ring_fmt], shape), plain)


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("ring_fmt", [FMT_CF64, FMT_CF32], ids=["ring_cf64", "ring_cf32"])
def test_fractional_float32_against_the_statement(engine, ring_fmt, cplx):
    layout = dc.InputLayout(dc.FIELD_FLOAT32, complex=cplx)
    raw = cases.fractional(cplx)
    x = raw.astype(np.float64)
    x_max = float(np.max(np.hypot(x[0::2], x[1::2]))) if cplx else float(np.max(np.abs(x)))
    engine.iq_alloc(CAPACITY, ring_fmt)
    for shape in cases.SHAPES:
        cfg = cases.config(shape, cases.FCWS["odd"], 1000.0, layout=layout)
        v = dc.statement(cfg, [raw])
        got = cases.push_all(engine, cfg, raw, v.size)
        check_ring(got, v, cfg, ring_fmt, x_max, ("float32", cplx, dcases.RING_NAMES[ring_fmt], shape))


# ------------------------------------------------------------------------------------------------ 4. the cut
CUTS = [(cases.packed_layout(2), (33, 2)), (cases.packed_layout(1, stride=3, lane=1), (33, 2)), (dc.InputLayout(dc.FIELD_FLOAT32, complex=True), (512, 16)),
        (cases.packed_layout(4, complex=True), (1, 1)), (cases.packed_layout(2), (250, 341, 1500)),
        # (frames of whole bytes behind a resampler: pushes of exactly 1, Tp - 2, Tp - 1 and Tp = 3 frames, none rounded up)
        (dc.InputLayout(dc.FIELD_INT8, 0, 8, 5, True), (3, 2, 7))]


@pytest.mark.parametrize("layout,shape", CUTS, ids=lambda v: repr(v) if isinstance(v, dc.InputLayout) else cases.shape_id(v))
def test_the_ring_does_not_depend_on_how_the_bytes_were_cut(engine, layout, shape):
    raw = cases.stream(layout)
    n = cases.N_FRAMES
    total = cases.out_total(shape, n)
    cfg = cases.config(shape, cases.FCWS["odd"], cases.gain_for(layout, FMT_CF64), layout=layout)
    lengths = cases.rounded_lengths(cases.phase_taps(shape), layout.frame_group)
    assert 0 in lengths                                                         # (and pushes shorter than the history: 1, 2, 3 rounded up)
    engine.iq_alloc(CAPACITY, FMT_CF64)
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, raw, 0) == total
        whole = engine.iq_download(total, 0)
        engine.iq_upload(np.zeros(2 * CAPACITY), 0)
        engine.ddc_reset(ddc)
        st = dc.Statement(cfg)
        at = seen = 0
        for piece in cases.cut_bytes(raw, layout, lengths):
            n_in = layout.frames_in(piece.nbytes)
            want = st.out_count(n_in)
            assert engine.ddc_out_count(ddc, n_in) == want
            assert engine.ddc_push(ddc, np.ascontiguousarray(piece), at) == want
            st.n_seen += n_in                                                     # (the statement's count alone: its outputs are not needed)
            at, seen = at + want, seen + n_in
        assert at == total and seen == n
        pieces = engine.iq_download(total, 0)
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(pieces.view(np.uint8), whole.view(np.uint8)), np.flatnonzero(pieces != whole)[:8]
    assert np.any(whole != 0)


# ------------------------------------------------------------------------------------------------ 5. refusals
def _create_raw(engine, layout, D=1, taps=(1.0,), n_taps=None, flags=0, gain=1.0, L=1, in_fmt=77):
    t = (C.c_double * max(len(taps), 1))(*taps)
    cfg = _lib.DdcCfg(in_fmt, D, len(taps) if n_taps is None else n_taps, flags, 0, gain, C.cast(t, C.POINTER(C.c_double)))
    h = C.c_void_p()
    rc = _lib.load().sdr_ddc_create_layout(engine._h, C.byref(cfg), L, C.byref(layout) if layout is not None else None, C.byref(h))
    if rc == 0:
        _lib.load().sdr_ddc_destroy(engine._h, h)
    return rc, h.value


def _status(fn):
    with pytest.raises(SdrError) as err:
        fn()
    return err.value.status


def test_refusals_leave_the_ring_and_the_converter_as_they_were(engine):
    cap = 8192
    engine.iq_alloc(cap, FMT_CI16)
    pattern = np.random.default_rng(cases.SEED + 6).integers(-3000, 3000, 2 * cap).astype(np.int16)
    engine.iq_upload(pattern, 0)
    good = _lib.DdcLayout(3, 2, 1, 0, 0, 0)
    # every bad layout
    for kw in (dict(field=4), dict(field=-1), dict(field=3, bits=0), dict(field=3, bits=3), dict(field=3, bits=8), dict(bits=1), dict(field=1, bits=2),
               dict(field=2, bits=4), dict(stride=0), dict(stride=65), dict(stride=-1), dict(lane=-1), dict(lane=1), dict(stride=2, lane=1, flags=1),
               dict(flags=1), dict(stride=2, flags=2), dict(stride=2, flags=4), dict(field=1, stride=2, flags=5), dict(field=2, stride=2, flags=4),
               dict(stride=2, flags=8), dict(stride=2, flags=-1), dict(reserved=1)):
        args = dict(field=0, bits=0, stride=1, lane=0, flags=0, reserved=0)
        args.update(kw)
        rc, handle = _create_raw(engine, _lib.DdcLayout(*[args[k] for k in ("field", "bits", "stride", "lane", "flags", "reserved")]))
        assert rc == INVALID and not handle, kw
    assert _create_raw(engine, None)[0] == INVALID
    # cfg errors as sdr_ddc_create's and sdr_ddc_create_rational's; cfg->in_fmt is not read
    for kw in (dict(D=0), dict(D=65), dict(D=-1), dict(n_taps=0), dict(taps=(0.001,) * 513), dict(taps=(1.0, float("nan"))), dict(taps=(float("inf"),)),
               dict(gain=float("nan")), dict(gain=float("-inf")), dict(flags=1), dict(L=0), dict(L=1025), dict(L=2, D=129), dict(L=2, taps=(0.001,) * 1025)):
        rc, handle = _create_raw(engine, good, **kw)
        assert rc == INVALID and not handle, kw
    assert _create_raw(engine, good, D=64, taps=(0.001,) * 512)[0] == 0 and _create_raw(engine, good, in_fmt=-5)[0] == 0
    assert _create_raw(engine, _lib.DdcLayout(3, 4, 64, 62, 7, 0), L=2, D=3, taps=(0.5,) * 9)[0] == 0
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _lib.DdcCfg(0, 1, 1, 0, 0, 1.0, C.cast((C.c_double * 1)(1.0), C.POINTER(C.c_double)))
    assert lib.sdr_ddc_create_layout(engine._h, None, 1, C.byref(good), C.byref(h)) == INVALID
    assert lib.sdr_ddc_create_layout(engine._h, C.byref(cfg), 1, C.byref(good), None) == INVALID
    # pushes: a packed push that is not whole bytes (through the C call: the wrapper would refuse the array first), the ring's limits
    for shape in ((3, 2), (3, 2, 7)):
        layout = cases.packed_layout(1, stride=3, lane=1)
        raw = cases.stream(layout, 4000)
        new_cfg = cases.config(shape, cases.FCWS["odd"], dcases.GOLD * 24.0, layout=layout)
        ddc = engine.ddc_create(new_cfg)
        try:
            n_out = C.c_int64(-7)
            for call in (lib.sdr_ddc_push, lib.sdr_ddc_push_queue):
                for n_in in (1, 7, 9, 3999):
                    assert call(engine._h, ddc.handle, raw.ctypes.data, n_in, 0, C.byref(n_out)) == INVALID and n_out.value == -7
                assert call(engine._h, ddc.handle, raw.ctypes.data, -8, 0, C.byref(n_out)) == INVALID
                assert call(engine._h, ddc.handle, None, 8, 0, C.byref(n_out)) == INVALID
            for bad in (raw[:1000].view(np.int8), raw[:1000], raw[:1501][::2], raw[:1500].reshape(-1, 3)):      # (1000 bytes: 2666.67 frames)
                with pytest.raises(ValueError):
                    engine.ddc_push(ddc, bad, 0)
                with pytest.raises(ValueError):
                    engine.ddc_push_queue(ddc, bad, 0)
            big = cases.stream(layout, 32000)
            assert _status(lambda: engine.ddc_push(ddc, big, 0)) == RANGE                 # more outputs than the ring holds
            assert _status(lambda: engine.ddc_push(ddc, raw[:300].copy(), cap)) == RANGE
            assert _status(lambda: engine.ddc_push_queue(ddc, raw[:300].copy(), -1)) == RANGE
            assert engine.ddc_push(ddc, raw[:0].copy(), 0) == 0                           # n_in = 0 succeeds and writes nothing
            assert engine.ddc_out_count(ddc, 4000) == cases.out_total(shape, 4000)        # (no refused push has advanced the converter)
            assert np.array_equal(engine.iq_download(cap, 0), pattern)
            # ... and its next push gives what it would have given
            got_n = engine.ddc_push(ddc, raw, 0)
            got = engine.iq_download(got_n, 0)
        finally:
            engine.ddc_destroy(ddc)
        want = cases.push_all(engine, cases.config(shape, new_cfg.fcw, new_cfg.gain, dc.IN_R8), cases.decoded(raw, layout), got_n)
        assert np.array_equal(got, want) and np.any(want != 0)
        engine.iq_upload(pattern, 0)
    bare = Engine(0)                                                                      # no ring allocated
    try:
        ddc = bare.ddc_create(cases.config((3, 2), 0, 1.0, layout=cases.packed_layout(2)))
        assert _status(lambda: bare.ddc_push(ddc, np.zeros(25, dtype=np.uint8), 0)) == STATE
        bare.ddc_destroy(ddc)
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------ 6. push_queue
@pytest.mark.parametrize("page_locked", [False, True], ids=["pageable", "page_locked"])
def test_push_queue_equals_push_for_a_packed_input(engine, page_locked):
    layout = cases.packed_layout(2, complex=True)
    raw = cases.stream(layout)
    n, ring_fmt = cases.N_FRAMES, FMT_CI16
    cfg = cases.config((33, 2), cases.FCWS["odd"], cases.gain_for(layout, ring_fmt), layout=layout)
    engine.iq_alloc(16384, ring_fmt)
    ddc = engine.ddc_create(cfg)
    block = engine.host_alloc(raw.size, np.uint8) if page_locked else None
    try:
        n_out = engine.ddc_push(ddc, raw, 0)
        want = engine.iq_download(n_out, 0)
        engine.iq_upload(np.zeros(2 * 16384, dtype=np.int16), 0)
        engine.ddc_reset(ddc)
        src = block if page_locked else raw.copy()
        src[:] = raw
        at, step = 0, layout.bytes_for(4004)
        for lo in range(0, raw.size, step):                # several pushes in flight behind each other, no wait between them
            at += engine.ddc_push_queue(ddc, src[lo:lo + step], at)
        engine.sync()
        assert at == n_out == n // 2
        assert np.array_equal(engine.iq_download(n_out, 0), want) and np.any(want != 0)
    finally:
        engine.ddc_destroy(ddc)
        if block is not None:
            engine.host_free(block)


# ------------------------------------------------------------------------------------------------ 7. with a mitigator
@pytest.mark.parametrize("ring_fmt", [FMT_CI8, FMT_CF64], ids=["ring_ci8", "ring_cf64"])
def test_a_mitigator_behind_a_packed_input(engine, ring_fmt):
    """2-bit real input with a blanker and a 64-point excisor: the ring and the counters of the IN_R8 converter with the same
    mitigator on the unpacked stream."""
    layout = cases.packed_layout(2)
    raw = cases.stream(layout)
    plain = cases.decoded(raw, layout)
    shape, gain = (33, 2), 8.0 * dcases.GOLD
    new_cfg, old_cfg = cases.config(shape, cases.FCWS["odd"], gain, layout=layout), cases.config(shape, cases.FCWS["odd"], gain, dc.IN_R8)
    v = dc.statement(old_cfg, [plain])
    # (the blanker's level: the statement's 99th percentile of |v|, so that about one output in a hundred triggers it)
    mit = mt.MitigationConfig(float(np.quantile(np.abs(v), 0.99)), 2, 5, 64, mt.excision_limits(v[:8192], 64, 3.0))
    n_out = v.size
    engine.iq_alloc(cases.ring_capacity(n_out), ring_fmt)
    results = []
    for cfg, data in ((new_cfg, raw), (old_cfg, plain)):
        ddc = engine.ddc_create(cfg)
        try:
            engine.ddc_mitigate(ddc, mit)
            assert engine.ddc_delay(ddc) == 64 + 2
            half = layout.bytes_for(10000) if cfg is new_cfg else 10000                   # (two pushes: the mitigator's state is carried)
            assert engine.ddc_push(ddc, data[:half], 0) + engine.ddc_push(ddc, data[half:], 5000) == n_out
            results.append((engine.iq_download(n_out, 0), engine.ddc_mitigation_stats(ddc)))
        finally:
            engine.ddc_destroy(ddc)
    (got, got_stats), (want, want_stats) = results
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert got_stats == want_stats and want_stats.n_triggers > 0 and want_stats.n_bins_excised > 0 and want_stats.n_outputs == n_out


# ------------------------------------------------------------------------------------------------ 8. a NaN
def test_a_nan_changes_only_the_outputs_whose_window_contains_it(engine):
    shape, at = (33, 2), 10001
    layout = dc.InputLayout(dc.FIELD_FLOAT32)
    clean = cases.fractional(False).copy()
    clean[at] = 0.0
    dirty = clean.copy()
    dirty[at] = np.nan
    cfg = cases.config(shape, cases.FCWS["odd"], 1000.0, layout=layout)
    n_out = cases.out_total(shape, cases.N_FRAMES)
    engine.iq_alloc(CAPACITY, FMT_CF64)
    want = cases.push_all(engine, cfg, clean, n_out)
    got = cases.push_all(engine, cfg, dirty, n_out)
    m = np.repeat(np.arange(n_out), 2)
    inside = (2 * m >= at) & (2 * m - 32 <= at)                                           # output m reads inputs 2 m - 32 .. 2 m
    assert inside.sum() == 2 * 16
    assert np.array_equal(got[~inside].view(np.uint64), want[~inside].view(np.uint64)) and np.all(np.isfinite(want))
    # ... and across pushes: the NaN in the history of the next push reaches no further
    ddc = engine.ddc_create(cfg)
    try:
        cutat = at + 5
        assert engine.ddc_push(ddc, dirty[:cutat], 0) + engine.ddc_push(ddc, dirty[cutat:], -(-cutat // 2)) == n_out
        pieces = engine.iq_download(n_out, 0)
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(pieces[~inside].view(np.uint64), want[~inside].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 9. end to end
def test_search_and_receiver_over_the_packed_real_recording(engine, tmp_path):
    """downconvert_cases.real_if_recording() quantised to 2 bits and packed four samples to a byte, through
    RFSignal(sample_format="packed") and the device's converter: the ring equals the statement's ci8 output byte for byte (no
    statement component lies within the tolerance band of a tie: 0 of 491 040, max |out| 37), sdr_pcps finds the oracle's peak
    on it (the oracle on the statement's output: bin 13, sample 2899, ratio 9.1), and a ChannelManager over the packed file
    hands out, packet for packet, what a manager over the statement's output stored as a plain ci8 file hands out."""
    from oracle import sydr_oracle as orc
    import packed_cases
    sig, conv_sig, converted = cases.write_packed_and_converted(tmp_path)
    packed, few = cases.packed_real_recording()
    ms, fs, prn = dcases.REAL_MS, dcases.FS_REAL / 2, dcases.SATELLITE["prn"]
    n = orc.samples_per_code(fs)
    cfg = sig.frontEnd.config
    assert cfg.layout == cases.packed_layout(2) and cfg.gain == 16.0 and sig.frontEnd.outputBits == 8
    v = dc.statement(cfg, [packed])
    assert converted.size == 2 * ms * n == 491040 and dc.ambiguous(v, dc.tolerance(cfg, 3.0)) == 0 and int(np.max(np.abs(converted))) == 37
    engine.iq_alloc(ms * n, FMT_CI8)
    ddc = engine.ddc_create(cfg)
    try:
        assert engine.ddc_push(ddc, sig.samples(0, ms * 8184), 0) == ms * n
    finally:
        engine.ddc_destroy(ddc)
    assert np.array_equal(engine.iq_download(ms * n, 0), converted)
    engine.code_slots(1)
    engine.load_gps_code(0, prn)
    pb, pc, pr, _ = engine.pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)
    rf = orc.iq_to_complex(converted[:2 * n].astype(np.float64)).reshape(1, -1)
    cmap = orc.pcps_map(rf, 0.0, fs, orc.code_spectrum(orc.gold_code(prn), fs), 5000.0, 250.0, n)
    peak, ratio = orc.two_peak_compare(cmap, n, round(fs / orc.CODE_RATE))
    assert peak == [13, 2899] and abs(ratio - 9.1) < 0.05, (peak, ratio)
    assert [int(pb[0]), int(pc[0])] == peak and abs(pr[0] - ratio) <= 1e-12 * ratio, (pb, pc, pr, peak, ratio)
    kcfg = packed_cases.kaplan_config()
    got, mgr = packed_cases.receive(sig, engine, prns=[prn], cfg=kcfg, ms=ms, mode="ticks")
    ring_fmt, ring_size = mgr.sharedBuffer.fmt, mgr.sharedBuffer.maxSize
    mgr.close()
    want, want_mgr = packed_cases.receive(conv_sig, engine, prns=[prn], cfg=kcfg, ms=ms, mode="ticks")
    want_mgr.close()
    assert ring_fmt == FMT_CI8 and ring_size == 100 * n
    assert len(got) == len(want) == ms
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, k
    assert packed_cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 1 and packed_cases.count(got) > 40
