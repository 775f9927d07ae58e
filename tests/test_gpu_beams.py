"""Beams of the device's array converters (sdr_ddc_beam_attach, _beam_weights, _beam_count, _beams_clear): several weight sets
over ONE push, beam b >= 1 into the ring of an engine of its own.

The definition needs no tolerance: a beam's ring holds, byte for byte, what an independent converter with that beam's weights
on an engine of its own writes -- the parent's path, `solo` below.  Every comparison here is equality of bytes, of WHOLE rings
filled with a pattern first, so that nothing outside the written span may change either.  Against the NumPy statement
(`beams_statement`, quantised by `downconvert.quantise`) bytes are equal where the converter's own tests hold the statement bit
for bit: with fcw = 0 (no phasor; with a mixer the device's sine differs from NumPy's in the last bit, which
test_gpu_array.py holds within `dc.tolerance`) -- so every case of the sweep runs twice, with the odd frequency word against the
independent converters and with fcw = 0 against both."""
import ctypes as C

import numpy as np
import pytest

import array_cases as acases
import beams_cases as cases
import ddc_layout_cases as lcases
import downconvert_cases as dcases

from sydr_amd import SdrError, _lib
from sydr_amd.engine import FMT_CF64, FMT_CI8, FMT_CI16, Engine, make_items
from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6
MAX_BEAMS = 16


@pytest.fixture(scope="module")
def targets():
    """The engines of beams 1 .. 15, and one more for what must be refused."""
    made = [Engine(0) for _ in range(MAX_BEAMS)]
    yield made
    for e in made:
        e.close()


@pytest.fixture(scope="module")
def solo():
    """The engine of the independent converters."""
    e = Engine(0)
    yield e
    e.close()


def same_bytes(got, want, what):
    assert got.dtype == want.dtype and got.size == want.size, what
    bad = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (what, bad.size, bad[:5])


def set_weights(leader, ddc, cfg, beam, w):
    if beam:
        leader.ddc_beam_weights(ddc, beam, w)
    elif cases.is_stap(cfg):
        leader.ddc_stap_weights(ddc, w)
    else:
        leader.ddc_array_weights(ddc, w)


def prepare(engines, ring_fmts, capacity, seed=0):
    for e, fmt in zip(engines, ring_fmts):
        e.iq_alloc(capacity, fmt)
        e.iq_upload(cases.fill(fmt, capacity, seed), 0)


def feed(leader, ddc, cfg, pushes, capacity, offset=0, weights_at=None, queue=False):
    """The pushes one behind the other from ring sample `offset` on (modulo the ring), the weight changes of weights_at =
    {push index: {beam: weights}} in front of theirs -> the outputs written."""
    at = offset
    for k, raw in enumerate(pushes):
        for beam, w in (weights_at or {}).get(k, {}).items():
            set_weights(leader, ddc, cfg, beam, w)
        at += (leader.ddc_push_queue if queue else leader.ddc_push)(ddc, raw, at % capacity)
    return at - offset


def fan_out(engines, cfg, weight_sets, ring_fmts, pushes, capacity, offset=0, weights_at=None, queue=False, seed=0):
    """One converter on engines[0] with beam b on engines[b] -> (every beam's whole ring, the outputs written).  With one
    engine and one weight set this is the parent's path: no beam call is made."""
    engines = engines[:len(weight_sets)]
    prepare(engines, ring_fmts, capacity, seed)
    leader = engines[0]
    cfg = cases.with_weights(cfg, weight_sets[0])
    ddc = leader.ddc_create(cfg)
    try:
        for b in range(1, len(weight_sets)):
            assert leader.ddc_beam_attach(ddc, engines[b], weight_sets[b]) == b
        if len(weight_sets) > 1:
            assert leader.ddc_beam_count(ddc) == len(weight_sets)
        n = feed(leader, ddc, cfg, pushes, capacity, offset, weights_at, queue)
        if queue:
            leader.sync()
        return [e.iq_download(capacity, 0) for e in engines], n
    finally:
        leader.ddc_destroy(ddc)


def independent(solo, cfg, weight_sets, ring_fmts, pushes, capacity, offset=0, weights_at=None, seed=0):
    """Every beam by a converter of its own on `solo`, one after the other -> the whole rings."""
    rings = []
    for b, (w, fmt) in enumerate(zip(weight_sets, ring_fmts)):
        changes = {k: {0: per[b]} for k, per in (weights_at or {}).items() if b in per}
        rings.append(fan_out([solo], cfg, [w], [fmt], pushes, capacity, offset, changes, seed=seed)[0][0])
    return rings


# ------------------------------------------------------------------------------------------------ 1. independent converters, the statement
@pytest.mark.parametrize("name", list(cases.SWEEP))
def test_every_beam_equals_an_independent_converter_and_the_statement(engine, targets, solo, name):
    layout, lanes, shape, T, R = cases.SWEEP[name]
    for fcw in (acases.FCWS["odd"], 0):
        cfg, raw, K, _ = cases.config(name, fcw)
        sets, units = cases.weight_sets(K, T, R)
        fmts = cases.ring_formats(R, turn=len(name))
        assert R < 4 or set(fmts) == set(cases.RINGS)
        n_out = lcases.out_total(shape, layout.frames_in(raw.nbytes))
        cap = lcases.ring_capacity(n_out)
        got, n = fan_out([engine] + targets, cfg, sets, fmts, [raw], cap)
        assert n == n_out
        want = independent(solo, cfg, sets, fmts, [raw], cap)
        for b in range(R):
            same_bytes(got[b], want[b], (name, fcw, "beam", b, dcases.RING_NAMES[fmts[b]]))
            assert np.any(got[b][:2 * n_out] != cases.fill(fmts[b], cap)[:2 * n_out]), (name, b)
        if fcw == 0:
            for b, v in enumerate(cases.beams_statement(cfg, sets, [raw], fmts)):
                same_bytes(got[b], cases.placed(fmts[b], cap, v, 0), (name, "statement", b))
        # a unit vector gives the ring of sdr_ddc_create_layout at that lane, as the header promises for beam 0
        for b, a in list(units.items())[:2]:
            solo.iq_alloc(cap, fmts[b])
            solo.iq_upload(cases.fill(fmts[b], cap), 0)
            plain = acases.config(shape, fcw, cfg.gain, ar.element_layout(layout, lanes[a]))
            lcases.push_all(solo, plain, raw, n_out)
            same_bytes(got[b], solo.iq_download(cap, 0), (name, fcw, "layout converter at lane", lanes[a]))


# ------------------------------------------------------------------------------------------------ 2. the cut
CUT_CASES = ["K3_int16_T33D2_R4", "K8_int8_rational_R2", "stap3_K8_int8_T33D2_R4"]


@pytest.mark.parametrize("ring_fmt", [FMT_CF64, FMT_CI8], ids=["ring_cf64", "ring_ci8"])
@pytest.mark.parametrize("name", CUT_CASES)
def test_the_rings_do_not_depend_on_the_cut(engine, targets, name, ring_fmt):
    """One push; pushes of 1 frame; pushes of Tp - 1, Tp and Tp + 1 frames; random cuts with an empty push -- of 1200 frames."""
    layout, lanes, shape, T, R = cases.SWEEP[name]
    cfg, raw, K, _ = cases.config(name, acases.FCWS["odd"])
    n, Tp = 1200, lcases.phase_taps(shape)
    assert layout.frame_group == 1
    raw = acases.piece(raw, layout, 0, n)
    sets, _ = cases.weight_sets(K, T, R)
    rng = np.random.default_rng(cases.SEED + 2)
    marks = np.sort(rng.choice(np.arange(1, n), 12, replace=False))
    marks = np.concatenate([[0], marks, [marks[5]], [n]])
    marks.sort()                                                    # (a repeated mark: an empty push)
    around = []
    while sum(around) < n:
        around += [Tp - 1, Tp, Tp + 1]
    cuts = {"one": [n], "single frames": [1] * n, "around Tp": around, "random": list(np.diff(marks))}
    assert 0 in cuts["random"]
    cap = lcases.ring_capacity(lcases.out_total(shape, n))
    first = None
    for what, lengths in cuts.items():
        cut, at = [], 0
        for v in lengths:
            v = min(int(v), n - at)
            cut.append((at, v))
            at += v
        assert at == n
        got, count = fan_out([engine] + targets, cfg, sets, [ring_fmt] * R, cases.pieces(raw, layout, cut), cap, queue=(what == "single frames"))
        assert count == lcases.out_total(shape, n)
        if first is None:
            first = got
            assert all(np.any(r[:2 * count] != cases.fill(ring_fmt, cap)[:2 * count]) for r in got)
        for b in range(R):
            same_bytes(got[b], first[b], (name, what, b))


# ------------------------------------------------------------------------------------------------ 3. weights changed between pushes
@pytest.mark.parametrize("name", ["K3_int16_T33D2_R4", "stap3_K8_int8_T33D2_R4"])
def test_weight_changes_at_fixed_inputs_under_two_cuts(engine, targets, solo, name):
    """Beam 2 alone changed at input 1000, every beam changed at input 1008 (inputs combined with the old and the new weights
    both still in the filter's history); fcw = 0, so the statement is held byte for byte as well."""
    layout, lanes, shape, T, R = cases.SWEEP[name]
    cfg, raw, K, _ = cases.config(name, 0)
    n = layout.frames_in(raw.nbytes)
    sets, _ = cases.weight_sets(K, T, R)
    marks = (1000, 1008)
    later = {b: cases.general(K, T, 50 + b) for b in range(R)}
    fmts = cases.ring_formats(R)
    n_out = lcases.out_total(shape, n)
    cap = lcases.ring_capacity(n_out)
    results = []
    for lengths in ([], [1, 2, 500, 3, 31, 32, 33, 600, 0, 7]):
        cut = acases.cut_with_marks(lengths, marks, n)
        at = {first: k for k, (first, count) in enumerate(cut) if count > 0 and first in marks}
        changes = {at[marks[0]]: {2: cases.general(K, T, 40)}, at[marks[1]]: later}
        got, count = fan_out([engine] + targets, cfg, sets, fmts, cases.pieces(raw, layout, cut), cap, weights_at=changes)
        assert count == n_out
        results.append(got)
    three = cases.pieces(raw, layout, [(0, marks[0]), (marks[0], marks[1] - marks[0]), (marks[1], n - marks[1])])
    changes = {1: {2: cases.general(K, T, 40)}, 2: later}
    want = cases.beams_statement(cfg, sets, three, fmts, changes)
    plain = cases.beams_statement(cfg, sets, three, fmts)
    alone = independent(solo, cfg, sets, fmts, three, cap, weights_at=changes)
    unchanged, _ = fan_out([engine] + targets, cfg, sets, fmts, three, cap, weights_at={2: later})
    for b in range(R):
        same_bytes(results[1][b], results[0][b], (name, "two cuts", b))
        same_bytes(results[0][b], cases.placed(fmts[b], cap, want[b], 0), (name, "statement", b))
        same_bytes(results[0][b], alone[b], (name, "independent", b))
        assert not np.array_equal(want[b], plain[b])                              # (the changes are in the ring)
        if b != 2:                                                                # beams that the first change left alone
            same_bytes(results[0][b], unchanged[b], (name, "left alone", b))
    assert not np.array_equal(results[0][2], unchanged[2])


# ------------------------------------------------------------------------------------------------ 4. the ring's end, 5. reset
@pytest.mark.parametrize("name", ["K4_2bit_T33D2_R16", "stap3_K3_int16_T1D1_R2"])
def test_a_push_across_the_rings_end_changes_nothing_else(engine, targets, solo, name):
    layout, lanes, shape, T, R = cases.SWEEP[name]
    cfg, raw, K, _ = cases.config(name, acases.FCWS["odd"])
    sets, _ = cases.weight_sets(K, T, R)
    fmts = cases.ring_formats(R, 1)
    n_out = lcases.out_total(shape, layout.frames_in(raw.nbytes))
    cap = lcases.ring_capacity(n_out + 400)
    offset = cap - n_out // 3
    got, n = fan_out([engine] + targets, cfg, sets, fmts, [raw], cap, offset, seed=4)
    want = independent(solo, cfg, sets, fmts, [raw], cap, offset, seed=4)
    assert n == n_out and offset + n > cap
    for b in range(R):
        same_bytes(got[b], want[b], (name, b))
        untouched = np.arange(2 * (offset + n - cap), 2 * offset)               # (between the wrapped end and the start)
        assert np.array_equal(got[b][untouched], cases.fill(fmts[b], cap, 4)[untouched]) and untouched.size == 2 * (cap - n)


def test_reset_zeroes_every_history_and_keeps_every_weight(engine, targets):
    name = "stap3_K8_int8_T33D2_R4"
    layout, lanes, shape, T, R = cases.SWEEP[name]
    cfg, raw, K, _ = cases.config(name, acases.FCWS["odd"])
    sets, _ = cases.weight_sets(K, T, R)
    fmts = cases.ring_formats(R)
    n_out = lcases.out_total(shape, layout.frames_in(raw.nbytes))
    cap = lcases.ring_capacity(n_out)
    engines = [engine] + targets[:R - 1]
    prepare(engines, fmts, cap)
    cfg0 = cases.with_weights(cfg, cases.general(K, T, 90))
    ddc = engine.ddc_create(cfg0)
    try:
        for b in range(1, R):
            engine.ddc_beam_attach(ddc, engines[b], cases.general(K, T, 90 + b))
        for b in range(R):                                                        # (the weights of the runs: set after the attachment)
            set_weights(engine, ddc, cfg0, b, sets[b])
        runs = []
        for k in range(2):
            assert engine.ddc_push(ddc, raw, 0) == n_out
            runs.append([e.iq_download(cap, 0) for e in engines])
            for e, fmt in zip(engines, fmts):
                e.iq_upload(cases.fill(fmt, cap), 0)
            if k == 0:                                                            # without the reset the histories go on
                assert engine.ddc_push(ddc, raw, 0) == n_out
                assert all(not np.array_equal(e.iq_download(cap, 0), r) for e, r in zip(engines, runs[0]))
                engine.ddc_reset(ddc)
                assert engine.ddc_beam_count(ddc) == R
    finally:
        engine.ddc_destroy(ddc)
    fresh, _ = fan_out(engines, cfg, sets, fmts, [raw], cap)
    for b in range(R):
        same_bytes(runs[1][b], runs[0][b], ("after the reset", b))
        same_bytes(runs[0][b], fresh[b], ("a fresh converter", b))


# ------------------------------------------------------------------------------------------------ 6. ordering without a host wait
def test_a_queued_push_is_ordered_with_the_targets_own_streams(engine, targets, solo):
    """sdr_ddc_push_queue, then at once (no wait on the leader) a download and a search on a target: both see the push.  An upload
    queued on the target's own stream just before the push, at the same ring samples: the push wins."""
    from oracle import sydr_oracle as orc
    raw, fs = acases.jammed_recording(), acases.E2E_FS
    per_ms = int(fs * 1e-3)
    n = 3 * per_ms
    raw = acases.piece(raw, acases.E2E_LAYOUT, 0, n)
    R, count = ar.covariance(acases.piece(raw, acases.E2E_LAYOUT, 0, 2 * per_ms), acases.E2E_LAYOUT, acases.E2E_LANES)
    sets = [ar.unit_weights(4, 0), ar.power_inversion(R, count), ar.unit_weights(4, 2)]
    cfg = dc.DownConverterConfig(dc.IN_R8, 1, np.ones(1), 0, 1.0 / 8.0, 1, acases.E2E_LAYOUT, ar.ArrayGeometry(acases.E2E_LANES))
    cap = lcases.ring_capacity(n)
    fmts = [FMT_CI16] * 3
    engines = [engine] + targets[:2]
    want = independent(solo, cfg, sets, fmts, [raw], cap)
    # what a search finds on beam 1's ring, by the same engine call behind a synchronous upload
    solo.iq_alloc(cap, FMT_CI16)
    solo.iq_upload(want[1], 0)
    solo.code_slots(1)
    solo.load_gps_code(0, acases.E2E_PRN)
    want_search = solo.pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)[:3]
    prepare(engines, fmts, cap)
    engines[1].code_slots(1)
    engines[1].load_gps_code(0, acases.E2E_PRN)
    junk = np.full(2 * cap, 77, dtype=np.int16)
    ddc = engine.ddc_create(cases.with_weights(cfg, sets[0]))
    try:
        for b in (1, 2):
            engine.ddc_beam_attach(ddc, engines[b], sets[b])
        engines[2].sync()
        engines[2].iq_upload_queue(junk, 0)                                        # queued on the target's stream, not waited for
        assert engine.ddc_push_queue(ddc, raw, 0) == n
        got_search = engines[1].pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)[:3]     # the target's own call, at once
        got_1 = engines[1].iq_download(cap, 0)
        got_2 = engines[2].iq_download(cap, 0)
        engine.sync()
        got_0 = engine.iq_download(cap, 0)
    finally:
        engine.ddc_destroy(ddc)
    same_bytes(got_1, want[1], "download behind a queued push")
    same_bytes(got_0, want[0], "beam 0")
    want_2 = want[2].copy()
    want_2[2 * n:] = 77                                                           # (the upload covered the whole ring, the push its first n)
    same_bytes(got_2, want_2, "the push behind the target's own upload")
    assert [int(got_search[0][0]), int(got_search[1][0])] == [int(want_search[0][0]), int(want_search[1][0])] == [13, 2826]
    assert float(got_search[2][0]) == float(want_search[2][0]) > 4.0


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_change_nothing(engine, targets, solo):
    """Every SDR_ERR_* case of the header, each in the middle of a stream whose rest is then compared with an undisturbed run."""
    name = "K3_int16_T33D2_R4"
    layout, lanes, shape, T, R = cases.SWEEP[name]
    cfg, raw, K, _ = cases.config(name, acases.FCWS["odd"])
    n = layout.frames_in(raw.nbytes)
    sets, _ = cases.weight_sets(K, T, R)
    fmts = cases.ring_formats(R)
    n_out = lcases.out_total(shape, n)
    cap = lcases.ring_capacity(n_out)
    want, _ = fan_out([engine] + targets, cfg, sets, fmts, cases.pieces(raw, layout, [(0, 1001), (1001, n - 1001)]), cap)
    lib = _lib.load()
    wp = lambda v: np.ascontiguousarray(v, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    good = wp([1.0, 0.0] * K)
    beam = C.c_int(-7)
    engines = [engine] + targets[:R - 1]
    spare, small, bare = targets[R], targets[R + 1], Engine(0)                     # (bare: never given a ring)
    prepare(engines, fmts, cap)
    spare.iq_alloc(cap, FMT_CI16)
    small.iq_alloc(cap - 8, FMT_CI16)
    cfg0 = cases.with_weights(cfg, sets[0])
    ddc = engine.ddc_create(cfg0)
    plain = engine.ddc_create(acases.config(shape, 0, 1.0, ar.element_layout(layout, 0)))
    mitigated = engine.ddc_create(cfg0)
    mit = mt.MitigationConfig(100.0, 2, 5, 0, None)
    try:
        attach = lambda d, t, w=good: lib.sdr_ddc_beam_attach(engine._h, d.handle, t._h if t is not None else None, w, C.byref(beam))
        # before anything is attached
        assert engine.ddc_beam_count(ddc) == 1 and lib.sdr_ddc_beam_count(None) == INVALID
        assert attach(plain, spare) == INVALID                                    # neither an array nor a space-time converter
        assert attach(ddc, engine) == INVALID and attach(ddc, None) == INVALID and attach(ddc, spare, None) == INVALID
        assert attach(ddc, small) == INVALID and attach(ddc, bare) == INVALID     # another capacity, no ring
        assert lib.sdr_ddc_beam_attach(solo._h, ddc.handle, spare._h, good, None) == INVALID      # (the converter is another engine's)
        for bad in ([1.0, 0.0, float("nan"), 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0, 0.0, float("-inf")]):
            assert attach(ddc, spare, wp(bad)) == INVALID
        assert lib.sdr_ddc_beam_weights(engine._h, ddc.handle, 1, good) == INVALID and lib.sdr_ddc_beam_weights(engine._h, ddc.handle, 0, good) == INVALID
        engine.ddc_mitigate(mitigated, mit)
        assert attach(mitigated, spare) == UNSUPPORTED and engine.ddc_beam_count(mitigated) == 1
        assert beam.value == -7 and engine.ddc_beam_count(ddc) == 1
        for b in range(1, R):
            assert engine.ddc_beam_attach(ddc, engines[b], sets[b]) == b
        assert attach(ddc, engines[2]) == INVALID                                 # attached twice
        with pytest.raises(SdrError) as err:
            engine.ddc_mitigate(ddc, mit)
        assert err.value.status == UNSUPPORTED
        engine.ddc_mitigate(ddc, None)                                            # (detaching what is not there stays allowed)
        at = lcases.out_total(shape, 1001)
        assert engine.ddc_push(ddc, acases.piece(raw, layout, 0, 1001), 0) == at
        # in the middle of the stream
        assert attach(ddc, spare) == STATE and lib.sdr_ddc_beams_clear(engine._h, ddc.handle) == STATE
        for b in (0, R, -1, 16):
            assert lib.sdr_ddc_beam_weights(engine._h, ddc.handle, b, good) == INVALID
        assert lib.sdr_ddc_beam_weights(engine._h, ddc.handle, 1, None) == INVALID
        assert lib.sdr_ddc_beam_weights(engine._h, ddc.handle, 1, wp([float("inf")] * 2 * K)) == INVALID
        n_out_c = C.c_int64(-7)
        for call in (lib.sdr_ddc_push, lib.sdr_ddc_push_queue):
            assert call(engine._h, ddc.handle, raw.ctypes.data, 100, cap, C.byref(n_out_c)) == RANGE
            assert call(engine._h, ddc.handle, raw.ctypes.data, 100, -1, C.byref(n_out_c)) == RANGE and n_out_c.value == -7
        assert engine.ddc_beam_count(ddc) == R
        assert engine.ddc_push(ddc, acases.piece(raw, layout, 1001, n - 1001), at) == n_out - at
        for b, e in enumerate(engines):
            same_bytes(e.iq_download(cap, 0), want[b], ("after the refusals", b))
        # the sixteenth beam is the last; clearing needs a reset
        engine.ddc_reset(ddc)
        for k in range(R - 1, MAX_BEAMS - 1):
            targets[k].iq_alloc(cap, FMT_CI8)
            assert engine.ddc_beam_attach(ddc, targets[k], sets[1]) == k + 1
        assert engine.ddc_beam_count(ddc) == MAX_BEAMS
        targets[15].iq_alloc(cap, FMT_CI8)
        assert attach(ddc, targets[15]) == INVALID and engine.ddc_beam_count(ddc) == MAX_BEAMS
        engine.ddc_beams_clear(ddc)
        assert engine.ddc_beam_count(ddc) == 1
        engine.iq_upload(cases.fill(fmts[0], cap), 0)
        assert engine.ddc_push(ddc, raw, 0) == n_out                              # beam 0 goes on alone
        alone, _ = fan_out([solo], cfg, sets[:1], fmts[:1], [raw], cap)
        same_bytes(engine.iq_download(cap, 0), alone[0], "beam 0 after the clearing")
    finally:
        for d in (ddc, plain, mitigated):
            engine.ddc_destroy(d)
        bare.close()


# ------------------------------------------------------------------------------------------------ 8. no beams, no difference
def test_without_beams_the_launches_are_the_old_ones_and_with_beams_one_more(engine, targets):
    layout, lanes = acases.GEOMETRIES["K3_int8_complex"]
    raw = acases.stream(layout)
    SCOPES = ("ddc_kernel", "resample_kernel", "ddc_beam_kernel", "resample_beam_kernel", "ddc_history_kernel", "ddc_array_cov_kernel", "call_ddc_push")
    engine.prof_enable(True)
    try:
        for shape, kernel in (((33, 2), "ddc"), ((3, 2, 7), "resample")):
            cfg = acases.config(shape, 0, 1.0 / 4.0, layout, ar.ArrayGeometry(lanes, acases.general_weights(3)))
            n_out = lcases.out_total(shape, acases.N_FRAMES)
            cap = lcases.ring_capacity(n_out)
            for R in (1, 3):
                engines = [engine] + targets[:R - 1]
                prepare(engines, [FMT_CF64] * R, cap)
                ddc = engine.ddc_create(cfg)
                try:
                    for b in range(1, R):
                        engine.ddc_beam_attach(ddc, engines[b], acases.general_weights(3, b))
                    engine.sync()
                    engine.prof_reset()
                    engine.ddc_push(ddc, raw, 0)
                    engine.sync()
                    counts = {name: engine.prof_read(name)[1] for name in SCOPES}
                    total = engine.prof_read("")[1]
                    ring = engine.iq_download(cap, 0)
                    engine.prof_enable(True, calls_only=True)                     # ... and one bracket around all of them
                    engine.ddc_reset(ddc)
                    engine.prof_reset()
                    engine.ddc_push(ddc, raw, 0)
                    engine.sync()
                    assert engine.prof_read("call_ddc_push")[1] == engine.prof_read("")[1] == 1
                    engine.prof_enable(True)
                finally:
                    engine.ddc_destroy(ddc)
                want = dict.fromkeys(SCOPES, 0)
                want.update({kernel + "_kernel": 1, "ddc_history_kernel": 1})         # (call_* scopes record in their own mode)
                if R > 1:
                    want[kernel + "_beam_kernel"] = 1
                assert counts == want and total == sum(want.values()), (shape, R, counts, total)
                same_bytes(ring, cases.placed(FMT_CF64, cap, ar.statement(cfg, [raw], FMT_CF64), 0), (shape, R))
    finally:
        engine.prof_enable(False)


# ------------------------------------------------------------------------------------------------ 9. through the engines
def test_a_jammed_recording_through_five_engines(engine, targets):
    """array_cases.jammed_recording (4 elements, 4 MHz, 8 ms): beam 0 with power-inversion weights, beams 1..4 the elements.  The
    search on beam 0 finds what the oracle finds on the statement's ring, the search on an element beam misses as docs/notes/array.md
    records, and the prompts of the four element engines are the oracle's EPL on the statement's element rings within
    test_gpu_epl.py's tolerance (1e-9 of the accumulator's norm)."""
    from oracle import sydr_oracle as orc
    raw, fs, prn = acases.jammed_recording(), acases.E2E_FS, acases.E2E_PRN
    per_ms = int(fs * 1e-3)
    n = acases.E2E_MS * per_ms
    R, count = ar.covariance(acases.piece(raw, acases.E2E_LAYOUT, 0, acases.E2E_TRAIN_MS * per_ms), acases.E2E_LAYOUT, acases.E2E_LANES)
    sets = [ar.power_inversion(R, count)] + list(ar.element_weights(4))
    cfg = dc.DownConverterConfig(dc.IN_R8, 1, np.ones(1), 0, 1.0 / 8.0, 1, acases.E2E_LAYOUT, ar.ArrayGeometry(acases.E2E_LANES))
    rings = ar.beams_statement(cfg, sets, [raw], [FMT_CI16] * 5)
    n_code = orc.samples_per_code(fs)
    code = orc.gold_code(prn)
    spectrum = orc.code_spectrum(code, fs)

    def search(ring):
        x = orc.iq_to_complex(ring.astype(np.float64))
        cmap = orc.pcps_map(x[:n_code].reshape(1, -1), 0.0, fs, spectrum, 5000.0, 250.0, n_code)
        return orc.two_peak_compare(cmap, n_code, round(fs / orc.CODE_RATE))

    engines = [engine] + targets[:4]
    cap = lcases.ring_capacity(n)
    prepare(engines, [FMT_CI16] * 5, cap)
    for e in engines:
        e.code_slots(1)
        e.load_gps_code(0, prn)
    ddc = engine.ddc_create(cases.with_weights(cfg, sets[0]))
    try:
        for b in range(1, 5):
            engine.ddc_beam_attach(ddc, engines[b], sets[b])
        assert engine.ddc_push(ddc, raw, 0) == n
        for b, e in enumerate(engines):
            same_bytes(e.iq_download(n, 0), rings[b], ("ring", b))
        peak, ratio = search(rings[0])
        pb, pc, pr, _ = engine.pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)
        assert [int(pb[0]), int(pc[0])] == peak == [13, 2826] and abs(pr[0] - ratio) <= 1e-9 * ratio and ratio > 4.0
        peak1, ratio1 = search(rings[1])
        pb, pc, pr, _ = engines[1].pcps([0], 0, fs, 0.0, 5000.0, 250.0, 1, 1)
        assert [int(pb[0]), int(pc[0])] == peak1 != peak and abs(pr[0] - ratio1) <= 1e-9 * ratio1 and ratio1 < 1.5
        step = orc.CODE_RATE / fs
        m = orc.required_samples(0.0, step)
        starts = peak[1] + 1 + np.arange(acases.E2E_MS - 2) * n_code
        items = make_items(0, m, starts, acases.E2E_SAT["doppler"], 0.0, 0.0, step)
        for b in range(1, 5):
            got = engines[b].epl_batch(items, (-0.5, 0.0, 0.5), fs)
            x = orc.iq_to_complex(rings[b].astype(np.float64))
            for k, s in enumerate(starts):
                ref = np.array(orc.epl(x[s:s + m], orc.pad_code(code), fs, acases.E2E_SAT["doppler"], 0.0, 0.0, step, (-0.5, 0.0, 0.5)))
                scale = np.repeat(np.hypot(ref[0::2], ref[1::2]), 2)
                assert np.max(np.abs(got[k] - ref) / scale) <= 1e-9, (b, k)
    finally:
        engine.ddc_destroy(ddc)
