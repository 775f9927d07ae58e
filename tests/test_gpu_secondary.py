"""sdr_acq_secondary on the MI355X against its NumPy statement (tests/secondary_cases.py; the CPU file tests/test_secondary.py
shows that the inputs are fair): parity of segment sums, power table, indices and prompt; the segment sums against
sdr_acq_refine's, bit for bit; ring formats and the ring's end; batching and frequency tiles; the edges of the grouping;
determinism, NaN, refusals, independence of the engine's history; and the reason for the feature end to end (the zero-padded
search's result taken to a secondary phase and a fine frequency)."""
import numpy as np
import pytest

import refine_cases as rc
import secondary_cases as sc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import (FMT_CF32, FMT_CF64, FMT_CI16, FMT_CI8, Engine, make_refine_items, make_secondary_items)
from test_secondary import MARGIN

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6


def check_parity(res, power, z, mdl, M, S, mode, tag="", degenerate=False):
    """One item of a call against the model's (fine, h, k, P, z, prompt): the tolerances of sdr_acq_refine's check_parity."""
    fine_m, h_m, k_m, P_m, z_m, x_m = mdl
    assert sc.margin(P_m[:1] if degenerate else P_m) > MARGIN, tag          # (the indices are then decided beyond rounding)
    zmax = np.abs(z_m).max()
    err_z = np.abs(z - z_m).max() / zmax
    bound_p = 4e-9 * (M * S * zmax) ** 2
    err_p = np.abs(power - P_m).max()
    print(f"{tag}: max|dz|/max|z| = {err_z:.2e} (cap 1e-9), max|dP| = {err_p:.3e} (cap {bound_p:.3e}), idx {res['fine_idx']},{res['sec_phase']}")
    assert err_z <= 1e-9, tag
    assert err_p <= bound_p, tag
    assert (int(res["fine_idx"]), int(res["sec_phase"])) == (k_m, h_m), tag
    assert res["fine_hz"] == fine_m and abs(res["power"] - P_m[h_m, k_m]) <= bound_p, tag
    assert abs(res["power_other"] - sc.power_other(P_m, h_m)) <= bound_p, tag
    if mode == 0:
        bound_x = 2e-9 * M * S * zmax
        assert abs(res["prompt_re"] - x_m.real) <= bound_x and abs(res["prompt_im"] - x_m.imag) <= bound_x, tag
    else:
        assert res["prompt_re"] == 0.0 and res["prompt_im"] == 0.0, tag


def stage(engine, raw, code, fmt=FMT_CI8, capacity=None, offset=0):
    n = raw.size if np.iscomplexobj(raw) else raw.size // 2
    engine.iq_alloc(capacity or (n + 7) // 8 * 8, fmt)
    engine.iq_upload(raw, offset)
    engine.code_slots(2, max(1023, len(code)))
    engine.set_code(1, np.asarray(code).astype(np.int8))


def run(engine, c, span=sc.SPAN, step=sc.STEP, start=None, want_tables=True):
    items = make_secondary_items(1, 0, c["s0"] if start is None else start, c["f0"], c["code_hz"])
    return engine.acq_secondary(items, c["sec"], c["fs"], c["M"], c["S"], span, step, c["mode"], want_tables=want_tables)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_parity(engine, name):
    c = sc.case(name)
    stage(engine, c["raw"], c["code"])
    res, power, z = run(engine, c)
    check_parity(res[0], power[0], z[0], sc.model(name), c["M"], c["S"], c["mode"], name)
    assert res[0]["sec_phase"] == c["true_phase"] and abs(res[0]["fine_hz"] - c["doppler"]) <= sc.STEP / 2
    # two identical calls: identical bytes; and the tables are optional
    res2, power2, z2 = run(engine, c)
    assert res.tobytes() == res2.tobytes() and power.tobytes() == power2.tobytes() and z.tobytes() == z2.tobytes()
    assert run(engine, c, want_tables=False).tobytes() == res.tobytes()


@pytest.mark.parametrize("name", ["E1", "E2", "E3", "E4"])
def test_segment_sums_are_acq_refines_bit_for_bit(engine, name):
    c = sc.case(name)                                           # M = 12 <= 20: both calls take the window
    stage(engine, c["raw"], c["code"])
    starts = [c["s0"], c["s0"] - c["N"]] if c["later"] else [c["s0"], c["s0"] + c["N"]]
    z = engine.acq_secondary(make_secondary_items(1, 0, starts, c["f0"], c["code_hz"]), c["sec"], c["fs"], c["M"], c["S"], sc.SPAN,
                             sc.STEP, 0, want_tables=True)[2]
    z_ref = engine.acq_refine(make_refine_items(1, starts, c["f0"], c["code_hz"]), c["fs"], c["M"], c["S"], sc.SPAN, sc.STEP,
                              want_tables=True)[2]
    assert z.shape == z_ref.shape == (2, 12, 4) and z.tobytes() == z_ref.tobytes()


@pytest.mark.parametrize("fmt_name", ["ci16", "cf32", "cf64"])
def test_parity_other_ring_formats(engine, fmt_name):
    c = sc.case("A1")
    if fmt_name == "ci16":
        stage(engine, c["raw"].astype(np.int16), c["code"], FMT_CI16)
    else:
        stage(engine, c["rf"], c["code"], FMT_CF32 if fmt_name == "cf32" else FMT_CF64)      # (small integers: exact in float32)
    res, power, z = run(engine, c)
    check_parity(res[0], power[0], z[0], sc.model("A1"), c["M"], c["S"], c["mode"], fmt_name)


def test_parity_window_across_the_rings_end(engine):
    """A ring of the window + 8 samples, written so that the window starts three and a half periods before the ring's end;
    the item's start_sample is given a whole turn of the ring too high (indices are taken modulo the capacity)."""
    c = sc.case("A1")
    cap = c["M"] * c["N"] + 8
    piece = c["raw"][2 * c["s0"]:2 * (c["s0"] + cap)]
    assert piece.size == 2 * cap and cap % 8 == 0
    offset = cap - 3 * c["N"] - c["N"] // 2
    stage(engine, piece, c["code"], capacity=cap, offset=offset)
    ring = np.roll(orc.iq_to_complex(piece), offset)
    res, power, z = run(engine, c, start=offset + cap)
    mdl = sc.secondary_model(ring, offset, c["code"], c["sec"], c["fs"], c["f0"], c["M"], c["S"], mode=c["mode"])
    check_parity(res[0], power[0], z[0], mdl, c["M"], c["S"], c["mode"], "wrap")
    assert mdl[1] == c["true_phase"] and np.array_equal(mdl[4], sc.model("A1")[4])      # (the same samples, the same sums)


def test_32_items_in_one_call_and_one_by_one(engine):
    raw, rf, secs, items, M, S = sc.batch32()
    code = orc.gold_code(sc.PRN)
    stage(engine, raw, code)
    rec = make_secondary_items(1, [r for r, *_ in items], [s for _, s, *_ in items], [f for _, _, f, *_ in items], orc.CODE_RATE)
    assert len(rec) == 32
    res, power, z = engine.acq_secondary(rec, secs, 4e6, M, S, want_tables=True)
    for i, (row, s0, f0, phase, dop) in enumerate(items):
        mdl = sc.secondary_model(rf, s0, code, secs[row], 4e6, f0, M, S)
        check_parity(res[i], power[i], z[i], mdl, M, S, 0, f"item {i}")
        assert res[i]["sec_phase"] == phase
        one = make_secondary_items(1, 0, s0, f0, orc.CODE_RATE)
        r1, p1, z1 = engine.acq_secondary(one, secs[row], 4e6, M, S, want_tables=True)
        assert r1.tobytes() == res[i:i + 1].tobytes() and p1.tobytes() == power[i].tobytes() and z1.tobytes() == z[i].tobytes(), i


@pytest.mark.parametrize("name", sc.EXTRA_NAMES)
def test_parity_edges_of_tiles_and_groups(engine, name):
    c, span, step = sc.extra(name)
    stage(engine, c["raw"], c["code"])
    res, power, z = run(engine, c, span, step)
    assert power.shape == (1, len(c["sec"]), engine.acq_refine_bins(span, step))
    check_parity(res[0], power[0], z[0], sc.extra_model(name), c["M"], c["S"], c["mode"], name, degenerate=name == "M2")
    if name == "M2":
        assert power[0, 0].tobytes() == power[0, 1].tobytes()


def test_a_row_of_ones_is_acq_refines_no_edge_row(engine):
    c = sc.case("E1")
    stage(engine, c["raw"], c["code"])
    ones = np.ones(5, np.int8)
    res, power, _ = engine.acq_secondary(make_secondary_items(1, 0, c["s0"], c["f0"], c["code_hz"]), ones, c["fs"], 12, 4, want_tables=True)
    ref, power_ref, _ = engine.acq_refine(make_refine_items(1, c["s0"], c["f0"], c["code_hz"]), c["fs"], 12, 4, sc.SPAN, sc.STEP, want_tables=True)
    assert np.allclose(power[0, 0], power_ref[0, 0], rtol=1e-12, atol=0.0) and res[0]["sec_phase"] == 0
    assert all(power[0, h].tobytes() == power[0, 0].tobytes() for h in range(5))
    assert res[0]["power"] == res[0]["power_other"] == power[0, 0].max() and res[0]["fine_idx"] == int(power[0, 0].argmax())


def test_not_a_number_in_one_items_window(engine):
    c = sc.make_case(1, 1630.0, 0, orc.gold_code(sc.PRN), sc.NH20, 4e6, orc.CODE_RATE, sc.CODE_PHASE, 12, 4, 0, 8.0, extra_periods=26)
    starts = [c["s0"], c["s0"] + 12 * c["N"], c["s0"] + 24 * c["N"]]            # three windows side by side
    items = make_secondary_items(1, 0, starts, c["f0"], c["code_hz"])
    stage(engine, c["rf"], c["code"], FMT_CF64)
    clean = engine.acq_secondary(items, c["sec"], c["fs"], 12, 4, want_tables=True)
    rf = c["rf"].copy()
    rf[starts[1] + 5 * c["N"] + 17] = np.nan
    stage(engine, rf, c["code"], FMT_CF64)
    res, power, z = engine.acq_secondary(items, c["sec"], c["fs"], 12, 4, want_tables=True)
    assert np.isnan(res[1]["power"]) and np.isnan(res[1]["power_other"]) and np.isnan(power[1]).all()
    assert res[1]["fine_hz"] == c["f0"] and res[1]["fine_idx"] == 25 and res[1]["sec_phase"] == 0
    assert res[1]["prompt_re"] == 0.0 and res[1]["prompt_im"] == 0.0
    for i in (0, 2):
        assert not np.isnan(res[i]["power"])
        assert res[i:i + 1].tobytes() == clean[0][i:i + 1].tobytes() and power[i].tobytes() == clean[1][i].tobytes()
        assert z[i].tobytes() == clean[2][i].tobytes()


def test_refused_calls_leave_the_engine_as_it_was(engine):
    c = sc.case("A1")
    stage(engine, c["raw"], c["code"])
    item = make_secondary_items(1, 0, c["s0"], c["f0"], c["code_hz"])
    good = engine.acq_secondary(item, c["sec"], c["fs"], 40, 4, want_tables=True)
    base = dict(items=item, sec_codes=c["sec"], fs=c["fs"], n_periods=40, n_segments=4, span_hz=sc.SPAN, step_hz=sc.STEP, mode=0)
    zero_chip = c["sec"].copy()
    zero_chip[7] = 0
    two_rows = make_secondary_items(1, [0, 2], c["s0"], c["f0"], c["code_hz"])
    for kwargs, status in ((dict(n_periods=1), INVALID), (dict(n_periods=129), INVALID), (dict(n_segments=0), INVALID),
                           (dict(n_segments=65), INVALID), (dict(sec_codes=np.ones(1, np.int8)), INVALID),
                           (dict(sec_codes=np.ones(129, np.int8)), INVALID), (dict(sec_codes=zero_chip), INVALID),
                           (dict(sec_codes=np.stack([c["sec"]] * 2)), INVALID),          # more rows than items
                           (dict(items=two_rows, sec_codes=np.stack([c["sec"]] * 2)), INVALID),      # sec_row 2 of two rows
                           (dict(mode=2), INVALID), (dict(step_hz=0.0), INVALID), (dict(span_hz=float("nan")), INVALID),
                           (dict(items=make_secondary_items(0, 0, c["s0"], c["f0"], c["code_hz"])), INVALID),      # nothing staged there
                           (dict(items=make_secondary_items(1, 0, c["s0"], float("inf"), c["code_hz"])), INVALID),
                           (dict(items=make_secondary_items(1, 0, c["s0"], c["f0"], 0.0)), INVALID),
                           (dict(n_segments=64), UNSUPPORTED),                           # 40 x 64 segments
                           (dict(span_hz=50000.0), UNSUPPORTED),                         # K = 20001
                           (dict(fs=40e3, n_periods=2, n_segments=64), UNSUPPORTED),     # 64 segments in a period of 40 samples
                           (dict(n_periods=43), RANGE),                                  # the recording holds 42 periods
                           (dict(items=make_secondary_items(1, 0, -1, c["f0"], c["code_hz"])), RANGE)):
        args = dict(base)
        args.update(kwargs)
        with pytest.raises(_lib.SdrError) as err:
            engine.acq_secondary(**args)
        assert err.value.status == status and str(err.value), (kwargs, err.value.status)
        again = engine.acq_secondary(item, c["sec"], c["fs"], 40, 4, want_tables=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, good)), kwargs
    lib = _lib.load()
    res = np.zeros(1, dtype=_lib.SEC_RESULT_DTYPE)
    sec = np.ascontiguousarray(c["sec"])
    call = lambda it, s, r: lib.sdr_acq_secondary(engine._h, it, 1, s, 1, 20, c["fs"], 40, 4, sc.SPAN, sc.STEP, 0, r, None, None)
    assert call(_lib.ptr(item), _lib.ptr(sec), None) == INVALID and b"results" in lib.sdr_last_error()
    assert call(None, _lib.ptr(sec), _lib.ptr(res)) == INVALID
    assert call(_lib.ptr(item), None, _lib.ptr(res)) == INVALID and b"sec_codes" in lib.sdr_last_error()
    assert call(_lib.ptr(item), _lib.ptr(sec), _lib.ptr(res)) == 0 and res.tobytes() == good[0].tobytes()
    fresh = Engine(0)
    try:
        with pytest.raises(_lib.SdrError) as err:
            fresh.acq_secondary(item, c["sec"], c["fs"], 40, 4)
        assert err.value.status == STATE
        fresh.iq_alloc(1024, FMT_CI8)
        with pytest.raises(_lib.SdrError) as err:
            fresh.acq_secondary(item, c["sec"], c["fs"], 40, 4)
        assert err.value.status == STATE and "slots" in str(err.value)
    finally:
        fresh.close()


def test_bits_do_not_depend_on_the_engines_history():
    """acq_refine, acq_secondary, pcps_signal, acq_secondary on one engine: each call's bits are those of a fresh engine."""
    a = rc.acquired(4e6, *rc.SATELLITES[0])
    sec_item = make_secondary_items(1, 0, a["s0"], a["f0"], orc.CODE_RATE)

    def staged():
        e = Engine(0)
        stage(e, a["raw"], a["code"])
        return e

    calls = [lambda e: e.acq_refine(make_refine_items(1, a["s0"], a["f0"]), 4e6, 10, 8, 250.0, 5.0, want_tables=True),
             lambda e: e.acq_secondary(sec_item, sc.NH20, 4e6, 30, 4, want_tables=True),
             lambda e: e.pcps_signal([1], 0, 4e6, 0.0, 5000.0, 250.0, orc.CODE_RATE, pad=1, noncoh=2, want_map=True, n_chips=1023),
             lambda e: e.acq_secondary(sec_item, sc.NH10, 4e6, 24, 8, 250.0, 5.0, mode=1, want_tables=True)]
    used = staged()
    try:
        for i, call in enumerate(calls):
            got = call(used)
            fresh = staged()
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want) and all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), i
    finally:
        used.close()


def test_end_to_end_padded_search_then_secondary_sync(engine):
    c = sc.case("C")
    stage(engine, c["raw"], c["code"])
    pb, pc, pr, _ = engine.pcps_signal([1], 0, c["fs"], 0.0, 2000.0, 250.0, c["code_hz"], pad=1, noncoh=2)
    coarse = -np.arange(-2000.0, 2001.0, 250.0)[int(pb[0])]          # the searches mix with if_hz - bin
    print(f"padded search: Doppler {coarse}, code sample {int(pc[0])} (truth {c['s0'] % c['N']}), ratio {pr[0]:.2f}")
    assert coarse == 1750.0 and int(pc[0]) == c["s0"] % c["N"]
    start = int(pc[0]) + c["N"]                                      # a code period's start with 50 periods behind it
    res = engine.acq_secondary(make_secondary_items(1, 0, start, coarse, c["code_hz"]), sc.SEC25, c["fs"], 50, 4)[0]
    print(f"secondary: phase {res['sec_phase']}, fine {res['fine_hz']}, power ratio {res['power'] / res['power_other']:.2f}")
    assert res["sec_phase"] == 5 and res["fine_hz"] == 1630.0 and res["power"] / res["power_other"] > 2.0


def test_function_level_secondary_sync():
    from sydr_amd.dsp.signalsearch import SecondarySync
    c = sc.case("A3")
    fine, phase, ratio, P = SecondarySync(c["rf"][c["s0"]:c["s0"] + c["M"] * c["N"]], c["fs"], c["code"], c["code_hz"], c["sec"], c["f0"], c["M"])
    assert fine == 4120.0 and phase == c["true_phase"] and ratio > 2.0 and P.shape == (20, 51)
