"""sdr_pcps_coherent on the MI355X against its NumPy statement (tests/coherent_cases.py; the CPU file tests/test_coherent.py
shows that the inputs are fair): parity of the reduced map R, of the peak cell's power table, of every index and of the
carrier; the transform routes, the two-peak window's edges, ring formats and the ring's end; one call against separate calls
and against another cut of the scratch, bit for bit; determinism and independence of the engine's history; the reason for the
feature end to end (found with a ratio >= 1.5 where the padded search stays below); the hand-over to sdr_acq_secondary; refusals.

The fine grid has K = 2*floor(span/step) + 1 frequencies, an odd number: K = 63 is the largest grid the call takes, K = 65
(SDR_ERR_UNSUPPORTED) the next; k63first / k63last stand where the issue spoke of K = 64."""
import ctypes as C

import numpy as np
import pytest

import coherent_cases as cc
import secondary_cases as sc
from oracle import sydr_oracle as orc
from sydr_amd import _lib
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI16, FMT_CI8, Engine, make_secondary_items
from test_coherent import MARGIN

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, RANGE, STATE = -1, -4, -5, -6
CAP = 1e-9                     # of the statement's own maximum: the cap sdr_acq_deep's maps are held to


def stage(engine, raw, codes, fmt=FMT_CI8, capacity=None, offset=0):
    """The recording into the ring, code p of `codes` into slot p + 1 (slot 0 stays empty)."""
    n = raw.size if np.iscomplexobj(raw) else raw.size // 2
    engine.iq_alloc(capacity or (n + 7) // 8 * 8, fmt)
    engine.iq_upload(raw, offset)
    codes = np.atleast_2d(codes)
    engine.code_slots(len(codes) + 1, max(1023, codes.shape[1]))
    for p, code in enumerate(codes):
        engine.set_code(p + 1, np.asarray(code).astype(np.int8))


def run(engine, c, want=True, **over):
    a = dict(c)
    a.update(over)
    slots = a.get("slots", list(range(1, len(a["codes"]) + 1)))
    return engine.pcps_coherent(slots, a["rows"], a["secs"], a["start"], a["fs"], a["if_hz"], a["range"], a["step"], a["code_hz"],
                                a["M"], a["span"], a["fine"], a["mode"], a["excl"], want_map=want, want_power=want,
                                n_chips=a["codes"].shape[1])


def same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check_parity(got, mdl, c, tag, ties=False):
    """One call of one PRN against the statement's (results, R, P)."""
    res, R, P = got
    res_m, R_m, P_m = mdl
    r, m = res[0], res_m[0]
    assert cc.map_margin(R_m[0], int(m["peak_bin"]), int(m["peak_code"]), cc.excl_of(c)) >= MARGIN, tag
    assert cc.table_margin(P_m[0], ties) >= MARGIN, tag       # (the indices are then decided beyond rounding)
    err_r = np.abs(R - R_m).max() / R_m.max()
    err_p = np.abs(P - P_m).max() / P_m.max()
    print(f"{tag}: max|dR|/max R = {err_r:.2e}, max|dP|/max P = {err_p:.2e} (cap {CAP:.0e}), peak ({r['peak_bin']}, {r['peak_code']}), "
          f"phase {r['sec_phase']}, k {r['fine_idx']}, ratio {r['peak_ratio']:.3f}")
    assert R.shape == R_m.shape and P.shape == P_m.shape, tag
    assert err_r <= CAP and err_p <= CAP, tag
    for name in ("peak_bin", "peak_code", "fine_idx", "sec_phase"):
        assert int(r[name]) == int(m[name]), (tag, name)
    assert r["carrier_hz"] == m["carrier_hz"] and r["reserved"] == 0, tag
    assert abs(r["peak"] - m["peak"]) <= CAP * R_m.max() and abs(r["peak_ratio"] - m["peak_ratio"]) <= 2 * CAP * (1 + m["peak_ratio"]) * m["peak_ratio"], tag
    assert abs(r["power"] - m["power"]) <= CAP * P_m.max() and abs(r["power_other"] - m["power_other"]) <= CAP * P_m.max(), tag
    # what the call returns hangs together: the results are the map's and the table's own entries, bit for bit
    assert r["peak"] == R[0, r["peak_bin"], r["peak_code"]] and r["power"] == P[0, r["sec_phase"], r["fine_idx"]], tag
    assert r["peak"] == np.sqrt(r["power"]), tag
    if c["mode"] == 0:
        bound = CAP * np.sqrt(P_m.max())
        assert abs(r["prompt_re"] - m["prompt_re"]) <= bound and abs(r["prompt_im"] - m["prompt_im"]) <= bound, tag
    else:
        assert r["prompt_re"] == 0.0 and r["prompt_im"] == 0.0, tag


# ------------------------------------------------------------------------------------------------ 1-5. parity
@pytest.mark.parametrize("name", cc.PARITY_NAMES)
def test_parity(engine, name):
    c = cc.case(name)
    stage(engine, c["raw"], c["codes"])
    got = run(engine, c)
    check_parity(got, cc.model(name), c, name, ties=name in cc.TIES)
    r = got[0][0]
    assert abs(int(r["peak_code"]) - c["true_code"]) <= 1 and r["sec_phase"] == c["true_phase"]
    if name == "m2":               # the two hypotheses tie bit for bit
        assert got[2][0, 0].tobytes() == got[2][0, 1].tobytes() and r["sec_phase"] == 0 and r["power_other"] == r["power"]
    if name.startswith("k63"):
        assert got[2].shape[2] == 63 and r["fine_idx"] == (0 if name == "k63first" else 62)
    if name == "k1":
        assert got[2].shape[2] == 1
    if name in ("lag0", "lagN1"):
        assert r["peak_code"] == (0 if name == "lag0" else c["N"] - 1)
    # the tables are optional
    assert run(engine, c, want=False)[0].tobytes() == got[0].tobytes()


# ------------------------------------------------------------------------------------------------ 6. ring formats, the ring's end
@pytest.mark.parametrize("fmt_name", ["ci16", "cf32", "cf64"])
def test_parity_other_ring_formats(engine, fmt_name):
    c = cc.case("pilot")
    if fmt_name == "ci16":
        stage(engine, c["raw"].astype(np.int16), c["codes"], FMT_CI16)
    else:
        stage(engine, c["rf"], c["codes"], FMT_CF32 if fmt_name == "cf32" else FMT_CF64)      # (small integers: exact in float32)
    check_parity(run(engine, c), cc.model("pilot"), c, fmt_name)


def test_parity_window_across_the_rings_end(engine):
    """A ring of the window + 8 samples, written so that the window starts three and a half periods before the ring's end."""
    c = cc.case("pilot")
    cap = (c["M"] + 1) * c["N"] + 8
    piece = c["raw"][2 * c["start"]:2 * (c["start"] + cap)]
    assert piece.size == 2 * cap and cap % 8 == 0
    offset = cap - 3 * c["N"] - c["N"] // 2
    stage(engine, piece, c["codes"], capacity=cap, offset=offset)
    ring = np.roll(orc.iq_to_complex(piece), offset)
    mdl = cc.statement(c, rf=ring, start=offset)
    check_parity(run(engine, c, start=offset), mdl, c, "wrap")
    assert mdl[0].tobytes() == cc.model("pilot")[0].tobytes()        # (the same samples, the same sums)


# ------------------------------------------------------------------------------------------------ 7. one call against separate calls
def test_three_slots_three_rows_in_one_call_and_one_by_one(engine):
    c = cc.case("pilot")
    secs = np.stack([sc.ROW_B, c["secs"][0], cc.ROW_C])
    codes = np.stack([c["codes"][0], c["codes"][0], orc.gold_code(9)])
    stage(engine, c["raw"], codes)
    res, R, P = run(engine, c, codes=codes, secs=secs, rows=[2, 1, 0])
    assert res[1]["sec_phase"] == c["true_phase"] and res[1]["peak_code"] == c["true_code"] and res[1]["peak_ratio"] > 2.0
    for p, row in enumerate([2, 1, 0]):
        one = run(engine, c, codes=codes[p:p + 1], slots=[p + 1], secs=secs[row:row + 1], rows=[0])
        assert one[0].tobytes() == res[p:p + 1].tobytes() and one[1].tobytes() == R[p:p + 1].tobytes(), p
        assert one[2].tobytes() == P[p:p + 1].tobytes(), p
    assert np.array_equal(res[1:2], run(engine, c, codes=codes[1:2], slots=[2])[0])


@pytest.mark.parametrize("units", [2, 1, 5])
def test_bits_do_not_depend_on_the_cut_of_the_scratch(units):
    """A budget of `units` (PRN, bin) units of 20 x 8000 complex doubles: one PRN's five bins in three chunks (2), a unit per
    chunk (1), a PRN per chunk (5) -- against the default's single chunk of both PRNs."""
    c = cc.case("pilot")
    codes = np.stack([c["codes"][0], orc.gold_code(9)])
    e = Engine(0)
    try:
        stage(e, c["raw"], codes)
        whole = run(e, c, codes=codes, rows=[0, 0])
        e.set_option("coherent_scratch_kb", units * 20 * 8000 * 16 // 1024)
        cut = run(e, c, codes=codes, rows=[0, 0])
        e.set_option("coherent_scratch_kb", 0)
        again = run(e, c, codes=codes, rows=[0, 0])
    finally:
        e.close()
    assert same(whole, cut) and same(whole, again)


# ------------------------------------------------------------------------------------------------ 8. determinism, history
def test_two_identical_calls_return_identical_bytes(engine):
    c = cc.case("data")
    stage(engine, c["raw"], c["codes"])
    assert same(run(engine, c), run(engine, c))


def test_bits_do_not_depend_on_the_engines_history():
    """sdr_pcps, sdr_pcps_signal pad 0 and 1 at another rate, sdr_acq_secondary, then the call: a fresh engine's bytes."""
    c = cc.case("pilot")
    d = cc.case("chirpz")

    def staged(case):
        e = Engine(0)
        stage(e, case["raw"], case["codes"])
        return e

    fresh = staged(c)
    try:
        want = run(fresh, c)
    finally:
        fresh.close()
    used = staged(d)
    try:
        used.pcps_signal([1], 0, d["fs"], 0.0, 2000.0, 250.0, d["code_hz"], pad=0, noncoh=2, want_map=True, n_chips=1019)
        used.pcps_signal([1], 0, d["fs"], 0.0, 2000.0, 250.0, d["code_hz"], pad=1, noncoh=2, want_map=True, n_chips=1019)
        run(used, d)
        stage(used, c["raw"], c["codes"])
        used.pcps([1], 0, 4e6, 0.0, 5000.0, 250.0, 1, 1)
        used.acq_secondary(make_secondary_items(1, 0, c["s0"], c["f0"], orc.CODE_RATE), sc.NH20, 4e6, 20, 4, want_tables=True)
        used.pcps_signal([1], c["start"], 4e6, c["if_hz"], 500.0, 250.0, orc.CODE_RATE, pad=1, noncoh=20)
        assert same(run(used, c), want)
        run(used, c, M=7, span=50.0)
        assert same(run(used, c), want)
    finally:
        used.close()


# ------------------------------------------------------------------------------------------------ 9. end to end, weak
@pytest.mark.parametrize("name", cc.WEAK_NAMES)
def test_end_to_end_weak_signal(engine, name):
    c = cc.case(name)
    stage(engine, c["raw"], c["codes"])
    r = run(engine, c, want=False)[0][0]
    pb, pc, pr, _ = engine.pcps_signal([1], c["start"], c["fs"], c["if_hz"], c["range"], c["step"], c["code_hz"], pad=1, noncoh=c["M"])
    print(f"{name}: coherent ratio {r['peak_ratio']:.3f} at ({r['peak_bin']}, {r['peak_code']}), phase {r['sec_phase']}, "
          f"{r['carrier_hz']} Hz; padded non-coherent ratio {pr[0]:.3f} at ({pb[0]}, {pc[0]})")
    assert r["peak_ratio"] >= 1.5 > pr[0]
    assert cc.coarse_ok(c, r["peak_bin"]) and abs(int(r["peak_code"]) - c["true_code"]) <= 1
    assert r["sec_phase"] == c["true_phase"] and abs(r["carrier_hz"] - c["doppler"]) <= c["fine"] / 2
    m = cc.model(name)[0][0]
    assert [int(r[k]) for k in ("peak_bin", "peak_code", "fine_idx", "sec_phase")] == [int(m[k]) for k in ("peak_bin", "peak_code", "fine_idx", "sec_phase")]


# ------------------------------------------------------------------------------------------------ 10. end to end, two routes
def test_end_to_end_agrees_with_acq_secondary(engine):
    c = cc.case("strong")
    stage(engine, c["raw"], c["codes"])
    r = run(engine, c, want=False)[0][0]
    bins = np.arange(-c["range"], c["range"] + 1, c["step"])
    coarse = c["if_hz"] - bins[r["peak_bin"]]
    start = c["start"] + int(r["peak_code"])
    res = engine.acq_secondary(make_secondary_items(1, 0, start, coarse, c["code_hz"]), c["secs"][0], c["fs"], c["M"], 4, c["span"],
                               c["fine"], 0)[0]
    print(f"coherent: phase {r['sec_phase']}, {r['carrier_hz']} Hz; acq_secondary from ({start}, {coarse}): phase "
          f"{res['sec_phase']}, {res['fine_hz']} Hz")
    assert res["sec_phase"] == r["sec_phase"] == c["true_phase"]
    assert abs(res["fine_hz"] - r["carrier_hz"]) <= c["fine"]


def test_function_level_coherent_search():
    from sydr_amd.dsp.signalsearch import CoherentSearch
    c = cc.case("pilot")
    seg = c["rf"][c["start"]:c["start"] + (c["M"] + 1) * c["N"]]
    cmap, peak, ratio, carrier, phase, pratio = CoherentSearch(seg, c["if_hz"], c["fs"], c["codes"][0], c["code_hz"], c["secs"][0],
                                                               c["range"], c["step"], c["M"], c["span"], c["fine"])
    m = cc.model("pilot")[0][0]
    assert cmap.shape == (5, 4000) and peak == [int(m["peak_bin"]), int(m["peak_code"])] and carrier == m["carrier_hz"]
    assert phase == c["true_phase"] and ratio > 5.0 and pratio > 2.0


# ------------------------------------------------------------------------------------------------ 11. refusals
def test_refused_calls_leave_the_engine_as_it_was(engine):
    c = cc.case("pilot")
    stage(engine, c["raw"], c["codes"])
    good = run(engine, c)
    zero_chip = c["secs"].copy()
    zero_chip[0, 7] = 0
    short = c["rf"].size // c["N"]                         # M + 1 periods are read: one more than the ring holds
    for over, status in ((dict(M=1), INVALID), (dict(M=129), INVALID), (dict(secs=np.ones((1, 1), np.int8)), INVALID),
                         (dict(secs=np.ones((1, 129), np.int8)), INVALID), (dict(secs=zero_chip), INVALID),
                         (dict(secs=np.stack([c["secs"][0]] * 2)), INVALID),          # more rows than PRNs
                         (dict(rows=[1]), INVALID), (dict(rows=[-1]), INVALID), (dict(mode=2), INVALID),
                         (dict(fine=0.0), INVALID), (dict(span=float("nan")), INVALID), (dict(code_hz=0.0), INVALID),
                         (dict(excl=-1), INVALID), (dict(excl=2000), INVALID), (dict(step=0.0), INVALID),
                         (dict(slots=[0]), INVALID),                                  # nothing staged there
                         (dict(slots=[]), INVALID), (dict(fs=float("inf")), INVALID),
                         (dict(span=160.0, fine=5.0), UNSUPPORTED),                   # K = 65
                         (dict(secs=np.ones((1, 128), np.int8), span=400.0, fine=25.0), UNSUPPORTED),      # 128 x 33 cells
                         (dict(fs=4.5e10), UNSUPPORTED),                              # T = 9e7
                         (dict(M=short), RANGE),
                         (dict(start=-1), RANGE)):
        with pytest.raises(_lib.SdrError) as err:
            run(engine, c, **over)
        assert err.value.status == status and str(err.value), (over, err.value.status)
        assert same(run(engine, c), good), over
    lib = _lib.load()
    res = np.zeros(1, dtype=_lib.COH_RESULT_DTYPE)
    cfg = _lib.CohCfg(c["code_hz"], c["span"], c["fine"], c["M"], 20, 0, 0, (C.c_int32 * 2)(0, 0))
    slots, rows, sec = np.array([1], np.int32), np.array([0], np.int32), np.ascontiguousarray(c["secs"])
    byref = C.byref

    def call(cfg_p, slots_p, rows_p, sec_p, res_p):
        return lib.sdr_pcps_coherent(engine._h, cfg_p, slots_p, rows_p, 1, sec_p, 1, c["start"], c["fs"], c["if_hz"], c["range"],
                                     c["step"], res_p, None, None, None, None)

    p = _lib.ptr
    assert call(None, p(slots), p(rows), p(sec), p(res)) == INVALID and b"cfg" in lib.sdr_last_error()
    assert call(byref(cfg), None, p(rows), p(sec), p(res)) == INVALID and b"code_slots" in lib.sdr_last_error()
    assert call(byref(cfg), p(slots), None, p(sec), p(res)) == INVALID and b"sec_rows" in lib.sdr_last_error()
    assert call(byref(cfg), p(slots), p(rows), None, p(res)) == INVALID and b"sec_codes" in lib.sdr_last_error()
    assert call(byref(cfg), p(slots), p(rows), p(sec), None) == INVALID and b"results" in lib.sdr_last_error()
    cfg.reserved[1] = 1
    assert call(byref(cfg), p(slots), p(rows), p(sec), p(res)) == INVALID and b"reserved" in lib.sdr_last_error()
    cfg.reserved[1] = 0
    assert call(byref(cfg), p(slots), p(rows), p(sec), p(res)) == 0 and res.tobytes() == good[0].tobytes()
    with pytest.raises(_lib.SdrError) as err:
        engine.set_option("coherent_scratch_kb", -1)
    assert err.value.status == RANGE
    fresh = Engine(0)
    try:
        with pytest.raises(_lib.SdrError) as err:
            run(fresh, c, want=False)
        assert err.value.status == STATE
        fresh.iq_alloc(1024, FMT_CI8)
        with pytest.raises(_lib.SdrError) as err:
            run(fresh, c, want=False)
        assert err.value.status == STATE and "slots" in str(err.value)
    finally:
        fresh.close()
