"""GPU parity at the edges of the map-free acquisition routes: the crafted streams of tests/pcps_edge_cases.py (every bin
of the Doppler grid a winning row over the rotations; first and second peaks on the row's ends and on the boundary columns
of the two-peak exclusion window) through ROUTE_FUSED (25 and 50 MHz), ROUTE_FUSED10K, ROUTE_SWEEPS and ROUTE_MAP
(pcps_plan.h: plan_pcps) -- indices equal to the oracle's, ratios within 1e-9 relative, and each call against the same call
taken off its route (general kernels, two-kernel sweeps, the map written): equal indices, ratios to rounding.
tests/test_pcps_edge_cases.py shows on the CPU that every one-column change of the window rule moves some ratio of every
stream by more than 1e-3."""
import numpy as np
import pytest

import pcps_edge_cases as pec
from sydr_amd.engine import FMT_CF64, FMT_CI8, FMT_CI16

pytestmark = pytest.mark.gpu

RATIO_RTOL = 1e-9          # against the oracle: the bar of tests/test_gpu_pcps.py
ROUTES_RTOL = 1e-12        # between two routes of the library: the same sums in another order
OPTION_DEFAULTS = {"pcps_fused": 1, "pcps_general_kernels": 0, "pcps_one_stream": 0, "pcps_prn_chunk": 0,
                   "pcps_no_shared_spectra": 0}
OFF_ROUTE = {"pcps_fused": 0, "pcps_general_kernels": 1}


def _id(case):
    return f"{case.fs / 1e6:g}MHz-step{case.dstep:g}-if{case.if_hz:g}-x{case.noncoh}-rot{case.rotation}"


def _stage(engine, case, fmt=FMT_CI8, start=0, capacity=None, split=None):
    """The case's stream into a ring of `fmt` at `start` (wrapping where the ring ends), in two uploads when `split`."""
    st = pec.stream(case)
    total = st.raw.size // 2
    cap = capacity or (total + start + 7) // 8 * 8
    engine.iq_alloc(cap, fmt)
    data = st.rf if fmt == FMT_CF64 else st.raw.astype(np.int16) if fmt == FMT_CI16 else st.raw
    per = 1 if fmt == FMT_CF64 else 2           # array elements per sample
    if split:
        engine.iq_upload(data[:per * split], start)
        engine.iq_upload(data[per * split:], (start + split) % cap)
    else:
        engine.iq_upload(data, start)
    engine.code_slots(len(pec.PRNS))
    for slot, prn in enumerate(pec.PRNS):
        engine.load_gps_code(slot, prn)


def _pcps(engine, case, start=0, want_map=False, **options):
    try:
        for name, value in options.items():
            engine.set_option(name, value)
        return engine.pcps(np.arange(len(pec.PRNS)), start, case.fs, case.if_hz, case.drange, case.dstep, 1, case.noncoh,
                           want_map=want_map)
    finally:
        for name in options:
            engine.set_option(name, OPTION_DEFAULTS[name])


def _vs_oracle(case, got, label):
    """indices equal to the oracle's, ratios within RATIO_RTOL; prints and returns the worst relative ratio error"""
    st, exp = pec.stream(case), pec.expected(case)
    pb, pc, pr = got[:3]
    worst = 0.0
    for i, e in enumerate(exp):
        assert e.peak == [st.bins[i], st.cols[i]]               # (the stream is what the CPU test says it is)
        worst = max(worst, abs(float(pr[i]) / e.ratio - 1.0))
    print(f"{label} {_id(case)}: worst relative ratio error {worst:.3g}")
    for i, e in enumerate(exp):
        assert [int(pb[i]), int(pc[i])] == e.peak, (label, st.names[i])
        assert pr[i] == pytest.approx(e.ratio, rel=RATIO_RTOL), (label, st.names[i])
    return worst


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    np.testing.assert_allclose(a[2], b[2], rtol=ROUTES_RTOL, atol=0)


def _on_and_off_route(engine, case, label, start=0, **options):
    """The call on its route (map-free) against the oracle, and against the same call with the general kernels, the
    two-kernel sweeps and the map written."""
    got = _pcps(engine, case, start, **options)
    assert got[3] is None
    _vs_oracle(case, got, label)
    off = _pcps(engine, case, start, want_map=True, **OFF_ROUTE)
    _same(got, off)
    return got, off


def _fills_a_fused_round(case):
    """transforms x operand terms >= 256: the search fills a round of the fused sweep's persistent workgroups"""
    n, _, _ = pec.geometry(case.fs)
    terms = {25000: 1, 50000: 2}[n]
    return case.noncoh == 1 and len(pec.PRNS) * pec.n_bins(case) * terms >= 256


def _classes(case):
    """P of plan_shared_spectra: the smallest P <= 64 (2 P <= bins) with P x step a whole number of transform bins, or 0"""
    n, _, _ = pec.geometry(case.fs)
    for p in range(1, 65):
        v = p * case.dstep * n / case.fs
        if 2 * p <= pec.n_bins(case) and round(v) >= 1 and abs(v - round(v)) <= 1e-9 * round(v):
            return p
    return 0


@pytest.mark.parametrize("case", pec.rotations(pec.FUSED_25) + [pec.FUSED_25_ODD_IF], ids=_id)
def test_fused_sweep_25mhz_every_bin_and_window_edge(engine, case):
    """ROUTE_FUSED, one operand term: over the four rotations every bin wins, the last bins' single-round short units
    (make_work_list) and the class spectra at their largest and at zero shift included; the fused second sweep applies
    the window at every edge; an intermediate frequency that is a multiple of the step, and one that is not."""
    assert _fills_a_fused_round(case) and _classes(case) == 4 and case.if_hz != 0.0
    _stage(engine, case)
    _on_and_off_route(engine, case, "fused 25 MHz")


@pytest.mark.parametrize("case", pec.rotations(pec.FUSED_50), ids=_id)
def test_fused_sweep_50mhz_every_bin_and_window_edge(engine, case):
    """ROUTE_FUSED, two operand terms, a row's columns split by parity (records carry 2 m + parity): S = 49 is odd, so
    peaks, window edges and second peaks fall on both parities."""
    n, s, _ = pec.geometry(case.fs)
    assert _fills_a_fused_round(case) and (n, s) == (50000, 49)
    st, exp = pec.stream(case), pec.expected(case)
    assert {c % 2 for c in st.cols} == {0, 1}
    assert {(c + s) % 2 for c in st.cols if c + s < n} == {0, 1} == {(c - s - 1) % 2 for c in st.cols if c - s >= 1}
    assert {pec.second_column(e.row, e.peak[1], n, s) % 2 for e in exp} == {0, 1}
    _stage(engine, case)
    _on_and_off_route(engine, case, "fused 50 MHz")


@pytest.mark.parametrize("case", pec.rotations(pec.FUSED_10K) + [pec.FUSED_10K_NONCOH], ids=_id)
def test_fused_search_10mhz_every_bin_and_window_edge(engine, case):
    """ROUTE_FUSED10K (its own first and second maximum per row), 34 bins in ten classes: every bin over three rotations;
    one rotation over three non-coherent blocks at an intermediate frequency."""
    n, _, _ = pec.geometry(case.fs)
    assert n == 10000 and len(pec.PRNS) * pec.n_bins(case) >= 32 and _classes(case) == 10
    _stage(engine, case)
    _on_and_off_route(engine, case, "fused 10 MHz")


@pytest.mark.parametrize("case,options", [(pec.FUSED_25, {"pcps_fused": 0, "pcps_prn_chunk": 5}),
                                          (pec.FUSED_25, {"pcps_fused": 0, "pcps_prn_chunk": 5, "pcps_one_stream": 1}),
                                          (pec.SWEEPS_4, {}), (pec.SWEEPS_12, {})],
                         ids=["25MHz-two-streams", "25MHz-one-stream", "4MHz", "12MHz"])
def test_two_kernel_sweeps_end_bins_and_window_edges(engine, case, options):
    """ROUTE_SWEEPS (the running maximum in the inverse row kernel, then the winning rows again with the window): the
    register-resident 125 x 200 kernels in sweeps of five PRNs on two streams and on one, pcps_fastn.h at 4 MHz, the
    general four-step kernels at 12 MHz -- the end bins among the winners."""
    n, _, _ = pec.geometry(case.fs)
    assert case.noncoh == 1 and (options.get("pcps_fused") == 0 or n not in (10000, 25000, 50000))
    if "pcps_prn_chunk" in options:
        assert len(pec.PRNS) > options["pcps_prn_chunk"]                   # more than one sweep
    assert {0, pec.n_bins(case) - 1} <= set(pec.stream(case).bins)
    _stage(engine, case)
    _on_and_off_route(engine, case, "sweeps", **options)


def test_map_route_winning_rows(engine):
    """ROUTE_MAP on the 25 MHz stream: peak_finish_kernel over the written map, and the winning rows themselves."""
    case = pec.FUSED_25
    _stage(engine, case)
    got = _pcps(engine, case, want_map=True)
    _vs_oracle(case, got, "map")
    _same(got, _pcps(engine, case, want_map=True, **OFF_ROUTE))
    for i, e in enumerate(pec.expected(case)):
        np.testing.assert_allclose(got[3][i, e.peak[0]], e.row, rtol=0, atol=1e-9 * e.row.max())


def test_fused_sweep_without_shared_spectra(engine):
    """One forward transform per bin (`pcps_no_shared_spectra`) against the four class spectra read at a shift."""
    case = pec.FUSED_25._replace(rotation=1)
    assert _fills_a_fused_round(case) and _classes(case) == 4
    _stage(engine, case)
    shared = _pcps(engine, case)
    own = _pcps(engine, case, pcps_no_shared_spectra=1)
    _vs_oracle(case, shared, "fused 25 MHz, shared spectra")
    _vs_oracle(case, own, "fused 25 MHz, a transform per bin")
    _same(shared, own)


@pytest.mark.parametrize("case", pec.rotations(pec.NO_CLASSES), ids=_id)
def test_fused_sweep_on_a_grid_without_classes(engine, case):
    """330 Hz steps at 25 MHz: 100 steps make a whole number of transform bins, over the limit of 64 classes, so the fused
    route transforms each of the 31 bins itself (P = 0) -- every bin a winner over three rotations."""
    assert _fills_a_fused_round(case) and pec.n_bins(case) == 31 and _classes(case) == 0
    _stage(engine, case)
    _on_and_off_route(engine, case, "fused 25 MHz, no classes")


@pytest.mark.parametrize("fmt", [FMT_CI16, FMT_CF64], ids=["ci16", "cf64"])
@pytest.mark.parametrize("case", [pec.FUSED_25._replace(rotation=2), pec.FUSED_10K_NONCOH], ids=_id)
def test_map_free_search_from_a_wrapping_ring_of_other_formats(engine, case, fmt):
    """run_fused / run_fused10k for complex int16 and complex double, the window crossing the ring's end (at 10 MHz inside
    the second of three blocks), the stream uploaded in two pieces."""
    n, _, _ = pec.geometry(case.fs)
    window = n * case.noncoh
    cap = (window * 3 // 2 + 7) // 8 * 8
    start = cap - window // 2 + 3
    assert start + window > cap > start and start % 8
    if case.noncoh > 1:
        assert n < cap - start < 2 * n
        assert n == 10000 and len(pec.PRNS) * pec.n_bins(case) >= 32
    else:
        assert _fills_a_fused_round(case)
    _stage(engine, case, fmt, start, cap, split=window // 3 + 1)
    _on_and_off_route(engine, case, f"ring {fmt}", start)


def test_fused_sweep_from_a_start_above_64(engine):
    case = pec.FUSED_25._replace(rotation=3)
    assert _fills_a_fused_round(case)
    _stage(engine, case, start=4321)
    _on_and_off_route(engine, case, "fused 25 MHz, start 4321", 4321)


@pytest.mark.gpu
def test_acquisition_entry_points_refuse_alike(engine):
    """sdr_pcps, sdr_acq_deep and sdr_serial_search derive what a request means and check it through one header
    (sydr_amd/csrc/acq_request.h): a request wrong in one way gets the same status from all three -- the statuses each has always
    answered -- nothing reaches the device (no profiling scope records), and a good search afterwards returns the bytes it
    returned before.  4 MHz (N = 4000), a ring of 8000 samples, two slots of which one is staged."""
    from sydr_amd import _lib
    from sydr_amd.engine import Engine
    INVALID, RANGE, STATE = -1, -5, -6
    fs = 4e6

    def searches(e, slots=(0,), start=0, step=250.0, blocks=1):
        return (lambda: e.pcps(slots, start, fs, 0.0, 5000.0, step, 1, blocks),
                lambda: e.acq_deep(slots, start, fs, 0.0, 5000.0, step, 1, blocks),
                lambda: e.serial_search(slots, start, fs, 5000.0, step, blocks))

    def refused(e, status, word="", **request):
        for search in searches(e, **request):
            with pytest.raises(_lib.SdrError) as err:
                search()
            assert err.value.status == status and word in str(err.value), (request, str(err.value))

    def good(e):
        pcps, deep, serial = (search() for search in searches(e, blocks=2))
        return b"".join(np.asarray(a).tobytes() for a in (*pcps[:3], deep[0], *serial[:3]))

    engine.iq_alloc(8000, FMT_CI8)
    engine.code_slots(2)
    engine.load_gps_code(0, 9)
    engine.iq_synth([dict(prn=9, doppler=1250.0, code_phase=311.4, phase=0.3, amp=8.0)], fs, 12.0, 5, 0, 8000)
    before = good(engine)
    engine.prof_enable(True)
    engine.prof_reset()
    try:
        refused(engine, INVALID, "not staged", slots=(1,))          # a slot that is not staged
        refused(engine, INVALID, step=0.0)                          # no grid
        refused(engine, RANGE, start=-1)
        refused(engine, RANGE, blocks=3)                            # one block more than the ring holds
        refused(engine, INVALID, slots=())                          # n_prn = 0
        assert engine.prof_read("")[1] == 0                         # no kernel, no scope: nothing reached the device
    finally:
        engine.prof_enable(False)
        engine.prof_reset()
    assert good(engine) == before
    fresh = Engine(0)
    try:
        refused(fresh, STATE, "ring")
        fresh.iq_alloc(8000, FMT_CI8)
        refused(fresh, STATE, "slots")
    finally:
        fresh.close()
