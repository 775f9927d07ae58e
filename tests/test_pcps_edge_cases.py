"""The crafted acquisition streams of tests/pcps_edge_cases.py, checked on the oracle alone: every peak lands on its placed
(bin, column), `ratio_under` restates the oracle's window rule, and every neighbouring rule (an edge one column off, the
last column allowed, the window taken circularly) changes some placement's ratio by far more than the 1e-9 the GPU
comparison allows -- the condition under which tests/test_gpu_pcps_edges.py can fail at all."""
import numpy as np
import pytest

import pcps_edge_cases as pec
from oracle import sydr_oracle as orc

# every rotation of the 25 MHz and 10 MHz grids, one of the others (their maps take longer or their route has one test)
CASES = (pec.rotations(pec.FUSED_25) + pec.rotations(pec.FUSED_25_ODD_IF, 1) + pec.rotations(pec.FUSED_10K)
         + pec.rotations(pec.FUSED_10K_NONCOH, 1) + pec.rotations(pec.NO_CLASSES) + pec.rotations(pec.FUSED_50, 1)
         + pec.rotations(pec.SWEEPS_4, 1) + pec.rotations(pec.SWEEPS_12, 1))
# a neighbouring rule must move some ratio by this much: six decades above the GPU comparison's 1e-9
SEEN = 1e-3


def _id(case):
    return f"{case.fs / 1e6:g}MHz-step{case.dstep:g}-if{case.if_hz:g}-x{case.noncoh}-rot{case.rotation}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_peaks_land_where_placed_and_every_neighbouring_rule_shows(case):
    n, s, _ = pec.geometry(case.fs)
    st, exp = pec.stream(case), pec.expected(case)
    assert st.clipped == 0 and int(np.max(np.abs(st.raw))) < 127
    moved = dict.fromkeys(pec.NEIGHBOURS, 0.0)
    for i, e in enumerate(exp):
        assert e.peak == [st.bins[i], st.cols[i]], st.names[i]
        assert e.row[e.peak[1]] == e.row.max()
        assert pec.ratio_under(e.row, e.peak[1], n, s) == e.ratio, st.names[i]
        for rule in pec.NEIGHBOURS:
            moved[rule] = max(moved[rule], abs(pec.ratio_under(e.row, e.peak[1], n, s, rule) / e.ratio - 1.0))
    print({rule: f"{v:.3g}" for rule, v in moved.items()})
    assert all(v > SEEN for v in moved.values()), moved


@pytest.mark.parametrize("case", [pec.FUSED_25, pec.FUSED_10K, pec.NO_CLASSES, pec.FUSED_50, pec.SWEEPS_4, pec.SWEEPS_12], ids=_id)
def test_every_bin_wins_over_the_rotations(case):
    nbins = pec.n_bins(case)
    assert nbins == {250.0: 41, 300.0: 34, 330.0: 31}[case.dstep]
    won = [b for r in range(pec.n_rotations(case)) for b in pec.winning_bins(nbins, r)]
    assert set(won) == set(range(nbins))
    assert {0, 1, nbins - 2, nbins - 1} <= set(pec.winning_bins(nbins, 0))     # the end bins and their neighbours at once
    assert len(set(pec.winning_bins(nbins, 0))) == len(pec.PRNS)


def test_window_rules_on_a_small_row():
    """`allowed_columns` against the oracle's two_peak_compare on rows short enough to enumerate: every peak column of a
    row of 40 with S = 4, the second peak planted on each column in turn."""
    n, s = 40, 4
    for top in range(n):
        cols = set(pec.allowed_columns(top, n, s).tolist())
        for second in range(n):
            if second == top:
                continue
            m = np.ones((2, n))
            m[1, top], m[1, second] = 9.0, 3.0
            _, ratio = orc.two_peak_compare(m, n, s)
            assert (ratio == 3.0) == (second in cols), (top, second)
    interior = 20
    assert set(pec.allowed_columns(interior, n, s).tolist()) == set(range(0, 16)) | set(range(24, 39))
    assert set(pec.allowed_columns(interior, n, s, "left_lower").tolist()) == set(range(0, 15)) | set(range(24, 39))
    assert set(pec.allowed_columns(interior, n, s, "left_higher").tolist()) == set(range(0, 17)) | set(range(24, 39))
    assert set(pec.allowed_columns(interior, n, s, "right_lower").tolist()) == set(range(0, 16)) | set(range(23, 39))
    assert set(pec.allowed_columns(interior, n, s, "right_higher").tolist()) == set(range(0, 16)) | set(range(25, 39))
    assert set(pec.allowed_columns(interior, n, s, "last_allowed").tolist()) == set(range(0, 16)) | set(range(24, 40))
    assert set(pec.allowed_columns(interior, n, s, "circular").tolist()) == set(pec.allowed_columns(interior, n, s).tolist())
    assert set(pec.allowed_columns(0, n, s, "circular").tolist()) == set(range(4, 36))
    assert set(pec.allowed_columns(0, n, s).tolist()) == set(range(4, 39))


def test_boundary_columns_fall_on_both_parities_at_50_mhz():
    """The 50 MHz sweep splits a row's columns by parity (2 m + parity): S = 49 is odd, so the placements put first peaks,
    window edges and second peaks on even and on odd columns."""
    case = pec.FUSED_50
    n, s, _ = pec.geometry(case.fs)
    assert (n, s) == (50000, 49)
    st, exp = pec.stream(case), pec.expected(case)
    assert {c % 2 for c in st.cols} == {0, 1}
    assert {(c + s) % 2 for c in st.cols if c + s < n} == {0, 1}
    assert {(c - s - 1) % 2 for c in st.cols if c - s >= 1} == {0, 1}
    assert {pec.second_column(e.row, e.peak[1], n, s) % 2 for e in exp} == {0, 1}
