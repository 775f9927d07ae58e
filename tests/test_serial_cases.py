"""The catalogue of tests/serial_cases.py, checked on the oracle alone: the rates have the empty, doubled and rounding-sensitive
chips they are listed for, every compared peak is clear of a tie, the exact-rational chip index and every neighbouring
second-peak rule move a result by far more than the 1e-9 the GPU comparison allows -- the conditions under which
tests/test_gpu_serial_edges.py can fail at all."""
import numpy as np
import pytest

import deep_cases as dc
import serial_cases as sc
from oracle import sydr_oracle as orc

# the exact-rational index must move the map by this much of its maximum: four decades above the GPU comparison's 1e-9
SEEN = 1e-5
# a neighbouring second-peak rule must move some small-map ratio by this much
SEEN_RULE = 1e-3
FS = 4e6


def _clear_of_a_tie(m, what):
    margin = dc.top2_margin(m)
    assert margin > dc.MARGIN, (what, margin)
    return margin


@pytest.mark.parametrize("rate", sc.RATES, ids=sc.RATE_IDS)
def test_rates_have_what_they_are_listed_for(rate):
    assert sc.rate_facts(rate.fs) == rate
    assert orc.samples_per_code(rate.fs) == rate.n
    raw = sc.samples(rate.fs)
    assert len(raw) == 2 * rate.n and int(np.max(np.abs(raw.astype(np.int16)))) < 127       # no sample clips
    for prn in (sc.SAT["prn"], sc.ABSENT_PRN):
        _clear_of_a_tie(sc.ref_map(rate.fs, prn), (rate.fs, prn))
    peak, ratio = orc.two_peak_compare_ss(sc.ref_map(rate.fs, sc.SAT["prn"]))
    assert peak == sc.PEAK and ratio > 2.0
    assert orc.two_peak_compare_ss(sc.ref_map(rate.fs, sc.ABSENT_PRN))[1] < 1.5


def test_rates_of_the_earlier_suite_have_no_sensitive_sample():
    """why 4, 10, 12, 25 and 50 MHz could not tell one index arithmetic from another"""
    for fs in (4e6, 10e6, 12e6, 25e6, 50e6):
        assert np.array_equal(orc.upsample_index(fs), sc.exact_index(fs))


@pytest.mark.parametrize("rate", [r for r in sc.RATES if r.sensitive], ids=[i for i, r in zip(sc.RATE_IDS, sc.RATES) if r.sensitive])
def test_exact_rational_index_would_show(rate):
    """The chip-sum statement with the oracle's index is the oracle's map; with the exact quotient's index (clipped to 1022)
    it is not, by more than SEEN of the maximum.  Measured: 1.3e-2 (1.023 MHz), 4.0e-3 (2.046), 6.2e-3 (4.092), 1.6e-3
    (16.368), 1.9e-4 (38.192)."""
    prn = sc.SAT["prn"]
    ref = sc.ref_map(rate.fs, prn)
    rf = sc.block(sc.samples(rate.fs), rate.fs, 0)
    same = sc.chipsum_map(rf, orc.gold_code(prn), sc.GRID, rate.fs, orc.upsample_index(rate.fs))
    assert np.max(np.abs(same - ref)) <= 1e-12 * ref.max()
    exact = np.minimum(sc.exact_index(rate.fs), orc.CODE_CHIPS - 1)
    other = sc.chipsum_map(rf, orc.gold_code(prn), sc.GRID, rate.fs, exact)
    moved = float(np.max(np.abs(other - ref)) / ref.max())
    print(f"{rate.fs / 1e6:g} MHz: exact-rational index moves the map by {moved:.2e} of its maximum "
          f"(chip sums reproduce the oracle to {float(np.max(np.abs(same - ref)) / ref.max()):.1e})")
    assert moved > SEEN


@pytest.mark.parametrize("length", sc.LENGTHS)
def test_length_cases(length):
    """both grids' maps are clear of a tie, and the chips past 1022 -- on which no sample lands -- are read through the shift"""
    code = ("random", length)
    assert len(sc.random_code(length)) == length and set(np.unique(sc.random_code(length))) == {-1, 1}
    for grid, bins in ((sc.ONE_BIN, 1), (sc.GRID, 5)):
        m = sc.ref_map(FS, code, grid)
        assert m.shape == (bins, length)
        _clear_of_a_tie(m, (length, grid))
        if length > orc.CODE_CHIPS:
            tail = m[:, orc.CODE_CHIPS:]
            assert tail.size == bins * (length - orc.CODE_CHIPS)
            assert tail.size == 1 or not np.all(tail == tail.flat[0])       # (1024 chips, one bin: a single column)
    # the same samples on the same chips, a different code behind them: the map is another one
    if length > orc.CODE_CHIPS:
        head = orc.serial_search(sc.block(sc.samples(FS), FS, 0), sc.random_code(length)[:orc.CODE_CHIPS].astype(np.float64),
                                 *sc.ONE_BIN, FS, 4000)
        assert not np.array_equal(head, sc.ref_map(FS, code, sc.ONE_BIN)[0, :orc.CODE_CHIPS])


def test_short_code_follows_the_index():
    """1022 chips: the reference's fancy index raises at 4 MHz (highest index 1022) and works at 1.0 MHz (1021)"""
    assert int(orc.upsample_index(FS).max()) + 1 == 1023 > sc.SHORT
    with pytest.raises(IndexError):
        sc.ref_map(FS, ("random", sc.SHORT), sc.ONE_BIN)
    assert int(orc.upsample_index(1.0e6).max()) + 1 == sc.SHORT
    m = sc.ref_map(1.0e6, ("random", sc.SHORT))
    assert m.shape == (5, sc.SHORT)
    _clear_of_a_tie(m, "1022 chips at 1.0 MHz")


def test_block_sums_and_seam():
    blocks = max(sc.NONCOH)
    raw = sc.samples(FS, blocks)
    assert len(raw) == 2 * blocks * 4000 and int(np.max(np.abs(raw.astype(np.int16)))) < 127
    parts = [sc.ref_block_map(FS, sc.SAT["prn"], sc.GRID, k, blocks) for k in range(blocks)]
    for noncoh in sc.NONCOH:
        m = sc.ref_map(FS, sc.SAT["prn"], sc.GRID, noncoh, blocks)
        assert np.array_equal(m, np.add.accumulate(parts[:noncoh])[-1])                      # added in block order
        _clear_of_a_tie(m, noncoh)
        assert orc.two_peak_compare_ss(m)[0] == sc.PEAK
    cap, start, noncoh = sc.SEAM["capacity"], sc.SEAM["start"], sc.SEAM["noncoh"]
    assert start % 2 == 1 and start + 4000 < cap < start + 2 * 4000 and noncoh * 4000 <= cap     # the second block straddles
    _clear_of_a_tie(sc.ref_map(FS, sc.SAT["prn"], sc.GRID, noncoh), "seam")


def test_many_prn_entries():
    entries = sc.many_entries()
    n_slots = len(sc.MANY["prns"])
    assert len(entries) == sc.MANY["entries"] == 40 and set(entries.tolist()) == set(range(n_slots)) and n_slots == 8
    where = np.nonzero(entries == sc.MANY["repeated"])[0]
    assert len(where) == 5 and np.all(np.diff(where) >= 1) and where[0] == 0 and where[-1] == 39 and np.max(np.diff(where)) > 5
    assert len({int(entries[i]) for i in sc.MANY["oracle_entries"]}) == 3
    assert sc.MANY["prns"][int(entries[sc.MANY["oracle_entries"][0]])] == sc.SAT["prn"]
    for i in sc.MANY["oracle_entries"]:
        _clear_of_a_tie(sc.ref_map(FS, sc.MANY["prns"][int(entries[i])], sc.GRID, sc.MANY["noncoh"]), i)


@pytest.mark.parametrize("doppler", list(sc.CORNER_DOPPLERS))
@pytest.mark.parametrize("phase", list(sc.CORNER_PHASES))
def test_corner_placements(doppler, phase):
    m = sc.ref_map(FS, sc.SAT["prn"], sc.GRID, 1, 1, doppler, phase)
    assert int(np.max(np.abs(sc.samples(FS, 1, doppler, phase).astype(np.int16)))) < 127
    _clear_of_a_tie(m, (doppler, phase))
    peak, ratio = orc.two_peak_compare_ss(m)
    assert peak == [sc.CORNER_DOPPLERS[doppler], sc.CORNER_PHASES[phase]]
    if peak[0] == 0 or peak[1] == 0:
        assert ratio == 1.0            # a block that starts at -1 selects nothing: the peak is its own second peak
    else:
        assert sc.INTERIOR_RATIO[0] < ratio < sc.INTERIOR_RATIO[1]
    assert sc.ratio_under(m) == ratio


def test_small_maps_and_neighbouring_rules():
    """`ratio_under` restates the oracle's rule on every small-map placement, and every neighbouring rule changes some
    placement's ratio."""
    moved = dict.fromkeys(sc.RULES, 0.0)
    count = 0
    for shape in sc.SMALL_SHAPES:
        for m in sc.small_maps(shape):
            peak, ratio = orc.two_peak_compare_ss(m)
            assert m[peak[0], peak[1]] == sc.TOP and sc.ratio_under(m) == ratio
            for rule in sc.RULES:
                moved[rule] = max(moved[rule], abs(sc.ratio_under(m, rule) / ratio - 1.0))
            count += 1
    print(f"{count} small maps; largest relative change of a ratio per neighbouring rule:",
          {rule: f"{v:.3g}" for rule, v in moved.items()})
    assert count == sum(r * c * (r * c - 1) for r, c in sc.SMALL_SHAPES) == 9318
    assert all(v > SEEN_RULE for v in moved.values()), moved
    with pytest.raises(ValueError):
        sc.ratio_under(np.ones((2, 2)), "no such rule")


def test_small_map_rows_meet_every_clamp():
    """maps of 1, 2 and 3 rows: a block that starts at -1 still selects row 0 of one row and row 1 of two rows"""
    one = np.full((1, 16), 0.5)
    one[0, 5], one[0, 6], one[0, 9] = sc.TOP, sc.SECOND, 2.0
    assert orc.two_peak_compare_ss(one) == ([0, 5], sc.TOP / 2.0)             # [-1:2] of one row is that row
    two = np.full((2, 17), 0.5)
    two[0, 5], two[1, 5], two[0, 6] = sc.TOP, sc.SECOND, 2.0
    assert orc.two_peak_compare_ss(two) == ([0, 5], 1.0)                      # [-1:2] of two rows is row 1: the peak stays
    two[1, 5], two[0, 5] = sc.TOP, sc.SECOND
    assert orc.two_peak_compare_ss(two) == ([1, 5], sc.TOP / 0.5)             # [0:3] of two rows is both
    three = np.full((3, 16), 0.5)
    three[0, 5], three[1, 5] = sc.TOP, sc.SECOND
    assert orc.two_peak_compare_ss(three) == ([0, 5], 1.0)                    # [-1:2] of three rows is empty
    for m in (one, two, three):
        assert sc.ratio_under(m) == orc.two_peak_compare_ss(m)[1]


def test_tie_maps():
    names = [name for name, _ in sc.tie_maps()]
    assert len(set(names)) == len(names) == 7
    for name, m in sc.tie_maps():
        first = np.unravel_index(int(np.argmax(m)), m.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            peak, ratio = orc.two_peak_compare_ss(m)
        assert peak == [int(first[0]), int(first[1])], name
        if name == "all zero":
            assert peak == [0, 0] and np.isnan(ratio)
        elif name == "two equal maxima, neighbours":
            assert ratio > 1.0
        else:
            assert ratio == 1.0, name
        assert np.count_nonzero(m == m.max()) >= 2
