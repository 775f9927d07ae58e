"""CPU half of the engine-history tests: the catalogue of tests/engine_history_cases.py is what it says it is.  Every probe
whose call decides something (a peak, an index, a sign, a lock state, an epoch length, a kernel variant, a rounded ring sample)
has a reference that is clear of a tie or threshold by more than MARGIN, so two correct computations cannot disagree on it; the
seven that decide nothing are named with their reasons; the grids of the fused probes have the bin counts and the classes
the stale-work-list sequence needs; and the bytes of a probe's outputs are a function of every output."""
import numpy as np
import pytest

import engine_history_cases as ehc


@pytest.mark.parametrize("name", [n for n in ehc.NAMES if n not in ehc.DECIDES_NOTHING])
def test_reference_decision_has_margin(name):
    probe = ehc.PROBES[name]
    m = probe.margin()
    print(f"{name}: margin {m}")
    assert probe.decides and m is not None and m > ehc.MARGIN, (name, m)


def test_probes_without_a_margin_are_the_named_ones():
    """Seven probes return sums, exact counts or table look-ups: each is named with its reason, and no other probe is let off."""
    assert len(ehc.DECIDES_NOTHING) == 7 and all(ehc.DECIDES_NOTHING.values())
    for name in ehc.DECIDES_NOTHING:
        assert not ehc.PROBES[name].decides and ehc.PROBES[name].margin() is None
    assert sum(p.decides for p in ehc.PROBES.values()) == len(ehc.NAMES) - 7


def test_classless_pair_shares_every_int_of_the_old_key():
    """(n_prn, vbins, block_bins) of the two classless fused probes are equal -- 4 PRNs, 82 = 2 x 41 virtual bins, no classes
    so blocks of 4 bins -- and only the pieces of a left-over transform differ: the pair the parent's key confused."""
    a, b = ehc.PROBES["fused_25mhz_classless"], ehc.PROBES["fused_50mhz_classless"]
    assert a.scene == b.scene == "wide"
    assert len(ehc.orc.doppler_bins(5000.0, 123.0)) == 82 and len(ehc.orc.doppler_bins(5000.0, 247.0)) == 41
    assert ehc.classes(25e6, 82, 123.0) == 0 and ehc.classes(50e6, 41, 247.0) == 0
    assert 4 * 82 == 4 * 2 * 41 == 256 + 72


def test_scenes_fit_their_probes():
    for name in ehc.SCENE_NAMES:
        s = ehc.SCENES[name]
        n = s.image.size if np.iscomplexobj(s.image) else s.image.size // 2
        assert n == s.capacity and s.capacity % 8 == 0 and len(s.slots) >= 2, name
    assert {p.scene for p in ehc.PROBES.values()} == set(ehc.SCENE_NAMES)


def test_bytes_cover_every_output():
    a = (np.arange(3), [np.float64(1.5), None], {"k": 2})
    b = (np.arange(3), [np.float64(1.5), None], {"k": 3})
    c = (np.arange(3).astype(np.int32), [np.float64(1.5), None], {"k": 2})
    assert ehc.to_bytes(a) == ehc.to_bytes(a) and len({ehc.to_bytes(a), ehc.to_bytes(b), ehc.to_bytes(c)}) == 3
