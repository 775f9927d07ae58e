"""The variant word of an E/P/L plan (sydr_amd/csrc/epl_variant.h) -- a HOST build of the header alone
(tests/csrc/epl_variant_dump.hip), no GPU:
  - choose_variant over a grid of list statistics, engine settings and spacings gives, point for point, the words the code
    gave before the word had one decoder and one table (tests/golden/epl_variant_grid.txt: that code's own output over the
    same grid, run-length coded);
  - decode names, for every word of the grid, the kernel bench.kernel_of_variant names (one wave per workgroup, setups
    present: what bench.py models);
  - four waves per workgroup and a plan without setups collapse as written out below;
  - "needs setups" is said exactly of the words with a compile-time tap geometry, and of the several-chip shapes;
  - the rows of the two units' lists of straight-line forms are exactly the tuples decode can ask for."""
import os
import subprocess

import pytest

import host_check
from conftest import REPO

import bench

CI8, CI16 = 0, 1
CHIP, KS_MASK, KI, C2 = 26, 0xF00, 4096, 8192

pytestmark = host_check.requires_hipcc


@pytest.fixture(scope="module")
def exe():
    return host_check.build("epl_variant_dump")


@pytest.fixture(scope="module")
def forms(exe):
    """[(fmt, n_taps, word, nt, wpw, has_setups, form)] of every distinct word of the grid and every chunk of its taps;
    form = dict(shape, fmt, nt, w, km, wpw, ks, ki, km2, row, setups)"""
    names = ("shape", "fmt", "nt", "w", "km", "wpw", "ks", "ki", "km2", "row", "setups")
    out = []
    for line in subprocess.check_output([exe, "decode"], text=True).splitlines():
        key, val = line.split(":")
        out.append(tuple(int(x) for x in key.split()) + (dict(zip(names, (int(x) for x in val.split()))),))
    assert out
    return out


@pytest.fixture(scope="module")
def tables(exe):
    """({(NT, KM, KS, KI): unit}, {shape: "4,9,14,19"}) as the header lists them"""
    rows, shapes = {}, {}
    for line in subprocess.check_output([exe, "rows"], text=True).splitlines():
        kind, rest = line.split(" ", 1)
        if kind == "row":
            unit, *t = rest.split()
            assert tuple(map(int, t)) not in rows, line            # (a tuple is spelled once, in one unit)
            rows[tuple(map(int, t))] = unit
        else:
            index, pack = rest.split(" ", 1)
            shapes[int(index)] = pack.replace(" ", "")
    return rows, shapes


def name_of(f, shapes):
    if f["shape"]:
        return f"epl2_kernel<{shapes[f['shape']]}>"
    return "epl_kernel<" + ",".join(str(f[k]) for k in ("fmt", "nt", "w", "km", "wpw", "ks", "ki", "km2")) + ">"


def test_choose_variant_matches_the_recorded_grid(exe):
    got = subprocess.check_output([exe, "grid"], text=True).splitlines()
    want = open(os.path.join(REPO, "tests", "golden", "epl_variant_grid.txt")).read().splitlines()
    assert sum(int(l.split()[0]) for l in want) == 47520             # (points of the grid)
    assert got == want


def test_decode_names_the_kernel_bench_names(forms, tables):
    checked = set()
    for fmt, n_taps, word, nt, wpw, has, f in forms:
        if fmt == CI8 and wpw == 1 and has:
            assert name_of(f, tables[1]) == bench.kernel_of_variant(word, nt), (n_taps, word, nt)
            assert (f["fmt"], f["nt"], f["wpw"]) == (CI8, nt, 1)
            checked.add(word)
    # every family of words was there to be checked
    assert {CHIP + 24 + 256 * 12, CHIP + 19 + 256 * 9, CHIP + 24 + KI, CHIP + 15 + KI, CHIP + 16, CHIP + 24, CHIP + 17, CHIP, 16, 8, 0,
            8 + C2, 8 + 2 * C2, 3 * C2} <= checked
    for km in range(16, 26):
        assert {CHIP + km + 256 * (km // 2), CHIP + km + KI} <= checked


def test_four_waves_per_workgroup_collapse(forms, tables):
    """A KS form, and a KI form of a block length other than 24, run <kChipMax, 0, 4>; 24 / 25 samples per chip run <kChipMax, 24, 4>,
    with taps whole chips apart the four-wave KI form of its own."""
    want = {(3, CHIP + 24 + 256 * 12): "epl_kernel<0,3,26,24,4,0,0,0>",
            (3, CHIP + 24 + KI): "epl_kernel<0,3,26,24,4,0,1,0>",
            (5, CHIP + 24 + KI): "epl_kernel<0,5,26,24,4,0,1,0>",
            (3, CHIP + 24): "epl_kernel<0,3,26,24,4,0,0,0>",
            (8, CHIP + 24): "epl_kernel<0,5,26,24,4,0,0,0> epl_kernel<0,3,26,24,4,0,0,0>",
            (3, CHIP + 19 + 256 * 9): "epl_kernel<0,3,26,0,4,0,0,0>",
            (3, CHIP + 25 + 256 * 12): "epl_kernel<0,3,26,0,4,0,0,0>",
            (3, CHIP + 20 + KI): "epl_kernel<0,3,26,0,4,0,0,0>",
            (5, CHIP + 20 + KI): "epl_kernel<0,5,26,0,4,0,0,0>",
            (3, CHIP + 15 + KI): "epl_kernel<0,3,26,0,4,0,0,0>",
            (3, CHIP + 17): "epl_kernel<0,3,26,0,4,0,0,0>",
            (3, CHIP + 16): "epl_kernel<0,3,26,0,4,0,0,0>",
            (2, CHIP): "epl_kernel<0,2,26,0,4,0,0,0>",
            (4, 16): "epl_kernel<0,3,16,0,4,0,0,0> epl_kernel<0,1,16,0,4,0,0,0>",
            (3, 8): "epl_kernel<0,3,8,0,4,0,0,0>",
            (1, 0): "epl_kernel<0,1,0,0,4,0,0,0>"}
    got = {}
    for fmt, n_taps, word, nt, wpw, has, f in forms:
        if fmt == CI8 and wpw == 4:
            if has:
                got.setdefault((n_taps, word), []).append(name_of(f, tables[1]))
            assert not f["row"] and f["ks"] == 0 and f["km"] in (0, 24) and f["km2"] == 0 and f["wpw"] == 4
            assert f["ki"] == (1 if has and word & KI and (word & 255) == CHIP + 24 and nt in (3, 5) else 0)
            assert f["km"] == (24 if (word & 255) == CHIP + 24 else 0)
    for key, names in want.items():
        assert " ".join(got[key]) == names, key


def test_a_plan_without_setups_runs_the_run_time_position_kernel(forms, tables):
    want = {(3, CHIP + 24 + 256 * 12): "epl_kernel<0,3,26,24,1,0,0,0>",
            (3, CHIP + 24 + KI): "epl_kernel<0,3,26,24,1,0,0,0>",
            (5, CHIP + 24 + KI): "epl_kernel<0,5,26,24,1,0,0,0>",
            (3, CHIP + 19 + 256 * 9): "epl_kernel<0,3,26,19,1,0,0,0>",       # (the block length alone stays compiled in)
            (3, CHIP + 20 + KI): "epl_kernel<0,3,26,20,1,0,0,0>",
            (5, CHIP + 20 + KI): "epl_kernel<0,5,26,0,1,0,0,0>",
            (3, CHIP + 16 + 256 * 8): "epl_kernel<0,3,26,15,1,0,0,16>",      # (16.x samples per chip: the 15 / 16 form serves them)
            (3, CHIP + 15 + KI): "epl_kernel<0,3,26,0,1,0,0,0>",
            (3, 8 + C2): "epl_kernel<0,3,8,0,1,0,0,0>",
            (3, 3 * C2): "epl_kernel<0,3,0,0,1,0,0,0>"}
    got = {}
    for fmt, n_taps, word, nt, wpw, has, f in forms:
        if fmt == CI8 and wpw == 1 and not has:
            got.setdefault((n_taps, word), []).append(name_of(f, tables[1]))
            assert f["ks"] == 0 and f["ki"] == 0 and f["shape"] == 0 and not f["setups"]
    for key, names in want.items():
        assert " ".join(got[key]) == names, key


def test_needs_setups_exactly_for_the_compile_time_tap_geometries_and_the_shapes(forms):
    said = 0
    for fmt, n_taps, word, nt, wpw, has, f in forms:
        want = fmt == CI8 and has and ((word & (KS_MASK | KI) and n_taps in (3, 5)) or (word // C2) & 3)
        assert f["setups"] == (1 if want else 0), (fmt, n_taps, word, nt, wpw, has)
        said += f["setups"]
        if fmt != CI8:
            assert f["w"] in (0, 8, 16) and not f["row"] and (f["km"], f["ks"], f["ki"], f["km2"], f["shape"]) == (0, 0, 0, 0, 0)
    assert said


def test_every_row_of_the_tables_is_reached_and_nothing_else_is_asked_for(forms, tables):
    rows, shapes = tables
    asked = {(f["nt"], f["km"], f["ks"], f["ki"]) for *_, f in forms if f["row"]}
    assert asked == set(rows), sorted(asked ^ set(rows))
    assert {f["shape"] for *_, f in forms if f["shape"]} == set(shapes) == {1, 2, 3}
    # what is no row is one of the general forms: a width alone, 24 / 25 samples per chip, or 15.x / 16.x
    for *_, f in forms:
        if not f["row"] and not f["shape"]:
            assert (f["ks"], f["km"], f["km2"]) in ((0, 0, 0), (0, 24, 0), (0, 15, 16)), f
            assert f["ki"] == 0 or (f["km"], f["wpw"]) == (24, 4), f
