"""Secondary-code phase and fine frequency (sdr_acq_secondary), the CPU side: the entry point in the ABI and its struct
layouts against the C compiler, the argument checks through the stand-alone request-check program, and the NumPy statement
alone on the inputs the GPU tests use (tests/test_gpu_secondary.py) -- the proof that those inputs are fair.

What the statement gives on the 18 cases (printed by test_model_recovers_phase_and_frequency; expectations, not asserts):
margin (max - second) / max: A 0.023-0.123, B 0.0023-0.0064, D 0.017-0.077, E 0.0009-0.0099, C 0.81, C' 0.21; best over
second-best hypothesis 2.5-5.2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import host_check
import refine_cases as rc
import secondary_cases as sc
from conftest import REPO
from sydr_amd import _lib
from sydr_amd.dsp.signalsearch import NH10, NH20
from test_abi import declared_symbols

MARGIN = 1e-6                  # the project's: the model's maximum must exceed every other entry of P by more than this times itself


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_secondary_symbol_is_declared_bound_and_exported():
    lib = _lib.load()
    assert "sdr_acq_secondary" in declared_symbols() and "sdr_acq_secondary" in _lib.exported_symbols()
    assert hasattr(lib, "sdr_acq_secondary")


def test_secondary_struct_layouts_agree_with_the_c_compiler(tmp_path):
    for ct, dt in ((_lib.SecItem, _lib.SEC_ITEM_DTYPE), (_lib.SecResult, _lib.SEC_RESULT_DTYPE)):
        assert C.sizeof(ct) == dt.itemsize
        assert [n for n, _ in ct._fields_] == list(dt.names)
        for name, (_, off) in dt.fields.items():
            assert getattr(ct, name).offset == off
    fields = [("sdr_sec_item", n) for n in _lib.SEC_ITEM_DTYPE.names] + [("sdr_sec_result", n) for n in _lib.SEC_RESULT_DTYPE.names]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %d %d'
                   + " %zu" * len(fields) + '\\n",sizeof(sdr_sec_item),sizeof(sdr_sec_result),SDR_SEC_PILOT,SDR_SEC_DATA,'
                   + ",".join(f"offsetof({s},{n})" for s, n in fields) + ");return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[:4] == [32, 48, _lib.SEC_PILOT, _lib.SEC_DATA] and C.sizeof(_lib.SecItem) == 32 and C.sizeof(_lib.SecResult) == 48
    assert got[4:] == [_lib.SEC_ITEM_DTYPE.fields[n][1] for n in _lib.SEC_ITEM_DTYPE.names] + \
        [_lib.SEC_RESULT_DTYPE.fields[n][1] for n in _lib.SEC_RESULT_DTYPE.names]


def test_make_secondary_items_packs_records():
    from sydr_amd.engine import make_secondary_items
    it = make_secondary_items([0, 1], [1, 0], [100, 2 ** 40], 1750.0, 1.023e6)
    assert it.dtype == _lib.SEC_ITEM_DTYPE and it["code_slot"].tolist() == [0, 1] and it["sec_row"].tolist() == [1, 0]
    assert it["start_sample"].tolist() == [100, 2 ** 40] and it["carrier_hz"].tolist() == [1750.0] * 2 and it["code_hz"].tolist() == [1.023e6] * 2


def test_neuman_hofman_codes():
    assert "".join("0" if c > 0 else "1" for c in NH10) == "0000110101"
    assert "".join("0" if c > 0 else "1" for c in NH20) == "00000100110101001110"
    assert NH10.dtype == np.int8 and set(NH20.tolist()) == {1, -1}


# ------------------------------------------------------------------------------------------------ 2. the argument checks
@host_check.requires_hipcc
def test_request_check_single_faults():
    exe = host_check.build("secondary_request_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) >= 70


# ------------------------------------------------------------------------------------------------ 3. the model alone
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_model_recovers_phase_and_frequency(name):
    c = sc.case(name)
    fine, h, k, P, z, x = sc.model(name)
    print(f"{name}: dop={c['doppler']} coarse={c['f0']} fine={fine} phase={h} true={c['true_phase']} "
          f"ratio={sc.hypothesis_ratio(P):.2f} margin={sc.margin(P):.3e}")
    assert P.shape == (len(c["sec"]), 51) and z.shape == (c["M"], c["S"])
    assert sc.margin(P) > MARGIN
    assert h == c["true_phase"]
    assert abs(fine - c["doppler"]) <= sc.STEP / 2
    assert sc.hypothesis_ratio(P) > 2.0
    if c["mode"] == 0:
        assert abs(abs(x) ** 2 - P[h, k]) <= 1e-12 * P[h, k]
    if name == "C":
        assert h == 5 and fine == 1630.0          # what the end-to-end GPU test asks for


def test_model_data_mode_with_one_group_is_the_pilot_mode():
    """Ls >= M and h = 0: all periods fall into one group, so mode 1 adds up one square -- mode 0's."""
    c = sc.case("E1")                              # NH20, M = 12
    z, tau = sc.segment_sums(c["rf"], c["s0"], c["code"], c["fs"], c["f0"], c["M"], c["S"])
    P0 = sc.search(z, tau, c["sec"], c["f0"], sc.SPAN, sc.STEP, 0)[3]
    P1 = sc.search(z, tau, c["sec"], c["f0"], sc.SPAN, sc.STEP, 1)[3]
    assert np.array_equal(P0[0], P1[0])
    assert not np.array_equal(P0[15], P1[15])      # (h = 15: the code wraps inside the window)
    zz, tt = z[:10], tau[:10]                      # M = Ls = 10 under NH10
    assert np.array_equal(sc.search(zz, tt, NH10, c["f0"], sc.SPAN, sc.STEP, 0)[3][0], sc.search(zz, tt, NH10, c["f0"], sc.SPAN, sc.STEP, 1)[3][0])


def test_model_all_ones_row_is_refines_no_edge_row():
    c = rc.acquired(4e6, *rc.SATELLITES[0])
    _, _, _, P_ref, z_ref = rc.refine_model(c["rf"], c["s0"], c["code"], 4e6, c["f0"], 10, 4, sc.SPAN, sc.STEP)
    _, _, _, P, z, _ = sc.secondary_model(c["rf"], c["s0"], c["code"], np.ones(7, np.int8), 4e6, c["f0"], 10, 4)
    assert np.array_equal(z, z_ref)
    assert P.shape == (7, 51) and np.array_equal(P[0], P_ref[0])
    assert all(np.array_equal(P[h], P[0]) for h in range(7))


@pytest.mark.parametrize("name", sc.EXTRA_NAMES)
def test_model_maximum_is_distinct_on_the_further_gpu_inputs(name):
    c, span, step = sc.extra(name)
    fine, h, k, P, _, _ = sc.extra_model(name)
    print(f"{name}: fine={fine} phase={h} true={c['true_phase']} k={k} of {P.shape[1]} margin={sc.margin(P):.3e}")
    if name == "M2":           # two hypotheses that are each other's negation: equal rows, the first maximum in row 0
        assert np.array_equal(P[0], P[1]) and h == 0 and sc.margin(P[:1]) > MARGIN
    else:
        assert sc.margin(P) > MARGIN
    if name.startswith("K401"):
        assert P.shape[1] == 401 and k == (0 if name == "K401first" else 400) and h == c["true_phase"]
    if name in ("M128", "L3h0", "L3h1", "L3h2"):
        assert h == c["true_phase"]
    assert {n: sc.extra(n)[0]["true_phase"] for n in ("L3h0", "L3h1", "L3h2")} == {"L3h0": 1, "L3h1": 2, "L3h2": 0}


def test_model_maximum_is_distinct_on_the_batch():
    _, rf, secs, items, M, S = sc.batch32()
    assert len(items) == 32 and {row for row, *_ in items} == {0, 1}
    for row, s0, f0, phase, dop in items:
        fine, h, _, P, _, _ = sc.secondary_model(rf, s0, sc.orc.gold_code(sc.PRN), secs[row], 4e6, f0, M, S)
        assert sc.margin(P) > MARGIN and h == phase and abs(fine - dop) <= sc.STEP / 2
