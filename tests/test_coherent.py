"""The coherent search under secondary-code hypotheses (sdr_pcps_coherent), the CPU side: the entry point in the ABI and its
struct layouts against the C compiler, the argument checks through the stand-alone request-check program, and the NumPy
statement alone on the inputs the GPU tests use (tests/test_gpu_coherent.py) -- the proof that those inputs are fair, and that
the statement finds with a ratio of 1.5 and more what the padded non-coherent search leaves below 1.5.

What the statement gives (printed by the tests; expectations, not asserts): margin of the map 8.8e-5 (lagN1) .. 0.91, of the
peak cell's table 4.9e-3 .. 0.95; weak_pilot (NH20, M = 40, amp 0.5, seed 4) ratio 1.72 against the padded search's 1.19,
weak_data (NH10, data mode, M = 40, amp 0.6, seed 2) 1.98 against 1.40.

The fine grid has K = 2*floor(span/step) + 1 frequencies, an odd number: the largest grid the call takes is K = 63, which the
cases k63first / k63last use where the issue spoke of K = 64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coherent_cases as cc
import host_check
from conftest import REPO
from sydr_amd import _lib
from sydr_amd.dsp.signalsearch import fine_grid
from test_abi import declared_symbols

MARGIN = 1e-6                  # the project's: a maximum must exceed every other entry by more than this times itself


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_coherent_symbol_is_declared_bound_and_exported():
    lib = _lib.load()
    assert "sdr_pcps_coherent" in declared_symbols() and "sdr_pcps_coherent" in _lib.exported_symbols()
    assert hasattr(lib, "sdr_pcps_coherent")
    assert lib.sdr_abi_version() == 5 == _lib.ABI_VERSION
    assert len(declared_symbols()) == 101


def test_coherent_struct_layouts_agree_with_the_c_compiler(tmp_path):
    for ct, dt in ((_lib.CohCfg, _lib.COH_CFG_DTYPE), (_lib.CohResult, _lib.COH_RESULT_DTYPE)):
        assert C.sizeof(ct) == dt.itemsize
        assert [n for n, _ in ct._fields_] == list(dt.names)
        for name, (_, off, *_rest) in dt.fields.items():
            assert getattr(ct, name).offset == off
    fields = [("sdr_coh_cfg", n) for n in _lib.COH_CFG_DTYPE.names] + [("sdr_coh_result", n) for n in _lib.COH_RESULT_DTYPE.names]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu'
                   + " %zu" * len(fields) + '\\n",sizeof(sdr_coh_cfg),sizeof(sdr_coh_result),'
                   + ",".join(f"offsetof({s},{n})" for s, n in fields) + ");return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[:2] == [48, 80] and C.sizeof(_lib.CohCfg) == 48 and C.sizeof(_lib.CohResult) == 80
    assert got[2:] == [_lib.COH_CFG_DTYPE.fields[n][1] for n in _lib.COH_CFG_DTYPE.names] + \
        [_lib.COH_RESULT_DTYPE.fields[n][1] for n in _lib.COH_RESULT_DTYPE.names]


# ------------------------------------------------------------------------------------------------ 2. the argument checks
@host_check.requires_hipcc
def test_request_check_single_faults_limits_and_cuts():
    exe = host_check.build("coherent_request_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
    assert int(out.stdout.split()[1]) >= 90


# ------------------------------------------------------------------------------------------------ 3. the statement alone
def test_fine_grid_is_acq_refines():
    assert fine_grid(125.0, 25.0).tolist() == [-125.0 + 25.0 * k for k in range(11)]
    assert fine_grid(10.0, 25.0).tolist() == [0.0] and len(fine_grid(155.0, 5.0)) == 63
    lib = _lib.load()
    for span, step in ((125.0, 25.0), (10.0, 25.0), (155.0, 5.0), (160.0, 5.0)):
        assert lib.sdr_acq_refine_bins(span, step) == len(fine_grid(span, step))


@pytest.mark.parametrize("name", cc.PARITY_NAMES + cc.WEAK_NAMES + ["strong"])
def test_statement_has_a_distinct_answer_and_recovers_what_was_planted(name):
    c = cc.case(name)
    res, R, P = cc.model(name)
    r = res[0]
    m_map = cc.map_margin(R[0], int(r["peak_bin"]), int(r["peak_code"]), cc.excl_of(c))
    m_tab = cc.table_margin(P[0], name in cc.TIES)
    print(f"{name}: bin {r['peak_bin']} code {r['peak_code']} (planted {c['true_code']}) phase {r['sec_phase']} (planted "
          f"{c['true_phase']}) carrier {r['carrier_hz']} (Doppler {c['doppler']}) ratio {r['peak_ratio']:.3f} "
          f"margins {m_map:.2e} {m_tab:.2e} power ratio {r['power'] / r['power_other']:.2f}")
    K = len(fine_grid(c["span"], c["fine"]))
    assert R.shape == (1, len(np.arange(-c["range"], c["range"] + 1, c["step"])), c["N"]) and P.shape == (1, len(c["secs"][0]), K)
    assert m_map >= MARGIN and m_tab >= MARGIN
    assert abs(int(r["peak_code"]) - c["true_code"]) <= 1
    assert int(r["sec_phase"]) == c["true_phase"]
    assert abs(r["carrier_hz"] - c["doppler"]) <= c["fine"] / 2
    assert cc.coarse_ok(c, r["peak_bin"])
    assert r["peak"] == R[0, r["peak_bin"], r["peak_code"]] and r["power"] == P[0, r["sec_phase"], r["fine_idx"]]
    assert abs(r["peak"] ** 2 - r["power"]) <= 1e-9 * r["power"]
    if c["mode"] == 0:
        assert abs(r["prompt_re"] ** 2 + r["prompt_im"] ** 2 - r["power"]) <= 1e-12 * r["power"]
    else:
        assert r["prompt_re"] == 0.0 and r["prompt_im"] == 0.0
    if name == "m2":               # two hypotheses that are each other's negation: equal rows, the first maximum in row 0
        assert np.array_equal(P[0, 0], P[0, 1]) and r["sec_phase"] == 0 and r["power_other"] == r["power"]
    if name == "k63first":
        assert K == 63 and r["fine_idx"] == 0
    if name == "k63last":
        assert K == 63 and r["fine_idx"] == 62
    if name == "k1":
        assert K == 1 and r["fine_idx"] == 0 and r["carrier_hz"] == 1625.0
    if name == "data":             # partial groups at both ends
        assert c["true_phase"] % 10 != 0 and (c["true_phase"] + c["M"]) % 10 != 0
    assert {n: cc.case(n)["true_phase"] for n in ("l3h0", "l3h1", "l3h2")} == {"l3h0": 1, "l3h1": 2, "l3h2": 0}


@pytest.mark.parametrize("name", cc.WEAK_NAMES)
def test_statement_finds_what_the_padded_search_leaves_below_threshold(name):
    """The reason for the feature: peak_ratio >= 1.5 on the truth where pcps_signal_statement(pad=1, noncoh=M) stays below."""
    c = cc.case(name)
    r = cc.model(name)[0][0]
    pb, pc, pr = cc.padded(name)
    print(f"{name}: coherent ratio {r['peak_ratio']:.3f} at code {r['peak_code']}, phase {r['sec_phase']}, {r['carrier_hz']} Hz; "
          f"padded non-coherent ratio {pr:.3f} at code {pc}")
    assert r["peak_ratio"] >= 1.5 > pr
    assert abs(int(r["peak_code"]) - c["true_code"]) <= 1 and r["sec_phase"] == c["true_phase"]
    assert abs(r["carrier_hz"] - c["doppler"]) <= c["fine"] / 2


def test_statement_data_mode_with_one_group_is_the_pilot_mode():
    """Ls >= M and h = 0: all periods fall into one group, so data mode adds up one square -- the pilot mode's."""
    from sydr_amd.dsp.signalsearch import coherent_cell
    rng = np.random.default_rng(5)
    col = rng.standard_normal(7) + 1j * rng.standard_normal(7)
    freqs = [1500.0 + d for d in fine_grid(50.0, 25.0)]
    p0, x0 = coherent_cell(col, cc.NH20, freqs, 4000, 4e6, 0)
    p1, x1 = coherent_cell(col, cc.NH20, freqs, 4000, 4e6, 1)
    assert np.array_equal(p0[0], p1[0]) and not np.array_equal(p0[15], p1[15]) and not x1.any()
    assert np.allclose(np.abs(x0) ** 2, p0, rtol=1e-12, atol=0.0)
