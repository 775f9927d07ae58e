"""CPU side of sdr_corr_profile (the correlation function on a dense tap grid): the model the GPU tests hold the device to
is the existing NumPy statement, the inputs are fair, and the run walk the kernel's lanes execute (sydr_amd/csrc/corr_bounds.h,
compiled for the host alone) is the run-length encoding of NumPy's chip indices, exactly."""
import itertools
import subprocess

import numpy as np

import corr_cases as cc
import host_check
from conftest import load_golden
from oracle import sydr_oracle as orc


# ------------------------------------------------------------------------------------- 1. the model is the statement
def test_model_is_the_existing_statement_on_the_golden_cases():
    """The grid (-0.5, 0.5, 3) is E, P, L: bit for bit what orc.epl((-0.5, 0, 0.5)) gives on the g5 cases."""
    g = load_golden("g5_epl.npz")
    assert list(cc.grid(-0.5, 0.5, 3)) == [-0.5, 0.0, 0.5]
    checked = 0
    for tag in g["cases"]:
        prn, fs, f, rc, rk, step, n = g[f"{tag}_params"]
        rf = orc.iq_to_complex(g[f"{tag}_iq"])
        code = orc.gold_code(int(prn))
        ref = np.array(orc.epl(rf, orc.pad_code(code), fs, f, rc, rk, step, (-0.5, 0.0, 0.5)))
        got = cc.profile_model(rf, code, fs, (0, int(n), 0, f, rc, rk, step), -0.5, 0.5, 3)
        assert np.array_equal(got.reshape(-1), ref), tag
        checked += 1
    prn, fs, f, rc, rk, step = g["fixture_params"]
    rf = orc.iq_to_complex(g["fixture_iq"])
    got = cc.profile_model(rf, orc.gold_code(int(prn)), fs, (0, len(rf), 0, f, rc, rk, step), -0.5, 0.5, 3)
    assert np.array_equal(got.reshape(-1), g["fixture_out"])
    assert checked >= 3


# ------------------------------------------------------------------------------------- 2. the parity cases are fair
def test_one_wrong_chip_shows_far_above_the_cap_in_every_parity_case():
    """Every case of the GPU parity test, every item: the chip of ONE sample of ONE tap flipped moves that tap's sum by
    2 * |x_k| -- more than 1e-6 of the item's maximum, a thousand caps.  Checked on a concrete sample (flipped in the
    model's own sum) and, so that the sample is no lucky pick, on the median over the window."""
    cases = cc.parity_cases()
    seen = dict(rates=set(), taps=set(), fmts=set())
    for name, c in cases.items():
        ref = cc.case_model(c)
        assert np.isfinite(ref).all(), name
        peak = np.hypot(ref[..., 0], ref[..., 1]).max(axis=1)
        for i, it in enumerate(c["items"]):
            _, n, start, f, rc, rk, cstep = it
            x = c["rf"][(int(start) + np.arange(int(n))) % c["capacity"]]
            assert 2.0 * np.median(np.abs(x)) > 1e-6 * peak[i], (name, i)
            # one concrete flip: tap j, a sample in the middle of the epoch
            j, k = c["n_taps"] // 2, int(n) // 2
            while abs(x[k]) == 0:
                k += 1
            s = cc.grid(c["first"], c["step"], c["n_taps"])[j]
            idx = orc.epl_indices(int(n), rk, cstep, s)
            L = len(c["codes"][it[0]])
            chips = np.asarray(c["codes"][it[0]], dtype=np.float64)[(idx - 1) % L]
            w = np.exp(1j * (-(f * 2.0 * np.pi * (np.arange(0.0, int(n)) / c["fs"])) + rc)) * x
            clean = np.sum(chips * w)
            assert abs(clean - complex(*ref[i, j])) <= 1e-12 * peak[i], (name, i)      # (the same sum the model made)
            chips[k] = -chips[k]
            assert abs(np.sum(chips * w) - clean) > 1e-6 * peak[i], (name, i)
        seen["rates"].add(c["fs"]), seen["taps"].add(c["n_taps"]), seen["fmts"].add(c["fmt"])
    # and the set is the one the issue asks for
    assert seen["rates"] == set(cc.RATES)
    assert {1, 3, 65, 129, 1024} <= seen["taps"]
    assert seen["fmts"] == {0, 1, 2, 3}
    assert max(len(c["items"]) for c in cases.values()) == 32
    assert any(c["step"] == 0.0 for c in cases.values()) and any(c["step"] < 0.0 for c in cases.values())
    assert any(c["max_chips"] == 4092 for c in cases.values())
    assert any(abs(c["first"]) >= 40 and c["max_periods"] == 1 for c in cases.values())


# ------------------------------------------------------------------------------------- 3. the run walk against NumPy
LONG_CHIPS = 4092
DOPPLERS = (0.0, -5000.0, 4999.0, 1234.5)
SPACINGS = np.arange(-64, 65) / 16.0          # -4 .. +4 in steps of 1/16


def _rem_codes():
    rng = np.random.default_rng(20260008)
    return (0.0, 1e-12, 0.25, 0.9999999, -0.3) + tuple(rng.uniform(-1.0, 1.0, 3))


def _rle(idx):
    first = np.concatenate(([0], np.flatnonzero(np.diff(idx)) + 1))
    return first, idx[first]


@host_check.requires_hipcc
def test_run_walk_is_the_run_length_encoding_of_numpys_indices():
    """corr_bounds.h on the host: for every combination of rate, Doppler, rem_code and spacing, over a 4 ms epoch of a
    4092-chip code, the (first sample, padded index) pairs the walk produces are exactly the run-length encoding of
    orc.epl_indices -- no case excluded."""
    exe = host_check.build("corr_bounds_check")
    sets = runs = exact_phase = 0
    for fs, dop in itertools.product(cc.BOUNDS_RATES, DOPPLERS):
        cstep = orc.CODE_RATE * (1.0 + dop / 1575.42e6) / fs
        for rk in _rem_codes():
            n = int(np.ceil((LONG_CHIPS - rk) / cstep))
            lines = "".join(f"{n} {float(rk).hex()} {float(cstep).hex()} {float(s).hex()}\n" for s in SPACINGS)
            out = subprocess.run([str(exe)], input=lines.encode(), capture_output=True, check=True)
            assert out.stderr.decode().strip() == f"ok {len(SPACINGS)}", out.stderr.decode()
            got = np.frombuffer(out.stdout, dtype=np.int32)
            at = 0
            for s in SPACINGS:
                idx = orc.epl_indices(n, rk, cstep, s)
                first, value = _rle(idx)
                count = int(got[at])
                assert count == len(first), (fs, dop, rk, s, count, len(first))
                pairs = got[at + 1:at + 1 + 2 * count].reshape(count, 2)
                assert np.array_equal(pairs[:, 0], first) and np.array_equal(pairs[:, 1], value), (fs, dop, rk, s)
                at += 1 + 2 * count
                sets += 1
                runs += count
                # (how often the trap is set: samples whose phase is a whole number before the ceil)
                shift = rk + s
                y = np.linspace(shift, cstep * n + shift, n, endpoint=False)
                exact_phase += int(np.count_nonzero(y == np.floor(y)))
            assert at == len(got)
    assert sets == len(cc.BOUNDS_RATES) * len(DOPPLERS) * 8 * len(SPACINGS)
    assert exact_phase > 10000, exact_phase
    print(f"run walk: {sets} parameter sets, {runs} runs, {exact_phase} samples with a whole-number phase")
