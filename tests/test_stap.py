"""CPU side of the space-time weights (sydr_amd/signal/stap.py, sdr_ddc_create_stap): the statement's identities against
`array.Statement` and against the layout's statement on a delayed stream, independence of the cut with the raw tail carried, the
lag covariance and the block-Toeplitz matrix made of it against direct sums on small integers, the two weight rules, the C
prototypes, the shared arithmetic run on the host (tests/csrc/ddc_stap_check.hip; also as a stand-alone sanitized binary), the
[RFSIGNAL] keys and the manager's training over a fake engine, and the table of the end-to-end recording the GPU test relies on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import array_cases as cases
import ddc_layout_cases as lcases
import host_check
import stap_cases as scases

from sydr_amd import _lib
from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import stap



# ---------------------------------------------------------------------------------------------- 1. identities of the statement
@pytest.mark.parametrize("name", list(cases.GEOMETRIES))
def test_one_tap_is_the_array_statement(name):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    w = cases.general_weights(K)
    for shape in cases.SHAPES:
        got = stap.statement(cases.config(shape, cases.FCWS["odd"], 0.37, layout, scases.geometry(lanes, 1, w.reshape(1, K), True)), [raw[:raw.size // 2], raw[raw.size // 2:]])
        want = ar.statement(cases.config(shape, cases.FCWS["odd"], 0.37, layout, ar.ArrayGeometry(lanes, w, True)), [raw])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.any(want != 0)
    st = stap.Statement(cases.config((1, 1), 0, 1.0, layout, scases.geometry(lanes, 1, None, True)))
    st.push(raw)
    R, n = ar.covariance(raw, layout, lanes)
    assert st.read_covariance()[1] == n and np.array_equal(st.read_covariance()[0][0], R)


@pytest.mark.parametrize("name", ["K3_int8_complex", "K3_int16_complex_swapped", "K8_int8_real"])
def test_one_nonzero_tap_is_the_layout_statement_on_the_delayed_stream(name):
    layout, lanes = cases.GEOMETRIES[name]
    raw, K = cases.stream(layout), len(lanes)
    for shape in cases.FILTERED:
        for T in (2, 8):
            for t0 in (0, T - 1):
                for a in (0, K - 1):
                    got = stap.statement(cases.config(shape, cases.FCWS["odd"], 0.37, layout, scases.geometry(lanes, T, stap.unit_weights(T, K, a, t0))), [raw])
                    want = dc.statement(cases.config(shape, cases.FCWS["odd"], 0.37, ar.element_layout(layout, lanes[a])), [scases.delayed(raw, layout, t0, cases.N_FRAMES)])
                    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.any(want != 0), (shape, T, t0, a)


def test_the_combine_rounds_every_product_and_every_sum_in_tap_then_element_order():
    rng = np.random.default_rng(scases.SEED + 1)
    T, K, n = 3, 2, 64
    sr, si = rng.integers(-3000, 3000, (K, n + T - 1)).astype(float), rng.integers(-3000, 3000, (K, n + T - 1)).astype(float)
    w = scases.general_weights(T, K)
    re, im = stap.combine(sr, si, w, T)
    for j in range(n):
        r = i = 0.0
        for t in range(T):
            for a in range(K):
                wr, wi, xr, xi = float(w[t, a].real), float(w[t, a].imag), sr[a, T - 1 + j - t], si[a, T - 1 + j - t]
                r = r + wr * xr
                r = r + wi * xi
                i = i + wr * xi
                i = i - wi * xr
        assert (r, i) == (re[j], im[j])
    exact = sum(np.conj(w[t, a]) * (sr[a, T - 1 - t:T - 1 - t + n] + 1j * si[a, T - 1 - t:T - 1 - t + n]) for t in range(T) for a in range(K))
    assert np.allclose(re + 1j * im, exact, rtol=0, atol=1e-9)


def test_geometry_limits():
    for T in (0, 9, -1):
        with pytest.raises(ValueError, match="taps"):
            stap.SpaceTimeGeometry((0, 1), T)
    with pytest.raises(ValueError, match="weights"):
        stap.SpaceTimeGeometry((0, 1), 3, np.ones(5))
    with pytest.raises(ValueError, match="finite"):
        stap.SpaceTimeGeometry((0, 1), 2, [[1, np.nan], [0, 0]])
    with pytest.raises(ValueError, match="elements"):
        stap.SpaceTimeGeometry((0,), 2)
    g = stap.SpaceTimeGeometry((3, 0), 4)
    assert g.weights.shape == (4, 2) and g.weights[0, 0] == 1 and np.count_nonzero(g.weights) == 1 and g.taps == 4 and isinstance(g, ar.ArrayGeometry)
    assert g == stap.SpaceTimeGeometry((3, 0), 4) and g != stap.SpaceTimeGeometry((3, 0), 5) and stap.default_reference_tap(8) == 3
    with pytest.raises(ValueError):
        stap.Statement(cases.config((1, 1), 0, 1.0, dc.InputLayout(dc.FIELD_INT8, 0, 4), ar.ArrayGeometry((3, 0))))


@pytest.mark.parametrize("shape", cases.FILTERED + [(1, 1)], ids=lcases.shape_id)
def test_the_statement_does_not_depend_on_the_cut_with_weights_changed_at_fixed_inputs(shape):
    layout, lanes = cases.GEOMETRIES["K3_int8_complex"]
    raw, T, K = cases.stream(layout), 8, 3
    marks = (1000, 1004)
    weights = [scases.general_weights(T, K, s) for s in range(3)]
    cfg = cases.config(shape, cases.FCWS["odd"], 0.37, layout, scases.geometry(lanes, T, weights[0], True))
    results = []
    for lengths in ([], [1, 1, 2, 3, 5, 900, 1, 4, 6, 2, 0, 40, 3]):
        st = stap.Statement(cfg)
        parts = []
        for first, count in cases.cut_with_marks(lengths, marks, cases.N_FRAMES):
            if first in marks and count > 0:
                st.set_weights(weights[1 + marks.index(first)])
            parts.append(st.push(cases.piece(raw, layout, first, count)))
        results.append((np.concatenate(parts), st.read_covariance()))
    assert np.array_equal(results[0][0].view(np.uint64), results[1][0].view(np.uint64))
    assert results[0][1][1] == results[1][1][1] == cases.N_FRAMES and np.array_equal(results[0][1][0], results[1][1][0])
    assert not np.array_equal(results[0][0], stap.statement(cfg, [raw]))


# ---------------------------------------------------------------------------------------------- 2. the covariance and the rules
def _stacked(sr, si, T):
    """y [n][T K] of the elements [K][n], frames before the first zero."""
    K, n = sr.shape
    s = np.concatenate([np.zeros((K, T - 1), dtype=np.complex128), sr + 1j * si], axis=1)
    return np.stack([np.concatenate([s[:, T - 1 + j - t] for t in range(T)]) for j in range(n)])


def test_space_time_covariance_against_direct_sums_on_small_integers():
    """The block-Toeplitz matrix made of the lags is Hermitian.  Against D = sum_j y_j y_j^H over ALL inputs j (frames before the
    first zero) entry ((t, a), (u, b)), u >= t, differs by exactly the t edge terms sum_{j = n - t}^{n - 1} s_a[j] conj(s_b[j - (u - t)]):
    the Toeplitz form counts every pair of frames the stream holds, the direct sum loses those whose later frame is among the last
    t.  Small integers: every sum is exact in a double."""
    rng = np.random.default_rng(scases.SEED + 2)
    T, K, n = 4, 3, 200
    sr, si = rng.integers(-9, 10, (K, n)).astype(float), rng.integers(-9, 10, (K, n)).astype(float)
    zeros = np.zeros((K, T - 1))
    C = stap.lag_covariance(np.concatenate([zeros, sr], axis=1), np.concatenate([zeros, si], axis=1), T, True)
    for tau in range(T):
        for a in range(K):
            for b in range(K):
                s_a, s_b = sr[a] + 1j * si[a], sr[b] + 1j * si[b]
                assert C[tau, a, b] == np.sum(s_a[tau:] * np.conj(s_b[:n - tau]))
    R = stap.space_time_covariance(C, 1)
    assert R.shape == (T * K, T * K) and np.array_equal(R, R.conj().T)
    assert np.array_equal(stap.space_time_covariance(C, 4), R / 4.0)
    y = _stacked(sr, si, T)
    D = np.einsum("ji,jk->ik", y, y.conj())
    s = sr + 1j * si
    edges = 0
    for t in range(T):
        for u in range(t, T):
            for a in range(K):
                for b in range(K):
                    edge = sum(s[a, j] * np.conj(s[b, j - (u - t)]) for j in range(n - t, n))
                    assert R[t * K + a, u * K + b] - D[t * K + a, u * K + b] == edge
                    edges += edge != 0
    assert edges > 50
    # ... and the sum over the inputs j >= T - 1 alone, whose stacked vectors hold no zero, lies between the two in the same way
    Dj = np.einsum("ji,jk->ik", y[T - 1:], y[T - 1:].conj())
    assert np.array_equal(Dj, Dj.conj().T) and np.max(np.abs(R - Dj)) <= (T - 1) * 2 * 81
    for bad in (np.zeros((9, 2, 2)), np.zeros((2, 2, 3)), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            stap.space_time_covariance(bad, 1)
    with pytest.raises(ValueError):
        stap.space_time_covariance(C, 0)


def test_float_lag_covariance_lies_within_its_bound_of_an_exact_sum():
    from fractions import Fraction
    rng = np.random.default_rng(scases.SEED + 3)
    T, K, n = 3, 2, 400
    sr, si = rng.uniform(-1, 1, (K, n + T - 1)).astype(np.float32).astype(float), rng.uniform(-1, 1, (K, n + T - 1)).astype(np.float32).astype(float)
    sr[:, :T - 1] = si[:, :T - 1] = 0.0
    C = stap.lag_covariance(sr, si, T, False)
    bound_re, bound_im = stap.lag_covariance_bound(sr, si, T)
    for tau in range(T):
        for a in range(K):
            for b in range(K):
                re = sum(Fraction(sr[a, T - 1 + j]) * Fraction(sr[b, T - 1 + j - tau]) + Fraction(si[a, T - 1 + j]) * Fraction(si[b, T - 1 + j - tau]) for j in range(n))
                im = sum(Fraction(si[a, T - 1 + j]) * Fraction(sr[b, T - 1 + j - tau]) - Fraction(sr[a, T - 1 + j]) * Fraction(si[b, T - 1 + j - tau]) for j in range(n))
                assert abs(Fraction(C[tau, a, b].real) - re) <= Fraction(bound_re[tau, a, b]) / 2 and abs(Fraction(C[tau, a, b].imag) - im) <= Fraction(bound_im[tau, a, b]) / 2


def test_the_weight_rules_against_a_direct_solve():
    rng = np.random.default_rng(scases.SEED + 4)
    T, K, n = 3, 2, 5000
    sr, si = rng.integers(-300, 300, (K, n + T - 1)).astype(float), rng.integers(-300, 300, (K, n + T - 1)).astype(float)
    C = stap.lag_covariance(sr, si, T, True)
    R = stap.space_time_covariance(C, n)
    Rl = R + 1e-3 * np.trace(R).real / (T * K) * np.eye(T * K)
    for reference, tap in ((0, None), (1, 0), (1, 2)):
        w = stap.power_inversion(C, n, reference, tap)
        e = np.zeros(T * K)
        e[(1 if tap is None else tap) * K + reference] = 1.0
        u = np.linalg.solve(Rl, e)
        assert w.shape == (T, K) and np.allclose(w.reshape(-1), u / np.vdot(e, u).real, rtol=1e-12, atol=0) and abs(w[1 if tap is None else tap, reference] - 1.0) < 1e-12
    steering = np.array([1.0, np.exp(0.7j)])
    w = stap.mvdr(C, n, steering, 2, 0.0)
    c = np.zeros((T, K), dtype=np.complex128)
    c[2] = steering
    assert abs(np.vdot(w.reshape(-1), c.reshape(-1)) - 1.0) < 1e-12
    u = np.linalg.solve(R, c.reshape(-1))
    assert np.allclose(w.reshape(-1), u / np.vdot(c.reshape(-1), u).real, rtol=1e-12, atol=0)
    # one tap: array.py's rules
    assert np.array_equal(stap.power_inversion(C[:1], n, 1).reshape(-1), ar.power_inversion(C[0], n, 1))
    assert np.array_equal(stap.mvdr(C[:1], n, steering).reshape(-1), ar.mvdr(C[0], n, steering))
    for kw in (dict(reference_tap=3), dict(reference_tap=-1), dict(loading=-1.0)):
        with pytest.raises(ValueError):
            stap.power_inversion(C, n, 0, **kw)


# ---------------------------------------------------------------------------------------------- 3. the C side without a device
def test_c_prototypes_and_host_side_refusals(tmp_path):
    proto = tmp_path / "proto.c"
    proto.write_text('#include "sydr_amd.h"\n'
                     "int (*const create)(sdr_engine*, const sdr_ddc_cfg*, int, const sdr_ddc_layout*, const sdr_ddc_array*, int, const double*, sdr_ddc**) = sdr_ddc_create_stap;\n"
                     "int (*const weights)(sdr_engine*, sdr_ddc*, const double*) = sdr_ddc_stap_weights;\n"
                     "int (*const cov)(sdr_engine*, sdr_ddc*, double*, int64_t*, int) = sdr_ddc_stap_covariance;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(REPO, "include"), "-c", str(proto),
                           "-o", str(tmp_path / "proto.o")])
    lib = _lib.load()
    assert lib.sdr_abi_version() == 5
    assert list(lib.sdr_ddc_create_stap.argtypes) == [C.c_void_p, C.POINTER(_lib.DdcCfg), C.c_int, C.POINTER(_lib.DdcLayout), C.POINTER(_lib.DdcArray),
                                                      C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_void_p)]
    assert lib.sdr_ddc_create_stap(None, None, 1, None, None, 3, None, None) != 0 and lib.sdr_ddc_stap_weights(None, None, None) != 0
    assert lib.sdr_ddc_stap_covariance(None, None, None, None, 0) != 0
    from sydr_amd.engine import stap_array_struct
    c = stap_array_struct(scases.geometry((5, 0, 2), 3, measure=True))
    assert (c.n_elements, c.flags, list(c.lanes)) == (3, 1, [5, 0, 2, 0, 0, 0, 0, 0])


@host_check.requires_hipcc
def test_stap_arithmetic_on_the_host():
    """sydr_amd/csrc/ddc_stap.h, the combine and the raw tail the converter's kernels and its host side share, compiled for the host
    alone (tests/csrc/ddc_stap_check.hip): as it is, with contraction allowed to the compiler, which the header must withstand,
    and as a stand-alone binary under the address and undefined-behaviour sanitizers."""
    for flags in (("-O1",), ("-O3", "-ffp-contract=fast"),
                  ("-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")):
        exe = host_check.build("ddc_stap_check", flags)
        out = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
        assert int(out.stdout.split()[1]) > 50000


# ---------------------------------------------------------------------------------------------- 4. the two-jammer recording
def test_the_oracle_needs_the_time_taps_on_the_two_jammer_recording():
    """stap_cases.two_jammers: two 0.5 MHz jammers from different directions, each 20 dB above the noise of an element, on two
    elements.  The oracle's PCPS and two_peak_compare on the fourth millisecond of the statement's ci16 ring, weights by power
    inversion of the statement's lag covariance of the first 2 ms (loading 1e-3, the reference element at the centre tap):

        stream                       peak [bin, sample]   ratio   output power over element 0
        element 0 alone              [36,  743] (wrong)   1.33      0.0 dB
        T = 1 (spatial)              [36,  743] (wrong)   1.23     -0.1 dB
        T = 3, centre tap 1          [13, 2828]           3.91    -20.8 dB
        T = 5, centre tap 2          [13, 2829]           3.76    -20.9 dB
        T = 7, centre tap 3          [13, 2830]           3.34    -21.2 dB

    The satellite is at bin 13 (1750 Hz), sample 2826 plus the centre tap.  Asserted: element 0 and T = 1 miss it or fall under the
    plugin's 1.5; T = 5 finds bin 13 within a sample of 2826 + 2 with a ratio above 1.5.  The power column is printed, not asserted."""
    from oracle import sydr_oracle as orc
    raw = scases.two_jammers()
    true_sample = round((orc.CODE_CHIPS - scases.E2E_SAT["code_phase"]) * scases.E2E_FS / orc.CODE_RATE)
    assert true_sample == 2826
    sr, si = ar.elements(raw, scases.E2E_LAYOUT, scases.E2E_LANES)
    p0 = np.mean(sr[0] ** 2 + si[0] ** 2)
    found = {}
    ring = stap.statement(scases.e2e_config(1), [raw], dc.FMT_CI16)                      # unit weight on element 0
    found[0] = scases.e2e_search(orc.iq_to_complex(ring.astype(np.float64)))
    print(f"element 0: peak {found[0][0]}, ratio {found[0][1]:.3f}")
    for T in (1, 3, 5, 7):
        C, n = scases.e2e_training(T)
        assert n == scases.E2E_TRAIN_MS * 4000
        cfg = scases.e2e_config(T, stap.power_inversion(C, n))
        found[T] = scases.e2e_search(orc.iq_to_complex(stap.statement(cfg, [raw], dc.FMT_CI16).astype(np.float64)))
        re, im = stap.Statement(cfg).combined(raw)
        print(f"T = {T}: peak {found[T][0]}, ratio {found[T][1]:.3f}, output power {10 * np.log10(np.mean(re ** 2 + im ** 2) / p0):.1f} dB over element 0")
    for k in (0, 1):
        assert found[k][1] < 1.5 or found[k][0] != [13, true_sample], found
    assert found[0][0] == [36, 743] and abs(found[0][1] - 1.333) < 0.001 and found[1][0] == [36, 743] and abs(found[1][1] - 1.234) < 0.001, found
    peak, ratio = found[5]
    assert peak[0] == 13 and abs(peak[1] - (true_sample + 2)) <= 1 and ratio > 1.5, found
    assert peak == [13, 2829] and abs(ratio - 3.756) < 0.001, found
    assert found[3][0] == [13, 2828] and found[7][0] == [13, 2830] and found[3][1] > 3.0 and found[7][1] > 3.0, found


# ---------------------------------------------------------------------------------------------- 5. the [RFSIGNAL] keys and the manager
_conf = scases.e2e_conf


def test_ini_keys_parse_and_are_refused(tmp_path):
    from sydr_amd.signal.iqsource import RFSignal
    path = tmp_path / "stap.bin"
    scases.two_jammers(1).tofile(path)
    sig = RFSignal(_conf(path))                                                            # without array_taps: as it was
    assert type(sig.frontEnd.config.array) is ar.ArrayGeometry and (sig.frontEnd.array.taps, sig.frontEnd.array.delay) == (1, 0)
    sig = RFSignal(_conf(path, array_taps=1, array_mode="power_inversion"))
    assert type(sig.frontEnd.config.array) is ar.ArrayGeometry and sig.frontEnd.config.array.measure and sig.frontEnd.array.delay == 0
    sig = RFSignal(_conf(path, array_taps=5, array_reference=1))
    cfg, plan = sig.frontEnd.config, sig.frontEnd.array
    assert isinstance(cfg.array, stap.SpaceTimeGeometry) and cfg.array.taps == 5 and not cfg.array.measure and cfg.layout == scases.E2E_LAYOUT
    assert np.array_equal(cfg.array.weights, stap.unit_weights(5, 2, 1, 2)) and (plan.taps, plan.reference_tap, plan.delay, plan.adaptive) == (5, 2, 2, False)
    sig = RFSignal(_conf(path, array_taps=2, array_weights="1,0, 0,1, -1,0, 0.5,-0.25", array_reference_tap=0))
    assert np.array_equal(sig.frontEnd.config.array.weights, [[1, 1j], [-1, 0.5 - 0.25j]]) and sig.frontEnd.array.delay == 0
    sig = RFSignal(_conf(path, array_taps=8, array_mode="power_inversion", array_reference_tap=6, array_loading=0.01, array_train_ms=1))
    cfg, plan = sig.frontEnd.config, sig.frontEnd.array
    assert cfg.array.measure and np.array_equal(cfg.array.weights, stap.unit_weights(8, 2, 0, 6))
    assert (plan.mode, plan.reference, plan.reference_tap, plan.loading, plan.train_ms, plan.adaptive, plan.delay) == ("power_inversion", 0, 6, 0.01, 1, True, 6)
    C_, n = scases.e2e_training(3)
    sig = RFSignal(_conf(path, array_taps=3, array_mode="mvdr", array_steering="1,0, 0,1"))
    assert np.array_equal(sig.frontEnd.array.solve(C_, n), stap.mvdr(C_, n, [1, 1j], 1))
    sig = RFSignal(_conf(path, array_taps=3, array_mode="power_inversion", array_reference=1))
    assert np.array_equal(sig.frontEnd.array.solve(C_, n), stap.power_inversion(C_, n, 1, 1))
    for bad, match in ((dict(array_taps=0), "array_taps"), (dict(array_taps=9), "array_taps"), (dict(array_taps=3, array_reference_tap=3), "array_reference_tap"),
                       (dict(array_reference_tap=1), "array_reference_tap"), (dict(array_lanes=None, array_taps=2), "array_lanes"),
                       (dict(array_lanes=None, array_reference_tap=0), "array_lanes"), (dict(array_taps=2, array_weights="1,0,0,0"), "pairs"),
                       (dict(array_taps=2, array_weights="1,0, 0,0, nan,0, 0,0"), "finite"), (dict(array_taps=2, blanking_factor=5.0), "mitigator"),
                       (dict(array_taps=2, array_mode="power_inversion", array_weights="1,0,0,0,0,0,0,0"), "belong")):
        with pytest.raises(ValueError, match=match):
            RFSignal(_conf(path, **bad))


def test_the_manager_trains_solves_resets_and_restarts(tmp_path):
    """array_taps = 5 with power inversion through ChannelManager over a fake engine whose converter is the statement: train_ms
    pushes with unit weight on (reference, reference tap), one clearing read of the lag covariance, the solved [T][K] weights set,
    one reset -- and then the recording from its first sample: the ring equals the statement's with that one weight matrix,
    whatever the block length."""
    from fake_engine import OracleEngine
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.signal.iqsource import RFSignal

    class StapOracleEngine(OracleEngine):
        def __init__(self):
            super().__init__()
            self.log = []

        def ddc_create(self, cfg):
            self.log.append("create")
            return stap.Statement(cfg)

        def ddc_push(self, ddc, raw, ring_offset=0):
            self.log.append(("push", ddc.n_seen, int(ring_offset), ddc.weights.tobytes()))
            v = ddc.push(raw)
            self.iq_upload(dc.quantise(v, self.iq_fmt), ring_offset)
            return v.size

        ddc_push_queue = ddc_push

        def ddc_stap_covariance(self, ddc, clear=False):
            self.log.append(("covariance", bool(clear)))
            return ddc.read_covariance(clear)

        def ddc_stap_weights(self, ddc, w):
            self.log.append("weights")
            ddc.set_weights(w)

        def ddc_reset(self, ddc):
            self.log.append("reset")
            ddc.reset()

        def ddc_destroy(self, ddc):
            pass

        def sync(self):
            pass

    T, ms = scases.E2E_TAPS, scases.E2E_MS
    raw = scases.two_jammers()
    path = tmp_path / "stap.bin"
    raw.tofile(path)
    per_ms = int(scases.E2E_FS * 1e-3)
    C_, n = scases.e2e_training(T)
    w = stap.power_inversion(C_, n)
    want = stap.statement(scases.e2e_config(T, w), [raw], dc.FMT_CI16)
    for block in (1, 4):
        sig = RFSignal(_conf(path, array_mode="power_inversion", array_train_ms=scases.E2E_TRAIN_MS, array_taps=T))
        eng = StapOracleEngine()
        mgr = ChannelManager(sig, engine=eng)
        e0 = stap.unit_weights(T, 2, 0, 2).tobytes()
        assert eng.log == ["create", ("push", 0, 0, e0), ("push", per_ms, 0, e0), ("covariance", True), "weights", "reset"]
        assert np.array_equal(mgr.arrayWeights, w) and mgr.arrayWeights.shape == (T, 2) and mgr.arrayDelay == 2 and sig.position == 0
        for _ in range(ms // block):
            mgr.addNewRFData(sig.getMilliseconds(block))
        pushes = [entry for entry in eng.log[6:] if entry[0] == "push"]
        assert [p[1] for p in pushes] == list(range(0, ms * per_ms, block * per_ms)) and all(p[3] == w.tobytes() for p in pushes)
        got_C, got_n = mgr.arrayCovariance()
        st = stap.Statement(scases.e2e_config(T, w, True))
        st.push(raw)
        assert got_n == ms * per_ms and np.array_equal(got_C, st.read_covariance()[0])
        assert np.array_equal(eng.ring[:2 * ms * per_ms], want) and np.any(want != 0)
        mgr.close()
