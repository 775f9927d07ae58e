"""CPU side of the antenna arrays (sydr_amd/signal/array.py, sdr_ddc_create_array): the statement's combine against `decode` and
against exact integer sums, the covariance, the two weight rules against a direct solve, independence of the cut, the C struct
and the refusals that need no device, the shared arithmetic run on the host (tests/csrc/ddc_array_check.hip), and the property
of the end-to-end recording the GPU test relies on -- the oracle misses the satellite on one element and finds it on the
power-inversion combination."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import array_cases as cases
import ddc_layout_cases as lcases
import host_check

from sydr_amd import _lib
from sydr_amd.engine import array_struct
from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc

INVALID = -1


# ---------------------------------------------------------------------------------------------- 1. the combine
@pytest.mark.parametrize("name", list(cases.GEOMETRIES))
def test_a_unit_weight_is_decode_at_that_lane(name):
    layout, lanes = cases.GEOMETRIES[name]
    raw = cases.stream(layout)
    sr, si = ar.elements(raw, layout, lanes)
    for a, lane in enumerate(lanes):
        re, im = ar.combine(sr, si, ar.unit_weights(len(lanes), a))
        want_re, want_im = dc.decode(raw, ar.element_layout(layout, lane))
        assert np.array_equal(re, want_re) and np.array_equal(im, want_im)
        assert not np.any(np.signbit(re[re == 0])) and not np.any(np.signbit(im[im == 0]))       # (zeros are +0, as decode's)
        v = ar.statement(cases.config((33, 2), cases.FCWS["odd"], 1.0, layout, ar.ArrayGeometry(lanes, ar.unit_weights(len(lanes), a))), [raw])
        want = dc.statement(cases.config((33, 2), cases.FCWS["odd"], 1.0, ar.element_layout(layout, lane)), [raw])
        assert np.array_equal(v.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", cases.INT8_GEOMETRIES)
def test_quarter_turn_weights_give_the_exact_integer_sum(name):
    layout, lanes = cases.GEOMETRIES[name]
    raw = cases.stream(layout)
    sr, si = ar.elements(raw, layout, lanes)
    for turn in range(4):
        w = cases.quarter_weights(len(lanes), turn)
        re, im = ar.combine(sr, si, w)
        want = cases.combined_integers(raw, layout, lanes, w)
        assert np.array_equal(re, want[0::2]) and np.array_equal(im, want[1::2]) and np.any(want != 0)


def test_the_combine_rounds_every_product_and_every_sum():
    """One frame whose fused evaluation differs: the statement is the unfused one, operation for operation."""
    w = np.array([1.0, 1.0 + 2.0 ** -30])
    sr, si = np.array([[-1.0], [1.0 + 2.0 ** -30]]), np.zeros((2, 1))
    re, im = ar.combine(sr, si, w)
    assert re[0] == 2.0 ** -29 and im[0] == 0.0                       # (the exact sum is 2^-29 + 2^-60)


def test_geometry_limits():
    layout = dc.InputLayout(dc.FIELD_INT8, 0, 4, 0, True)
    for lanes in ((0,), (), tuple(range(9)), (0, 0), (-1, 0)):
        with pytest.raises(ValueError):
            ar.ArrayGeometry(lanes)
    for lanes in ((0, 3), (3, 0)):
        with pytest.raises(ValueError):
            dc.DownConverterConfig(dc.IN_R8, layout=layout, array=ar.ArrayGeometry(lanes))
    with pytest.raises(ValueError):
        dc.DownConverterConfig(dc.IN_R8, array=ar.ArrayGeometry((0, 2)))          # no layout
    for w in ([1.0], [1.0, float("nan")], [1.0, complex(0.0, float("inf"))], [[1.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            ar.ArrayGeometry((0, 2), w)
    g = ar.ArrayGeometry((2, 0), [[1.0, 2.0], [3.0, -4.0]], measure=True)
    assert np.array_equal(g.weights, [1 + 2j, 3 - 4j]) and g.flags == ar.ARRAY_MEASURE and g.n_elements == 2
    assert dc.DownConverterConfig(dc.IN_R8, layout=layout, array=g).array is g


# ---------------------------------------------------------------------------------------------- 2. the cut
@pytest.mark.parametrize("shape", cases.FILTERED, ids=lcases.shape_id)
def test_the_statement_does_not_depend_on_the_cut_with_weights_changed_at_fixed_inputs(shape):
    layout, lanes = cases.GEOMETRIES["K3_int8_complex"]
    raw = cases.stream(layout)
    K, n = len(lanes), cases.N_FRAMES
    w0, w1, w2 = (cases.general_weights(K, s) for s in range(3))
    marks = (1000, 1007)                                                 # the second change while the first is still in the history
    cfg = cases.config(shape, cases.FCWS["odd"], 1.0, layout, ar.ArrayGeometry(lanes, w0))
    Tp = lcases.phase_taps(shape)
    results = []
    for lengths in ([], [1, 1, 1, 2, 3, max(Tp - 2, 0), 0, Tp + 1, 997, 1, 5, 1, 1], [n]):
        st, parts = ar.Statement(cfg), []
        for first, count in cases.cut_with_marks(lengths, marks, n):
            if first in marks:
                st.set_weights(w1 if first == marks[0] else w2)
            parts.append(st.push(cases.piece(raw, layout, first, count)))
        results.append(np.concatenate(parts))
    assert np.array_equal(results[0].view(np.uint64), results[1].view(np.uint64)) and np.array_equal(results[0].view(np.uint64), results[2].view(np.uint64))
    # ... and it is not the stream of any one weight vector
    for w in (w0, w1, w2):
        assert not np.array_equal(results[0], ar.statement(cases.config(shape, cfg.fcw, 1.0, layout, ar.ArrayGeometry(lanes, w)), [raw]))


# ---------------------------------------------------------------------------------------------- 3. the covariance
@pytest.mark.parametrize("name", list(cases.GEOMETRIES))
def test_covariance_of_integer_fields_is_the_exact_sum(name):
    layout, lanes = cases.GEOMETRIES[name]
    raw = cases.stream(layout, 1000)
    R, n = ar.covariance(raw, layout, lanes)
    sr, si = ar.elements(raw, layout, lanes)
    s = [[complex(int(a), int(b)) for a, b in zip(r, i)] for r, i in zip(sr, si)]        # Python integers inside: no rounding anywhere
    assert n == 1000
    for a in range(len(lanes)):
        for b in range(len(lanes)):
            re = sum(int(x.real) * int(y.real) + int(x.imag) * int(y.imag) for x, y in zip(s[a], s[b]))
            im = sum(int(x.imag) * int(y.real) - int(x.real) * int(y.imag) for x, y in zip(s[a], s[b]))
            assert R[a, b] == complex(re, im)
    assert np.array_equal(R, R.conj().T) and np.all(R.diagonal().imag == 0)
    st = ar.Statement(cases.config((1, 1), 0, 1.0, layout, ar.ArrayGeometry(lanes, measure=True)))
    st.push(cases.piece(raw, layout, 0, 400))
    st.push(cases.piece(raw, layout, 400, 600))
    got, got_n = st.read_covariance(clear=True)
    assert np.array_equal(got, R) and got_n == 1000 and st.read_covariance() == (pytest.approx(np.zeros_like(R)), 0)


def test_float_covariance_lies_within_its_bound_of_an_exact_sum():
    layout, lanes = dc.InputLayout(dc.FIELD_FLOAT32, 0, 6, 0, True), (4, 0, 2)
    raw = np.random.default_rng(cases.SEED + 5).uniform(-1.0, 1.0, 6 * 1000).astype(np.float32)
    R, n = ar.covariance(raw, layout, lanes)
    sr, si = ar.elements(raw, layout, lanes)
    import math
    bound_re, bound_im = ar.covariance_bound(raw, layout, lanes)
    for a in range(3):
        for b in range(3):
            re = math.fsum(sr[a] * sr[b]) + math.fsum(si[a] * si[b])
            im = math.fsum(si[a] * sr[b]) - math.fsum(sr[a] * si[b])
            assert abs(R[a, b].real - re) <= bound_re[a, b] and abs(R[a, b].imag - im) <= bound_im[a, b]
    assert np.all(bound_re < 1e-9) and np.all(bound_re > 0)


# ---------------------------------------------------------------------------------------------- 4. the weight rules
def _synthetic_R(K=4, jam=1.0e4, noise=1.0, seed=3):
    rng = np.random.default_rng(cases.SEED + seed)
    a_jam = np.exp(2j * np.pi * rng.uniform(0, 1, K))
    n = 4000
    return n * (jam * np.outer(a_jam, a_jam.conj()) + noise * np.eye(K)), n, a_jam, jam, noise


def test_power_inversion_nulls_a_dominant_rank_one_term():
    R, n, a_jam, jam, noise = _synthetic_R()
    K = len(a_jam)
    for ref in range(K):
        for loading in (0.0, 1e-3):
            w = ar.power_inversion(R, n, ref, loading)
            Rl = R / n + loading * np.trace(R / n).real / K * np.eye(K)
            e = np.zeros(K)
            e[ref] = 1.0
            u = np.linalg.solve(Rl, e)
            assert np.allclose(w, u / (e @ u), rtol=1e-12, atol=0) and abs(w[ref] - 1.0) < 1e-12
    # the unloaded solution leaves |w^H a|^2 / |w_ref|^2 = (sigma / (sigma + (K - 1) J))^2 of the jammer (Sherman-Morrison on
    # sigma I + J a a^H, |a_k| = 1): the loaded one, with sigma raised, stays below the reference element's 1 by orders too
    w = ar.power_inversion(R, n, 0, 0.0)
    unloaded = (noise / (noise + (K - 1) * jam)) ** 2
    assert abs(np.vdot(w, a_jam)) ** 2 / abs(w[0]) ** 2 <= unloaded * (1 + 1e-6)
    w = ar.power_inversion(R, n, 0)
    sigma = noise + ar.DEFAULT_LOADING * (noise + jam)
    assert abs(np.vdot(w, a_jam)) ** 2 / abs(w[0]) ** 2 <= (sigma / (sigma + (K - 1) * jam)) ** 2 * (1 + 1e-6) < 1e-5


def test_mvdr_keeps_the_steering_direction_and_nulls_the_jammer():
    R, n, a_jam, jam, noise = _synthetic_R()
    K = len(a_jam)
    a = np.exp(2j * np.pi * np.array([0.0, 0.11, 0.37, 0.62]))
    w = ar.mvdr(R, n, a)
    Rl = R / n + ar.DEFAULT_LOADING * np.trace(R / n).real / K * np.eye(K)
    u = np.linalg.solve(Rl, a)
    assert np.allclose(w, u / np.vdot(a, u).real, rtol=1e-12, atol=0)
    assert abs(np.vdot(w, a) - 1.0) < 1e-12 and abs(np.vdot(w, a_jam)) ** 2 < 1e-4
    for bad in (dict(R=np.eye(3)[:2], n=1, steering=a), dict(R=R, n=0, steering=a), dict(R=R, n=n, steering=a[:3]), dict(R=R, n=n, steering=a, loading=-1.0)):
        with pytest.raises(ValueError):
            ar.mvdr(**bad)


# ---------------------------------------------------------------------------------------------- 5. the C side without a device
def test_c_struct_prototypes_and_host_side_refusals(tmp_path):
    src = tmp_path / "array.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n",'
                   "sizeof(sdr_ddc_array),offsetof(sdr_ddc_array,n_elements),offsetof(sdr_ddc_array,flags),offsetof(sdr_ddc_array,lanes),"
                   "offsetof(sdr_ddc_array,weights),SDR_DDC_ARRAY_MEASURE);return 0;}\n")
    exe = tmp_path / "array"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    proto = tmp_path / "proto.c"
    proto.write_text('#include "sydr_amd.h"\n'
                     "int (*const create)(sdr_engine*, const sdr_ddc_cfg*, int, const sdr_ddc_layout*, const sdr_ddc_array*, sdr_ddc**) = sdr_ddc_create_array;\n"
                     "int (*const weights)(sdr_engine*, sdr_ddc*, const double*) = sdr_ddc_array_weights;\n"
                     "int (*const cov)(sdr_engine*, sdr_ddc*, double*, int64_t*, int) = sdr_ddc_array_covariance;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(REPO, "include"), "-c", str(proto),
                           "-o", str(tmp_path / "proto.o")])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.DdcArray
    assert got == [C.sizeof(A), A.n_elements.offset, A.flags.offset, A.lanes.offset, A.weights.offset, _lib.DDC_ARRAY_MEASURE]
    assert got == [168, 0, 4, 8, 40, ar.ARRAY_MEASURE]
    lib = _lib.load()
    assert lib.sdr_abi_version() == 5
    assert list(lib.sdr_ddc_create_array.argtypes) == [C.c_void_p, C.POINTER(_lib.DdcCfg), C.c_int, C.POINTER(_lib.DdcLayout), C.POINTER(A), C.POINTER(C.c_void_p)]
    assert lib.sdr_ddc_create_array(None, None, 1, None, None, None) != 0 and lib.sdr_ddc_array_weights(None, None, None) != 0
    assert lib.sdr_ddc_array_covariance(None, None, None, None, 0) != 0
    c = array_struct(ar.ArrayGeometry((5, 0, 2), [1 + 2j, 3 - 4j, 0.5j], measure=True))
    assert (c.n_elements, c.flags, list(c.lanes), [list(w) for w in c.weights][:3]) == (3, 1, [5, 0, 2, 0, 0, 0, 0, 0], [[1.0, 2.0], [3.0, -4.0], [0.0, 0.5]])


@host_check.requires_hipcc
def test_array_arithmetic_on_the_host():
    """sydr_amd/csrc/ddc_array.h, the decode and the combine the converter's kernels and its host side share, compiled for the host
    alone (tests/csrc/ddc_array_check.hip): limits, the K-element decode against a bit-by-bit reading, the combine's order against
    a restatement that stores every intermediate -- once as it is, once with contraction allowed to the compiler, which the
    header must withstand."""
    for flags in (("-O1",), ("-O3", "-ffp-contract=fast")):
        exe = host_check.build("ddc_array_check", flags)
        out = subprocess.run([str(exe)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
        assert int(out.stdout.split()[1]) > 30000


# ---------------------------------------------------------------------------------------------- 6. the jammed recording
def test_the_oracle_misses_on_one_element_and_finds_the_satellite_on_the_combination():
    """The 4-element recording of array_cases.jammed_recording (jammer 20 dB above the noise of an element, satellite 14 dB
    below it): the oracle's PCPS on element 0 alone falls under the plugin's ratio threshold of 1.5 at a wrong bin and code phase
    ([23, 579], ratio 1.45); on the statement-combined stream with power-inversion weights of the first 2 ms it finds bin 13,
    sample 2826 -- the satellite's 1750 Hz and (1023 - 300.25) chips of 3.91 samples -- with ratio 5.79."""
    from oracle import sydr_oracle as orc
    raw = cases.jammed_recording()
    fs, prn = cases.E2E_FS, cases.E2E_PRN
    n = orc.samples_per_code(fs)
    spectrum = orc.code_spectrum(orc.gold_code(prn), fs)

    def search(x):
        cmap = orc.pcps_map(x[:n].reshape(1, -1), 0.0, fs, spectrum, 5000.0, 250.0, n)
        return orc.two_peak_compare(cmap, n, round(fs / orc.CODE_RATE))

    true_sample = round((orc.CODE_CHIPS - cases.E2E_SAT["code_phase"]) * fs / orc.CODE_RATE)
    sr, si = ar.elements(raw, cases.E2E_LAYOUT, cases.E2E_LANES)
    peak, ratio = search(sr[0] + 1j * si[0])
    print(f"element 0: peak {peak}, ratio {ratio:.3f}")
    assert ratio < 1.5 and peak != [13, true_sample]
    R, count = ar.covariance(cases.piece(raw, cases.E2E_LAYOUT, 0, cases.E2E_TRAIN_MS * int(fs * 1e-3)), cases.E2E_LAYOUT, cases.E2E_LANES)
    w = ar.power_inversion(R, count)
    re, im = ar.combine(sr, si, w)
    peak, ratio = search(re + 1j * im)
    gain = abs(np.vdot(w, cases.E2E_JAMMER_DIRECTION)) ** 2 / abs(w[0]) ** 2
    print(f"combined: peak {peak}, ratio {ratio:.3f}; gain towards the jammer over the reference element's {10 * np.log10(gain):.1f} dB")
    assert peak == [13, true_sample] and true_sample == 2826 and ratio > 4.0
    # ... and the same two outcomes on the ci16 rings the statement makes of the recording ([RFSIGNAL] of array_cases.e2e_conf)
    cfg = dc.DownConverterConfig(dc.IN_R8, 1, np.ones(1), 0, 1.0 / 8.0, 1, cases.E2E_LAYOUT, ar.ArrayGeometry(cases.E2E_LANES))
    peak, ratio = search(orc.iq_to_complex(ar.statement(cfg, [raw], dc.FMT_CI16).astype(np.float64)))
    assert peak == [23, 579] and abs(ratio - 1.454) < 0.001, (peak, ratio)
    cfg.array.weights = w
    peak, ratio = search(orc.iq_to_complex(ar.statement(cfg, [raw], dc.FMT_CI16).astype(np.float64)))
    assert peak == [13, 2826] and abs(ratio - 5.777) < 0.001, (peak, ratio)


# ---------------------------------------------------------------------------------------------- 7. the [RFSIGNAL] keys and the manager
_conf = cases.e2e_conf


def test_ini_keys_parse_and_are_refused(tmp_path):
    from sydr_amd.signal.iqsource import RFSignal
    path = tmp_path / "array.bin"
    cases.jammed_recording(1).tofile(path)
    sig = RFSignal(_conf(path))
    cfg, plan = sig.frontEnd.config, sig.frontEnd.array
    assert cfg.layout == cases.E2E_LAYOUT and cfg.array.lanes == cases.E2E_LANES and not cfg.array.measure
    assert np.array_equal(cfg.array.weights, [1, 0, 0, 0]) and (plan.mode, plan.adaptive) == ("fixed", False)
    assert sig.totalSamples == 4000 and sig.samplesPerMs == 4000
    sig = RFSignal(_conf(path, array_weights="1,0, 0,1, -1,0, 0.5,-0.25", array_reference=2))
    assert np.array_equal(sig.frontEnd.config.array.weights, [1, 1j, -1, 0.5 - 0.25j])
    assert np.array_equal(RFSignal(_conf(path, array_reference=3)).frontEnd.config.array.weights, [0, 0, 0, 1])
    sig = RFSignal(_conf(path, array_mode="power_inversion", array_reference=1, array_loading=0.01, array_train_ms=3))
    cfg, plan = sig.frontEnd.config, sig.frontEnd.array
    assert cfg.array.measure and np.array_equal(cfg.array.weights, [0, 1, 0, 0])
    assert (plan.mode, plan.reference, plan.loading, plan.train_ms, plan.adaptive) == ("power_inversion", 1, 0.01, 3, True)
    sig = RFSignal(_conf(path, array_mode="MVDR", array_steering="1,0, 0,1, -1,0, 0,-1"))
    assert sig.frontEnd.array.mode == "mvdr" and np.array_equal(sig.frontEnd.array.steering, [1, 1j, -1, -1j]) and sig.frontEnd.array.train_ms == 2
    R, n = ar.covariance(cases.jammed_recording(1), cases.E2E_LAYOUT, cases.E2E_LANES)
    assert np.array_equal(sig.frontEnd.array.solve(R, n), ar.mvdr(R, n, [1, 1j, -1, -1j]))
    for bad, match in ((dict(sample_format=None, frame_fields=None), "sample_format"), (dict(array_lanes=None, array_mode="fixed"), "array_lanes"),
                       (dict(array_lanes=None, array_train_ms=2), "array_lanes"), (dict(decimation=None, filter_taps=None, output_gain=None), "front end"),
                       (dict(array_lanes="0"), "elements"), (dict(array_lanes="0,0"), "distinct"), (dict(array_lanes="0,7"), "fit"),
                       (dict(array_lanes="0,1,2,3,4,5,6,8,9"), "elements"), (dict(array_mode="music"), "array_mode"),
                       (dict(array_weights="1,0,0"), "pairs"), (dict(array_weights="1,0, 0,1, nan,0, 0,0"), "finite"),
                       (dict(array_reference=4), "array_reference"), (dict(array_loading=-1), "array_loading"), (dict(array_mode="mvdr"), "array_steering"),
                       (dict(array_mode="power_inversion", array_train_ms=0), "array_train_ms"), (dict(array_mode="power_inversion", array_weights="1,0,0,0,0,0,0,0"), "belong"),
                       (dict(array_loading=0.1), "belong"), (dict(array_mode="power_inversion", array_steering="1,0,0,0,0,0,0,0"), "belong"),
                       (dict(blanking_factor=5.0), "mitigator")):
        with pytest.raises(ValueError, match=match):
            RFSignal(_conf(path, **bad))


def test_the_manager_trains_solves_resets_and_restarts(tmp_path):
    """An adaptive mode through ChannelManager over a fake engine whose converter is the statement: train_ms pushes with unit
    weight on the reference element, one clearing read of the covariance, the solved weights set, one reset -- and then the
    recording from its first sample: the ring equals the statement's with that one weight vector, whatever the block length."""
    from fake_engine import OracleEngine
    from sydr_amd.channel.manager import ChannelManager
    from sydr_amd.signal.iqsource import RFSignal

    class ArrayOracleEngine(OracleEngine):
        def __init__(self):
            super().__init__()
            self.log = []

        def ddc_create(self, cfg):
            self.log.append("create")
            return ar.Statement(cfg)

        def ddc_push(self, ddc, raw, ring_offset=0):
            self.log.append(("push", ddc.n_seen, int(ring_offset), tuple(ddc.weights)))
            v = ddc.push(raw)
            self.iq_upload(dc.quantise(v, self.iq_fmt), ring_offset)
            return v.size

        ddc_push_queue = ddc_push

        def ddc_array_covariance(self, ddc, clear=False):
            self.log.append(("covariance", bool(clear)))
            return ddc.read_covariance(clear)

        def ddc_array_weights(self, ddc, w):
            self.log.append("weights")
            ddc.set_weights(w)

        def ddc_reset(self, ddc):
            self.log.append("reset")
            ddc.reset()

        def ddc_destroy(self, ddc):
            pass

        def sync(self):
            pass

    ms = cases.E2E_MS
    raw = cases.jammed_recording()
    path = tmp_path / "array.bin"
    raw.tofile(path)
    per_ms = int(cases.E2E_FS * 1e-3)
    R, n = ar.covariance(cases.piece(raw, cases.E2E_LAYOUT, 0, cases.E2E_TRAIN_MS * per_ms), cases.E2E_LAYOUT, cases.E2E_LANES)
    w = ar.power_inversion(R, n)
    rings = []
    for block in (1, 4):
        sig = RFSignal(_conf(path, array_mode="power_inversion", array_train_ms=cases.E2E_TRAIN_MS))
        eng = ArrayOracleEngine()
        mgr = ChannelManager(sig, engine=eng)
        e0 = tuple(ar.unit_weights(4, 0))
        assert eng.log == ["create", ("push", 0, 0, e0), ("push", per_ms, 0, e0), ("covariance", True), "weights", "reset"]
        assert np.array_equal(mgr.arrayWeights, w) and sig.position == 0
        for _ in range(ms // block):
            mgr.addNewRFData(sig.getMilliseconds(block))
        pushes = [entry for entry in eng.log[6:] if entry[0] == "push"]
        assert [p[1] for p in pushes] == list(range(0, ms * per_ms, block * per_ms)) and all(p[3] == tuple(w) for p in pushes)
        got_R, got_n = mgr.arrayCovariance()
        want_R, want_n = ar.covariance(raw, cases.E2E_LAYOUT, cases.E2E_LANES)
        assert got_n == want_n == ms * per_ms and np.array_equal(got_R, want_R)
        rings.append(eng.ring[:2 * ms * per_ms].copy())
        mgr.close()
    cfg = RFSignal(_conf(path, array_weights=",".join(f"{float(v.real).hex()},{float(v.imag).hex()}" for v in w))).frontEnd.config
    assert np.array_equal(cfg.array.weights, w)
    want = ar.statement(cfg, [raw], dc.FMT_CI16)
    assert np.array_equal(rings[0], want) and np.array_equal(rings[1], want) and np.any(want != 0)
    fixed = ChannelManager(RFSignal(_conf(path)), engine=ArrayOracleEngine())
    assert fixed.engine.log == ["create"] and fixed.arrayCovariance() is None
    fixed.close()
