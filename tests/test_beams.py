"""Beams without a device: the NumPy statements (sydr_amd/signal/array.py, stap.py `beams_statement`, `element_weights`,
`wiener_weights`), the C prototypes, the manager's followers over an oracle-backed engine, and why the feature exists."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import array_cases as acases
import beams_cases as cases
import packed_cases
from fake_engine import OracleEngine

from sydr_amd import _lib
from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
from sydr_amd.channel.manager import ChannelManager
from sydr_amd.signal import array as ar
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import stap
from sydr_amd.signal.iqsource import RFSignal
from sydr_amd.utils.enumerations import ChannelMessage

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- 10. the statement and the prototypes
@pytest.mark.parametrize("name", ["K3_int16_T33D2_R4", "K3_1bit_rational_R4", "stap3_K8_int8_T33D2_R4"])
def test_beams_statement_is_the_statement_per_weight_set(name):
    layout, lanes, shape, T, R = cases.SWEEP[name]
    cfg, raw, K, _ = cases.config(name, acases.FCWS["odd"])
    n = layout.frames_in(raw.nbytes)
    sets, _ = cases.weight_sets(K, T, R)
    fmts = cases.ring_formats(R)
    cut = [(0, 1000), (1000, 8), (1008, n - 1008)]
    pushes = cases.pieces(raw, layout, cut)
    changes = {1: {2: cases.general(K, T, 40)}, 2: {b: cases.general(K, T, 50 + b) for b in range(R)}}
    got = cases.beams_statement(cfg, sets, pushes, fmts, changes)
    one = stap.statement if T else ar.statement
    assert len(got) == R
    for b in range(R):
        own = {k: per[b] for k, per in changes.items() if b in per}
        want = one(cases.with_weights(cfg, sets[b]), pushes, fmts[b], weights_at=own)
        assert got[b].dtype == want.dtype and np.array_equal(got[b], want) and np.any(want != 0), (name, b)
    before = cfg.array.weights.copy()                                             # (cfg itself is left alone)
    assert np.array_equal(cases.with_weights(cfg, sets[0]).array.weights, sets[0]) and np.array_equal(cfg.array.weights, before)
    assert not np.array_equal(before, sets[0])


def test_element_and_wiener_weights():
    assert np.array_equal(ar.element_weights(4), np.eye(4)) and ar.element_weights(4).dtype == np.complex128
    e = stap.element_weights(3, 4, 1)
    assert e.shape == (4, 3, 4) and all(np.array_equal(e[a], stap.unit_weights(3, 4, a, 1)) for a in range(4))
    rng = np.random.default_rng(cases.SEED + 9)
    a_sig, a_jam = np.exp(2j * np.pi * rng.uniform(0, 1, 4)), np.exp(2j * np.pi * rng.uniform(0, 1, 4))
    R = 1e4 * np.outer(a_jam, a_jam.conj()) + np.eye(4)                    # a jammer 40 dB above unit noise
    w = ar.wiener_weights(R, a_sig, 0.0)
    assert np.allclose(R @ w, a_sig) and abs(np.vdot(w, a_jam)) < 1e-3 * abs(np.vdot(w, a_sig))
    loaded = ar.wiener_weights(R, a_sig, 0.5)
    assert np.allclose((R + 0.5 * np.trace(R).real / 4 * np.eye(4)) @ loaded, a_sig)
    for bad in (lambda: ar.wiener_weights(np.eye(9), np.ones(9)), lambda: ar.wiener_weights(np.eye(4), np.ones(3)),
                lambda: ar.wiener_weights(np.eye(4), np.ones(4), -1.0), lambda: ar.wiener_weights(np.eye(4), [1, 1, np.nan, 1])):
        with pytest.raises(ValueError):
            bad()
    # the space-time form on one tap is the array's
    Cl = R.reshape(1, 4, 4) * 7.0
    assert np.allclose(stap.wiener_weights(Cl, 7, a_sig, loading=0.0)[0], w)


def test_beam_prototypes_agree_with_the_c_compiler(tmp_path):
    """On the pattern of test_mit_struct_layouts_agree_with_the_c_compiler: the header's four declarations against function-pointer
    types written out here (a C compiler refuses a mismatch), SDR_DDC_MAX_BEAMS, and the ctypes argument lists."""
    proto = tmp_path / "proto.c"
    proto.write_text('#include "sydr_amd.h"\n'
                     "int (*const attach)(sdr_engine*, sdr_ddc*, sdr_engine*, const double*, int*) = sdr_ddc_beam_attach;\n"
                     "int (*const weights)(sdr_engine*, sdr_ddc*, int, const double*) = sdr_ddc_beam_weights;\n"
                     "int (*const count)(const sdr_ddc*) = sdr_ddc_beam_count;\n"
                     "int (*const clear)(sdr_engine*, sdr_ddc*) = sdr_ddc_beams_clear;\n"
                     "typedef char sixteen[SDR_DDC_MAX_BEAMS == 16 ? 1 : -1];\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(REPO, "include"), "-c", str(proto),
                           "-o", str(tmp_path / "proto.o")])
    lib = _lib.load()
    VP, PD = C.c_void_p, C.POINTER(C.c_double)
    assert list(lib.sdr_ddc_beam_attach.argtypes) == [VP, VP, VP, PD, C.POINTER(C.c_int)] and lib.sdr_ddc_beam_attach.restype is C.c_int
    assert list(lib.sdr_ddc_beam_weights.argtypes) == [VP, VP, C.c_int, PD]
    assert list(lib.sdr_ddc_beam_count.argtypes) == [VP] and list(lib.sdr_ddc_beams_clear.argtypes) == [VP, VP]
    # refusals that need no device
    assert lib.sdr_ddc_beam_count(None) == -1 and lib.sdr_ddc_beam_attach(None, None, None, None, None) != 0
    assert lib.sdr_ddc_beam_weights(None, None, 1, None) != 0 and lib.sdr_ddc_beams_clear(None, None) != 0


# ---------------------------------------------------------------------------------------------- 11. the manager
class BeamOracleEngine(OracleEngine):
    """The oracle-backed engine with the array converter's and the beams' entry points: a statement per beam, each quantised into
    the ring of its engine as that ring's format says -- what the device is held to (tests/test_gpu_beams.py)."""

    def __init__(self, device_id=0):
        super().__init__()
        self.beam_calls = dict(push=0, attach=0, weights=0)

    def ddc_create(self, cfg):
        return dict(cfg=cfg, beams=[(self, ar.Statement(cfg))])

    def ddc_beam_attach(self, ddc, target, weights):
        self.beam_calls["attach"] += 1
        assert ddc["beams"][0][1].n_seen == 0 and target is not self and target.iq_capacity == self.iq_capacity
        ddc["beams"].append((target, ar.Statement(ar.with_weights(ddc["cfg"], weights))))
        return len(ddc["beams"]) - 1

    def ddc_beam_weights(self, ddc, beam, weights):
        self.beam_calls["weights"] += 1
        ddc["beams"][beam][1].set_weights(weights)

    def ddc_push(self, ddc, raw, ring_offset=0):
        self.beam_calls["push"] += 1
        for engine, st in ddc["beams"]:
            v = st.push(raw)
            engine.iq_upload(dc.quantise(v, engine.iq_fmt), ring_offset)
        return v.size

    ddc_push_queue = ddc_push

    def ddc_destroy(self, ddc):
        pass

    def sync(self):
        pass

    def close(self):
        pass


class MitigatingBeamEngine(BeamOracleEngine):
    def ddc_create(self, cfg):
        return dict(cfg=cfg, beams=[])

    def ddc_mitigate(self, ddc, cfg):
        pass


def _ticks(leader, managers, sig, ms):
    out = [[] for _ in managers]
    for _ in range(ms):
        leader.addNewRFData(sig.getMilliseconds(1))
        for k, m in enumerate(managers):
            out[k].append([packed_cases.plain(p) for p in m.run()])
    return out


def test_followers_receive_what_a_plain_manager_receives_over_the_beams_stream(tmp_path):
    """array_cases.jammed_recording through a leader (beam 0: element 0, no channels) with two followers: beam 1 with the
    power-inversion weights, beam 2 with element 2, changed to the power-inversion weights after 3 ms.  Each follower's packets
    equal, tick for tick, those of a plain manager over a complex int16 file that holds the beam's statement output."""
    raw, ms, per_ms = acases.jammed_recording(), acases.E2E_MS, int(acases.E2E_FS * 1e-3)
    path = tmp_path / "array.bin"
    raw.tofile(path)
    R, n = ar.covariance(acases.piece(raw, acases.E2E_LAYOUT, 0, acases.E2E_TRAIN_MS * per_ms), acases.E2E_LAYOUT, acases.E2E_LANES)
    w = ar.power_inversion(R, n)
    sets = [ar.unit_weights(4, 0), w, ar.unit_weights(4, 2)]
    prn, cfg = acases.E2E_PRN, packed_cases.kaplan_config()
    sig = RFSignal(acases.e2e_conf(path))
    leader = ChannelManager(sig, engine=BeamOracleEngine())
    followers = [leader.addBeam(sets[1], engine=BeamOracleEngine()), leader.addBeam(sets[2], engine=BeamOracleEngine())]
    assert leader.beams() == followers and [f.beam for f in followers] == [1, 2]
    assert all(f.sharedBuffer.maxSize == leader.sharedBuffer.maxSize and f.engine is not leader.engine for f in followers)
    for f in followers:
        f.addChannel(ChannelL1CA_Kaplan, cfg, 1)
        f.requestTracking(prn)
        with pytest.raises(ValueError):
            f.addNewRFData(sig.getMilliseconds(0))
        with pytest.raises(ValueError):
            f.enableReadAhead(16)
    got = _ticks(leader, followers, sig, 3)
    assert [f.sharedBuffer.idxWrite for f in followers] == [leader.sharedBuffer.idxWrite] * 2 == [3 * per_ms] * 2
    leader.setBeamWeights(2, w)
    with pytest.raises(ValueError):
        leader.setBeamWeights(3, w)
    with pytest.raises(ValueError):
        leader.addBeam(w, engine=BeamOracleEngine())                              # after the first slab
    for k, part in enumerate(_ticks(leader, followers, sig, ms - 3)):
        got[k] += part
    assert leader.engine.beam_calls == dict(push=ms, attach=2, weights=1)         # one push per tick however many beams
    assert all(f.engine.beam_calls == dict(push=0, attach=0, weights=0) for f in followers)
    pushes = [acases.piece(raw, acases.E2E_LAYOUT, k * per_ms, per_ms) for k in range(ms)]
    want_rings = ar.beams_statement(sig.frontEnd.config, sets, pushes, [dc.FMT_CI16] * 3, weights_at={3: {2: w}})
    for b, m in enumerate([leader] + followers):
        assert np.array_equal(m.engine.ring[:2 * ms * per_ms], want_rings[b]), b
    for b, f in enumerate(followers, 1):
        beam_path = tmp_path / f"beam{b}.bin"
        want_rings[b].tofile(beam_path)
        plain_sig = RFSignal(dict(filepath=str(beam_path), sampling_frequency=acases.E2E_FS, is_complex="true", intermediate_frequency=0.0, data_size=16))
        want, plain_mgr = packed_cases.receive(plain_sig, OracleEngine(), prns=[prn], cfg=cfg, ms=ms, mode="ticks")
        assert len(got[b - 1]) == len(want) == ms
        for k, (x, y) in enumerate(zip(got[b - 1], want)):
            assert x == y, (b, k)
        acq = [p for tick in want for p in tick if p["type"] is ChannelMessage.ACQUISITION_UPDATE]
        assert len(acq) == 1 and ([int(acq[0]["frequency_idx"]), int(acq[0]["code_idx"])] == [13, 2826]) == (b == 1)
        plain_mgr.close()
    leader.close()


def test_add_beam_is_refused_where_the_issue_says(tmp_path):
    import mitigate_cases
    raw = acases.jammed_recording()
    path = tmp_path / "array.bin"
    raw.tofile(path)
    w = ar.unit_weights(4, 1)
    # a manager without a front end, and one whose front end is no array
    plain_path = tmp_path / "plain.bin"
    raw[:8000].tofile(plain_path)
    plain = ChannelManager(RFSignal(dict(filepath=str(plain_path), sampling_frequency=acases.E2E_FS, is_complex="true", intermediate_frequency=0.0,
                                         data_size=16)), engine=BeamOracleEngine())
    with pytest.raises(ValueError):
        plain.addBeam(w, engine=BeamOracleEngine())
    assert plain.beams() == []
    plain.close()
    # mitigation keys: beside the array's they are refused where the recording is opened (signal/iqsource.py); a manager that has
    # them is told so by addBeam
    with pytest.raises(ValueError):
        RFSignal(acases.e2e_conf(path, blanking_factor=6.0))
    mitigated = ChannelManager(mitigate_cases.write_jammed_and_mitigated(tmp_path)[0], engine=MitigatingBeamEngine())
    with pytest.raises(ValueError, match="mitigation"):
        mitigated.addBeam(w, engine=BeamOracleEngine())
    mitigated.close()
    # without addBeam a manager's addNewRFData is the class's converting route, untouched
    mgr = ChannelManager(RFSignal(acases.e2e_conf(path)), engine=BeamOracleEngine())
    assert mgr.addNewRFData.__func__ is ChannelManager._addNewRFData_converted and not hasattr(mgr, "_beams")
    f = mgr.addBeam(w, output_bits=8, engine=BeamOracleEngine())
    assert f.sharedBuffer.fmt == dc.FMT_CI8 and mgr.sharedBuffer.fmt == dc.FMT_CI16
    with pytest.raises(ValueError):
        mgr.addBeam(w, output_bits=12, engine=BeamOracleEngine())
    with pytest.raises(ValueError):
        f.addBeam(w, engine=BeamOracleEngine())
    mgr.close()


# ---------------------------------------------------------------------------------------------- 12. why the feature exists
def test_the_wiener_beam_from_element_prompts_finds_the_satellite():
    """array_cases.jammed_recording and two more draws of its noise, all on the CPU (beams_cases.why): power inversion on beam 0,
    the four element beams, their prompts over 6 ms at what beam 0 found, `wiener_weights`, the search on that beam.  Measured
    search ratios (element 0 / power inversion / Wiener): 1.454 / 5.777 / 6.128, 1.174 / 5.240 / 6.795, 1.110 / 4.994 / 6.883.
    The Wiener beam is ahead on all three draws, by 6 % on the first: no clear margin, so the ordering is recorded
    (docs/notes/beams.md) and not asserted.  Asserted: the Wiener beam and the power-inversion beam find the clean stream's bin
    and code phase above the ini files' ratio of 1.5; one element falls under it at a wrong place."""
    for seed in (0, 1, 2):
        found = cases.why(cases.jammed(seed))
        print(seed, {k: (v[0], round(float(v[1]), 3)) for k, v in found.items() if k != "weights"})
        assert found["wiener"][0] == [13, 2826] and found["wiener"][1] > 1.5, (seed, found["wiener"])
        assert found["power_inversion"][0] == [13, 2826] and found["power_inversion"][1] > 1.5, (seed, found["power_inversion"])
        assert found["element"][0] != [13, 2826] and found["element"][1] < 1.5, (seed, found["element"])
