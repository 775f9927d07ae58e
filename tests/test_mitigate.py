"""Pulse blanking and narrow-band excision in front of the ring, everything that needs no GPU: the NumPy statement
(sydr_amd/signal/mitigate.py) against brute-force restatements and against itself however the stream is cut; the helpers
that measure a level and limits; the [RFSIGNAL] keys; the acquisition case that motivates the stage, through the oracle; the
manager's route over the oracle-backed engine; the C structs' layout; the shared index arithmetic run on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from fake_engine import OracleEngine
import downconvert_cases as dcases
import host_check
import mitigate_cases as cases
import packed_cases

from sydr_amd import _lib
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt
from sydr_amd.signal.iqsource import RFSignal
from sydr_amd.utils.enumerations import ChannelMessage



def stream(n=20001):
    return cases.converted(1, 1, 0, 1.0, n)


# ---------------------------------------------------------------------------------------------- 1. the statement
@pytest.mark.parametrize("nfft", [64, 1024, 4096])
def test_overlap_add_is_the_identity_with_infinite_limits_and_the_delay(nfft):
    v = stream()
    cfg = mt.MitigationConfig(nfft=nfft, limit=np.full(nfft, np.inf))
    assert cfg.delay == nfft and cfg.state_length == 2 * nfft - 1
    st = mt.Statement(cfg)
    y = st.push(np.concatenate([v, np.zeros(cfg.delay)]))        # (the tail comes out behind L more zeros)
    assert y.size == v.size + nfft and np.all(y[:nfft] == 0.0)
    err = float(np.max(np.abs(y[nfft:] - v)))
    print(f"N = {nfft}: max |y - u| = {err:.2e} on |v| <= {np.abs(v).max():.0f}")
    assert err <= mt.tolerance(cfg, np.abs(v).max())
    assert st.stats.n_bins_excised == 0 and st.stats.n_segments == mt.segments_finished(y.size, nfft, nfft) == (y.size - 2 * nfft) // (nfft // 2) + 2
    # with a blanker in front the delay grows by its lead; without one lead and hold mean nothing
    assert mt.MitigationConfig(5.0, 7, 9, nfft, np.ones(nfft)).delay == nfft + 7
    assert mt.MitigationConfig(5.0, 7, 9, nfft, np.ones(nfft)).state_length == 2 * nfft - 1 + 16
    assert mt.MitigationConfig(5.0, 7, 9).delay == 7 and mt.MitigationConfig(5.0, 7, 9).state_length == 16
    assert mt.MitigationConfig(0.0, 7, 9, nfft, np.ones(nfft)).delay == nfft


def brute_blanker(v, level, lead, hold):
    t = [re * re + im * im > level * level for re, im in zip(v.real.tolist(), v.imag.tolist())]
    b = [any(t[max(m - hold, 0):m + lead + 1]) for m in range(len(t))]
    return np.array(t), np.array(b)


@pytest.mark.parametrize("lead,hold", [(0, 0), (2, 5), (5, 2), (0, 40), (1024, 1024)])
def test_blanker_dilation_against_a_loop(lead, hold):
    v = stream(6001).copy()
    v[0], v[-1], v[3000] = 120 + 5j, -3 + 125j, 100 - 100j       # triggers at the stream's first and last sample
    cfg = mt.MitigationConfig(cases.LEVEL, lead, hold)
    t, b = brute_blanker(v, cases.LEVEL, lead, hold)
    assert t[0] and t[-1] and 3 < t.sum() < t.size // 10
    st = mt.Statement(cfg)
    y = st.push(np.concatenate([v, np.zeros(lead)]))
    assert np.all(y[:lead] == 0.0)
    u = y[lead:]
    assert np.array_equal(u, np.where(b, 0.0, v))
    # before the tail was pushed the counters covered the u delivered by then; with it, all of them
    assert st.stats.n_triggers == int(t.sum()) and st.stats.n_blanked == int(b.sum()) and st.stats.n_outputs == v.size + lead
    part = mt.Statement(cfg)
    part.push(v[:4000])
    assert part.stats.n_triggers == int(t[:4000 - lead].sum()) and part.stats.n_blanked == int(b[:4000 - lead].sum())


def brute_counters(cfg, v, n):
    """The counters after n outputs, by the definitions: whole-stream arrays, no state."""
    N, H, L = cfg.nfft, cfg.nfft // 2, cfg.delay
    u = v
    triggers = blanked = 0
    if cfg.blanking:
        t, b = brute_blanker(v, cfg.blank_level, cfg.lead, cfg.hold)
        u = np.where(b, 0.0, v)
        triggers, blanked = int(t[:max(n - L, 0)].sum()), int(b[:max(n - L, 0)].sum())
    bins, segments = np.zeros(N, dtype=np.int64), 0
    if N:
        pad = np.concatenate([np.zeros(H), u])                   # pad[x] = u_{x - H}
        s = -1
        while s * H + N <= n - L:
            A = np.fft.fft(mt.hann(N) * pad[(s + 1) * H:(s + 1) * H + N])
            bins += A.real * A.real + A.imag * A.imag > cfg.limit
            segments += 1
            s += 1
    return mt.Stats(n, triggers, blanked, segments, int(bins.sum()), bins)


@pytest.mark.parametrize("mode", cases.MODES)
def test_counters_against_a_restatement(mode):
    v = stream()
    cfg = cases.settings(v, 256, mode)
    st = mt.Statement(cfg)
    at = 0
    for k in (1, 100, 127, 128, 129, 391, 5000, 7001):
        st.push(v[at:at + k])
        at += k
        assert st.stats == brute_counters(cfg, v, at), (mode, at)
    assert mode == "excise" or st.stats.n_triggers > 0
    assert mode == "blank" or st.stats.n_bins_excised > 0


@pytest.mark.parametrize("nfft,mode", [(64, "both"), (1024, "both"), (4096, "excise"), (1024, "blank")])
def test_statement_is_bit_identical_however_the_stream_is_cut(nfft, mode):
    v = stream(30001)
    cfg = cases.settings(v, nfft, mode)
    whole = mt.Statement(cfg)
    y = whole.push(v)
    st = mt.Statement(cfg)
    parts = [st.push(piece) for piece in cases.cut(v, cases.push_lengths(nfft))]
    assert [p.size for p in parts[:9]] == cases.push_lengths(nfft)
    assert np.concatenate(parts).tobytes() == y.tobytes() and st.stats == whole.stats
    st.reset()
    assert st.stats == mt.Statement(cfg).stats and st.push(v).tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------- 2. the helpers
def test_level_and_limits_on_jammed_noise_are_the_clean_noises():
    """Noise with pulses and a carrier wave that stands 19 dB over the floor of a 1024-point bin but holds an eighth of the
    noise's power (the level is a statistic of |v|^2 sample by sample: robust against what is rare, not against a continuous
    wave as strong as the noise -- that one the excisor takes out): both helpers land within 1 dB of the clean noise's."""
    n, sigma, nfft = 65536, 12.0, 1024
    rng = np.random.default_rng(cases.SEED + 1)
    clean = sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    dirty = clean + 6.0 * np.exp(2j * np.pi * cases.CW_CYCLES * np.arange(n))
    for at in rng.integers(0, n - 12, 60):
        dirty[at:at + 12] += 110.0
    db = lambda a, b: abs(10.0 * np.log10(a / b))
    assert db(mt.excision_limits(dirty, nfft, 10.0)[0], mt.excision_limits(clean, nfft, 10.0)[0]) < 1.0
    assert db(mt.blanking_level(dirty, 4.0) ** 2, mt.blanking_level(clean, 4.0) ** 2) < 1.0
    # ... and are what they say: the level `factor` times the noise's RMS amplitude, the limit `margin` over the mean bin
    assert db(mt.blanking_level(clean, 4.0) ** 2, 16.0 * 2.0 * sigma ** 2) < 0.2
    lim = mt.excision_limits(clean, nfft, 10.0)
    assert np.all(lim == lim[0]) and db(lim[0], 10.0 * 2.0 * sigma ** 2 * float(np.sum(mt.hann(nfft) ** 2))) < 0.5
    with pytest.raises(ValueError):
        mt.excision_limits(clean[:1000], nfft)


def test_config_validation():
    ok = np.ones(64)
    for bad in (dict(), dict(blank_lead=3, blank_hold=3), dict(blank_level=-1.0), dict(blank_level=float("nan")),
                dict(blank_level=1.0, blank_lead=1025), dict(blank_level=1.0, blank_hold=-1), dict(nfft=64), dict(nfft=32, limit=np.ones(32)),
                dict(nfft=8192, limit=np.ones(8192)), dict(nfft=96, limit=np.ones(96)), dict(nfft=64, limit=np.ones(63)),
                dict(nfft=64, limit=-ok), dict(nfft=64, limit=np.where(np.arange(64) == 5, np.nan, 1.0))):
        with pytest.raises(ValueError):
            mt.MitigationConfig(**bad)
    cfg = mt.MitigationConfig(2.5, 1024, 1024, 4096, np.full(4096, np.inf))
    assert cfg.blanking and cfg.limit.dtype == np.float64 and cfg.delay == 4096 + 1024
    assert mt.tolerance(mt.MitigationConfig(2.5), 128.0) == 0.0
    assert abs(mt.tolerance(mt.MitigationConfig(nfft=1024, limit=np.ones(1024)), 128.0) - 16 * 10 * 1024 * 2.0 ** -53 * 128.0) < 1e-20


# ---------------------------------------------------------------------------------------------- 3. [RFSIGNAL]
def test_rfsignal_mitigation_keys(tmp_path):
    path = tmp_path / "jammed.bin"
    raw = cases.jammed_recording(10)
    raw.tofile(path)
    sig = RFSignal(cases.jammed_signal_conf(path))
    fe = sig.frontEnd
    assert fe.config.n_taps == 1 and fe.config.decimation == 1 and fe.config.fcw == 0 and fe.config.in_fmt == dc.IN_CI8   # the identity
    assert (sig.samplingFrequency, sig.samplesPerMs) == (cases.ACQ_FS, 4092)
    m = fe.mitigation
    assert m is fe.mitigation                                     # measured once
    v = dc.statement(fe.config, [raw[:2 * 8 * 4092]])             # calibration_ms defaults to 8
    assert (m.nfft, m.blank_lead, m.blank_hold) == (1024, 2, 5) and fe.delay == m.delay == 1026
    assert m.blank_level == mt.blanking_level(v, 6.0) and np.array_equal(m.limit, mt.excision_limits(v, 1024, 10.0))
    other = RFSignal(cases.jammed_signal_conf(path, calibration_ms=3, excision_margin_db=13.0, excision_nfft=256)).frontEnd.mitigation
    assert np.array_equal(other.limit, mt.excision_limits(dc.statement(fe.config, [raw[:2 * 3 * 4092]]), 256, 13.0))
    only = {k: v for k, v in cases.jammed_signal_conf(path).items() if not k.startswith("blanking")}
    assert RFSignal(only).frontEnd.mitigation.blank_level == 0.0 and RFSignal(only).frontEnd.delay == 1024
    none = {k: v for k, v in only.items() if k != "excision_nfft"}
    assert RFSignal(none).frontEnd.mitigation is None and RFSignal(none).frontEnd.delay == 0
    # refused: the keys without a front end, the keys without a stage, values out of range
    plain = {k: v for k, v in cases.jammed_signal_conf(path).items() if k not in ("decimation", "filter_taps")}
    with pytest.raises(ValueError, match="decimation"):
        RFSignal(plain)
    for bad in (dict(none, blanking_lead=3), dict(none, calibration_ms=4), dict(only, excision_nfft=100), dict(only, excision_nfft=8192),
                dict(only, blanking_factor=0.0), dict(only, blanking_factor=4.0, blanking_hold=2000), dict(only, calibration_ms=0)):
        with pytest.raises(ValueError):
            RFSignal(bad)


# ---------------------------------------------------------------------------------------------- 4. why: acquisition under a jammer
def test_acquisition_is_lost_to_the_jammer_and_comes_back():
    """One C/A satellite (PRN 5, amplitude 1.6 in noise of sigma 10) and a carrier wave of amplitude 30: the oracle's search of
    one millisecond finds a wrong bin and sample on the raw stream, and on the statement's output -- behind its delay L -- the
    clean stream's bin and sample with a ratio above 2."""
    clean, jam = cases.acquisition_streams()
    cfg, ring = cases.acquisition_mitigated()
    peak, ratio = cases.acquire(clean)
    lost, lost_ratio = cases.acquire(jam)
    back, back_ratio = cases.acquire(ring, cfg.delay)
    print(f"clean {peak} {ratio:.2f}, jammed {lost} {lost_ratio:.2f}, mitigated {back} {back_ratio:.2f}")
    assert ratio > 2.0 and lost != peak and lost_ratio < 1.5
    assert back == peak and back_ratio > 2.0
    # the same through one more code period: the peak sample moves with L modulo the code's length
    n = 4092
    shifted, _ = cases.acquire(ring, 0)
    assert shifted[0] == peak[0] and shifted[1] == (peak[1] + cfg.delay) % n


# ---------------------------------------------------------------------------------------------- 5. the manager
class MitigatingOracleEngine(OracleEngine):
    """The oracle-backed engine with the converter's and the mitigator's entry points: the two statements in a row, quantised
    as the ring's format says -- what the device's kernels are held to (tests/test_gpu_mitigate.py)."""

    def __init__(self):
        super().__init__()
        self.mit_calls = dict(mitigate=0, push=0)

    def ddc_create(self, cfg):
        return dict(ddc=dc.Statement(cfg), mit=None)

    def ddc_mitigate(self, ddc, cfg):
        self.mit_calls["mitigate"] += 1
        ddc["mit"] = mt.Statement(cfg) if cfg is not None else None

    def ddc_mitigation_stats(self, ddc):
        return ddc["mit"].stats

    def ddc_push(self, ddc, raw, ring_offset=0):
        self.mit_calls["push"] += 1
        v = ddc["ddc"].push(raw)
        self.iq_upload(dc.quantise(ddc["mit"].push(v) if ddc["mit"] is not None else v, self.iq_fmt), ring_offset)
        return v.size

    ddc_push_queue = ddc_push

    def ddc_destroy(self, ddc):
        pass

    def sync(self):
        pass


def test_manager_over_a_jammed_recording_equals_the_mitigated_recording(tmp_path):
    sig, plain_sig, out = cases.write_jammed_and_mitigated(tmp_path)
    ms, prn = cases.REC_MS, dcases.SATELLITE["prn"]
    cfg = packed_cases.kaplan_config()
    eng = MitigatingOracleEngine()
    got, mgr = packed_cases.receive(sig, eng, prns=[prn], cfg=cfg, ms=ms, mode="ticks")
    want, want_mgr = packed_cases.receive(plain_sig, MitigatingOracleEngine(), prns=[prn], cfg=cfg, ms=ms, mode="ticks")
    assert len(got) == len(want) == ms
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, k
    assert packed_cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 1 and packed_cases.count(got) > 40
    assert np.array_equal(eng.ring, want_mgr.engine.ring)
    assert eng.mit_calls == dict(mitigate=1, push=ms) and want_mgr.engine.mit_calls == dict(mitigate=0, push=0)   # attached once, no call per tick
    stats = mgr.mitigationStats()
    assert stats.n_outputs == ms * 4092 and stats.n_bins_excised > 0 and want_mgr.mitigationStats() is None
    # a recording with a front end but without the keys never meets the mitigator
    bare = {k: v for k, v in cases.jammed_signal_conf(sig.filepath).items() if not k.startswith(("blanking", "excision"))}
    _, bare_mgr = packed_cases.receive(RFSignal(bare), MitigatingOracleEngine(), prns=[prn], cfg=cfg, ms=2, mode="ticks")
    assert bare_mgr.engine.mit_calls == dict(mitigate=0, push=2) and bare_mgr.mitigationStats() is None


# ---------------------------------------------------------------------------------------------- 6. the C structs
def test_mit_struct_layouts_agree_with_the_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   "sizeof(sdr_mit_cfg),offsetof(sdr_mit_cfg,nfft),offsetof(sdr_mit_cfg,blank_lead),offsetof(sdr_mit_cfg,blank_hold),"
                   "offsetof(sdr_mit_cfg,flags),offsetof(sdr_mit_cfg,blank_level),offsetof(sdr_mit_cfg,limit),sizeof(sdr_mit_stats),"
                   "offsetof(sdr_mit_stats,n_bins_excised));return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    M, S = _lib.MitCfg, _lib.MitStats
    assert got == [C.sizeof(M), M.nfft.offset, M.blank_lead.offset, M.blank_hold.offset, M.flags.offset, M.blank_level.offset, M.limit.offset,
                   C.sizeof(S), S.n_bins_excised.offset]
    assert got == [32, 0, 4, 8, 12, 16, 24, 40, 32]
    lib = _lib.load()
    for name in ("sdr_ddc_mitigate", "sdr_ddc_delay", "sdr_ddc_mitigation_stats"):
        assert hasattr(lib, name)
    assert lib.sdr_ddc_delay(None) == -1                          # (host arithmetic: refuses without a GPU too)
    assert lib.sdr_abi_version() == 5


# ---------------------------------------------------------------------------------------------- 7. the index arithmetic
@host_check.requires_hipcc
def test_push_segment_and_state_arithmetic_on_the_host():
    """sydr_amd/csrc/mit_plan.h, the arithmetic the mitigator's kernels and its host side share, compiled for the host alone
    and held against a brute-force restatement over small N, lead, hold, push lengths, ring offsets and capacities
    (tests/csrc/mit_plan_check.hip)."""
    exe = host_check.build("mit_plan_check")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 100000
