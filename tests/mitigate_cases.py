"""Shared inputs, seeds and settings of the mitigation tests (test_mitigate.py, test_gpu_mitigate.py).

Every stream is seeded; the converter's statement v, the mitigator's settings and the statement's outputs y are computed once
per case and shared (lru_cache, the arrays read-only).  The blanker's level is not an integer, so that no p_m of an
integer-valued v lies at it; the limits stand a margin over the median bin.  A gate is a discontinuity: `assert_unambiguous`
is what every device-against-statement test asserts of the statement before it demands equal counters and equal bytes."""
from functools import lru_cache

import numpy as np

import downconvert_cases as dcases

from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import mitigate as mt

SEED = 7
N_INPUTS = 70001
NOISE_SIGMA, CW_AMPLITUDE, CW_CYCLES, N_PULSES, PULSE_AMPLITUDE, PULSE_LENGTH = 12.0, 40.0, 0.0613, 25, 110.0, 12
LEVEL, LEAD, HOLD, MARGIN_DB = 90.5, 2, 5, 10.0
NFFTS = [64, 1024, 4096]
CONVERTERS = [(1, 1), (33, 2)]                              # (T, D): the identity converter, a filter and a decimation
MODES = ["blank", "excise", "both"]
FCWS = dcases.FCWS


@lru_cache(maxsize=None)
def jammed(n: int = N_INPUTS, seed: int = SEED) -> np.ndarray:
    """n ci8 inputs (interleaved): complex noise, a carrier wave at CW_CYCLES cycles per sample, N_PULSES rectangular pulses."""
    rng = np.random.default_rng(seed)
    x = NOISE_SIGMA * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    x += CW_AMPLITUDE * np.exp(2j * np.pi * CW_CYCLES * np.arange(n))
    for at in rng.integers(0, n - PULSE_LENGTH, N_PULSES):
        x[at:at + PULSE_LENGTH] += PULSE_AMPLITUDE * np.exp(2j * np.pi * rng.random())
    return interleave(x)


def interleave(x: np.ndarray) -> np.ndarray:
    raw = np.empty(2 * x.size, dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    raw.setflags(write=False)
    return raw


def gain_for(T: int, ring_fmt: int) -> float:
    """1 for the identity converter (v is the recording's integers), else the converter tests' irrational gains."""
    return 1.0 if T == 1 else dcases.gain_for(dc.IN_CI8, ring_fmt)


def converter(T: int, D: int, fcw: int, gain: float) -> dc.DownConverterConfig:
    return dcases.config(dc.IN_CI8, T, D, fcw, gain)


@lru_cache(maxsize=32)
def converted(T: int, D: int, fcw: int, gain: float, n: int = N_INPUTS) -> np.ndarray:
    """The converter's statement v of jammed(n), one push; read-only."""
    v = dc.statement(converter(T, D, fcw, gain), [jammed(n)])
    v.setflags(write=False)
    return v


def settings(v: np.ndarray, nfft: int, mode: str, gain: float = 1.0) -> mt.MitigationConfig:
    """The case's mitigator: LEVEL (in the recording's units, so times the gain), LEAD, HOLD; limits MARGIN_DB over the median
    bin of v's first 32768 samples."""
    level = LEVEL * gain if mode in ("blank", "both") else 0.0
    if mode == "blank":
        return mt.MitigationConfig(level, LEAD, HOLD)
    return mt.MitigationConfig(level, LEAD, HOLD, nfft, mt.excision_limits(v[:32768], nfft, MARGIN_DB))


@lru_cache(maxsize=32)
def mitigated(T: int, D: int, fcw: int, gain: float, nfft: int, mode: str, n: int = N_INPUTS):
    """-> (the mitigator's settings, the statement's outputs of converted(...) in one push, its counters); read-only."""
    v = converted(T, D, fcw, gain, n)
    cfg = settings(v, nfft, mode, gain)
    st = mt.Statement(cfg)
    y = st.push(v)
    y.setflags(write=False)
    return cfg, y, st.stats


def tolerance(cfg: mt.MitigationConfig, ddc_cfg: dc.DownConverterConfig, v: np.ndarray, raw: np.ndarray) -> float:
    """B_mit of the largest |v| plus twice the converter's own gain * B (what the phasor's few ulp become on the way)."""
    return mt.tolerance(cfg, float(np.max(np.abs(v)))) + 2.0 * dc.tolerance(ddc_cfg, dcases.max_abs(dc.IN_CI8, raw))


def assert_unambiguous(cfg: mt.MitigationConfig, v: np.ndarray, y: np.ndarray, band: float, integer_ring: bool, what=None):
    """No bin within a relative 1e-9 of its limit, no sample's power within a relative 1e-12 of the squared level, and -- for
    an integer ring -- no component of y within the tolerance of a half-integer."""
    near_bin, near_level, bin_margin, level_margin = mt.ambiguous_gates(cfg, v, 1e-9, 1e-12)
    assert near_bin == 0 and near_level == 0, ("a gate near its threshold: change the seed", what, bin_margin, level_margin)
    if integer_ring:
        assert dc.ambiguous(y, band) == 0, ("statement output near a rounding tie: change the seed", what)
    return bin_margin, level_margin


def push_lengths(nfft: int) -> list:
    H = nfft // 2
    return [1, 2, H - 1, H, H + 1, nfft, 0, nfft + 1, 3 * nfft + 7]


def cut(seq: np.ndarray, lengths, width: int = 1) -> list:
    """seq cut into pieces of the given lengths (in samples of `width` elements), then the rest."""
    out, at = [], 0
    for n in lengths:
        out.append(seq[width * at:width * (at + n)])
        at += n
    out.append(seq[width * at:])
    return out


# ------------------------------------------------------------------------------------------------ the acquisition case
ACQ_FS, ACQ_PRN, ACQ_MS = 4.092e6, 5, 3
ACQ_SATELLITE = dict(prn=ACQ_PRN, doppler=1750.0, code_phase=300.25, phase=0.1, amp=1.6)
ACQ_CW_AMPLITUDE, ACQ_NFFT = 30.0, 1024


@lru_cache(maxsize=None)
def acquisition_streams():
    """One C/A satellite in noise (sigma 10, seed 3, 4.092 MHz, ci8), ACQ_MS milliseconds.  -> (clean, jammed): the second with
    a carrier wave of amplitude 30 at CW_CYCLES cycles per sample added before the rounding."""
    from oracle import sydr_oracle as orc
    n = ACQ_MS * orc.samples_per_code(ACQ_FS)
    clean = orc.synth_iq(ACQ_FS, n, [ACQ_SATELLITE], 10.0, 3)
    x = orc.iq_to_complex(clean.astype(np.float64)) + ACQ_CW_AMPLITUDE * np.exp(2j * np.pi * CW_CYCLES * np.arange(n))
    clean.setflags(write=False)
    return clean, interleave(x)


def acquire(raw_or_complex, start: int = 0):
    """The oracle's search of one millisecond from sample `start`: -> ([bin, sample], ratio of the two peaks)."""
    from oracle import sydr_oracle as orc
    n = orc.samples_per_code(ACQ_FS)
    rf = np.asarray(raw_or_complex)
    if not np.iscomplexobj(rf):
        rf = orc.iq_to_complex(rf.astype(np.float64))
    cmap = orc.pcps_map(rf[start:start + n].reshape(1, -1), 0.0, ACQ_FS, orc.code_spectrum(orc.gold_code(ACQ_PRN), ACQ_FS), 5000.0, 250.0, n)
    return orc.two_peak_compare(cmap, n, round(ACQ_FS / orc.CODE_RATE))


@lru_cache(maxsize=None)
def acquisition_mitigated():
    """-> (settings, the statement's output of the jammed stream as a ci8 ring holds it): the identity converter, an excisor of
    1024 points, limits 10 dB over the median bin."""
    _, jam = acquisition_streams()
    v = dc.statement(dc.DownConverterConfig(dc.IN_CI8), [jam])
    cfg = mt.MitigationConfig(0.0, 0, 0, ACQ_NFFT, mt.excision_limits(v, ACQ_NFFT, MARGIN_DB))
    ring = dc.quantise(mt.statement(cfg, [v]), dc.FMT_CI8)
    ring.setflags(write=False)
    return cfg, ring


# ------------------------------------------------------------------------------------------------ a jammed recording, end to end
REC_MS = 60


@lru_cache(maxsize=None)
def jammed_recording(ms: int = REC_MS) -> np.ndarray:
    """The converter tests' satellite (amp 30 in noise of sigma 10) at 4.092 MHz as complex int8, with the carrier wave."""
    from oracle import sydr_oracle as orc
    n = ms * orc.samples_per_code(ACQ_FS)
    raw = orc.synth_iq(ACQ_FS, n, [dcases.SATELLITE], 10.0, dcases.SEED + 61)
    x = orc.iq_to_complex(raw.astype(np.float64)) + ACQ_CW_AMPLITUDE * np.exp(2j * np.pi * CW_CYCLES * np.arange(n))
    return interleave(x)


def jammed_signal_conf(path, **more):
    """[RFSIGNAL] of that recording: the identity converter with an excisor and a blanker."""
    conf = dict(filepath=str(path), sampling_frequency=ACQ_FS, is_complex="true", intermediate_frequency=0.0, data_size=8,
                decimation=1, filter_taps=1, excision_nfft=1024, blanking_factor=6.0, blanking_lead=2, blanking_hold=5)
    conf.update(more)
    return conf


def write_jammed_and_mitigated(tmp_path, ms: int = REC_MS):
    """-> (RFSignal over the jammed file with the keys set, RFSignal over the statement's output stored as an ordinary complex
    int8 recording, that output)"""
    from sydr_amd.signal.iqsource import RFSignal
    jam_path, out_path = tmp_path / "jammed_ci8.bin", tmp_path / "mitigated_ci8.bin"
    raw = jammed_recording(ms)
    raw.tofile(jam_path)
    sig = RFSignal(jammed_signal_conf(jam_path))
    v = dc.statement(sig.frontEnd.config, [raw])
    out = dc.quantise(mt.statement(sig.frontEnd.mitigation, [v]), dc.FMT_CI8)
    out.tofile(out_path)
    plain = RFSignal(dict(filepath=str(out_path), sampling_frequency=ACQ_FS, is_complex="true", intermediate_frequency=0.0, data_size=8))
    return sig, plain, out
