"""What tests/test_ddm.py (CPU) and tests/test_gpu_ddm.py (MI355X) share: the statement of sdr_ddm (include/sydr_amd.h)
built on the oracle -- the oracle's EPL, unchanged, per segment, and the second stage in NumPy -- and the inputs both run it
on.  The CPU file proves on the model that the inputs are fair (the maximum is distinct beyond rounding, the truth is
recovered) and holds sydr_amd.dsp.ddm.ddm_statement equal to this model; the GPU file holds the device to the model.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import corr_cases as cc
import refine_cases as rc
from oracle import sydr_oracle as orc

FMT_CI8, FMT_CI16, FMT_CF32, FMT_CF64 = 0, 1, 2, 3
CAP_Z = cc.CAP           # z within this of the item's max |z|: the project's cap for accumulators
CAP_MAP = 4e-9           # map and the three values within this * B * (S * max|z|)^2: test_gpu_refine's bound on P, per block
MARGIN = 1e-6            # the model's maximum exceeds every other entry by more than this times itself (the refine tests')


def ddm_model(rf, code, fs, item, B, S, first, step, T, span, step_hz):
    """One item (slot, W, s0, f0, rem_carrier, rem_code, code_step) -> dict(z[Q][T], map[K][T], tau[Q], result)."""
    _, W, s0, f0, remc, remk, cstep = item
    W, s0, Q = int(W), int(s0), B * S
    pc = orc.pad_code(np.asarray(code, dtype=np.float64))
    spacings = first + step * np.arange(T)
    z = np.zeros((Q, T), complex)
    tau = np.zeros(Q)
    for q in range(Q):
        a, b = (q * W) // Q, ((q + 1) * W) // Q
        x = rf[(s0 + np.arange(a, b)) % len(rf)]
        remc_q = (remc + (-(f0 * 2.0 * np.pi * a / fs))) % (2 * np.pi)
        out = np.array(orc.epl(x, pc, fs, f0, remc_q, remk + float(a) * cstep, cstep, spacings)).reshape(T, 2)
        z[q] = out[:, 0] + 1j * out[:, 1]
        tau[q] = (a + b - 1) / 2.0 / fs
    K = 2 * int(np.floor(span / step_hz)) + 1
    d = (np.arange(K) - (K - 1) // 2) * step_hz
    rot = np.exp(-2j * np.pi * d[None, :] * tau[:, None])                     # [Q][K]
    cmap = np.zeros((K, T))
    for b in range(B):
        Z = np.zeros((K, T), complex)
        for s in range(S):
            Z = Z + rot[b * S + s][:, None] * z[b * S + s][None, :]
        cmap = cmap + np.abs(Z) ** 2
    k, j = np.unravel_index(cmap.argmax(), cmap.shape)                        # first maximum in row-major order
    away = np.abs(spacings - spacings[j]) >= 1.0
    rest = cmap[:, away]
    result = dict(peak_bin=int(k), peak_tap=int(j), peak_hz=f0 + d[k], peak_chips=spacings[j], peak_value=cmap[k, j],
                  second_value=rest.max() if rest.size else 0.0, noise_mean=rest.mean() if rest.size else 0.0)
    return dict(z=z, map=cmap, tau=tau, result=result)


def margin(cmap):
    """(maximum - the largest other entry) / maximum."""
    flat = np.sort(cmap.ravel())
    return (flat[-1] - flat[-2]) / flat[-1] if flat.size > 1 else 1.0


def true_phase(c, s0):
    """Code phase in chips of rc.acquired's satellite at sample s0, in [-L/2, L/2)."""
    cstep = orc.CODE_RATE * (1.0 + c["doppler"] / 1575.42e6) / c["fs"]
    p = (rc.CODE_PHASE + s0 * cstep) % orc.CODE_CHIPS
    return p - orc.CODE_CHIPS if p >= orc.CODE_CHIPS / 2 else p


def wrap_chips(x):
    return (x + orc.CODE_CHIPS / 2) % orc.CODE_CHIPS - orc.CODE_CHIPS / 2


SHAPES = ((2, 8), (1, 4), (4, 2))         # (B, S) of rows 0, 1, 2
REM_CODES = (1.5, -2.25, 0.0)


def _case(name, fs, fmt, ring, rf, codes, prns, items, B, S, first, step, T, span, step_hz, truth=None):
    return dict(name=name, fs=fs, fmt=fmt, ring=ring, rf=rf, capacity=len(rf), codes=codes, prns=prns, items=items, B=B, S=S,
                first=first, step=step, T=T, span=span, step_hz=step_hz, truth=truth)


def _acquired_case(name, fs, row, B, S, W, rem_code, first=-4.0, step=0.25, T=33, span=250.0, step_hz=12.5, fmt=FMT_CI8,
                   start_turns=0, start=None):
    dtype = np.int16 if fmt == FMT_CI16 else np.int8
    c = rc.acquired(fs, *rc.SATELLITES[row], dtype=dtype)
    ring, rf = cc._ring_of(c["raw"], fmt)
    s0 = c["s0"] if start is None else start(c, len(rf))
    item = (0, W(c["N"]), s0 + start_turns * len(rf), c["f0"], 0.1 + 0.37 * row, rem_code, orc.CODE_RATE / fs)
    return _case(name, fs, fmt, ring, rf, [c["code"]], [rc.PRN], [item], B, S, first, step, T, span, step_hz,
                 truth=dict(doppler=c["doppler"], phase=true_phase(c, s0 % len(rf))))


def _many_case():
    raw, rf, its = rc.many_items()
    N = orc.samples_per_code(4e6)
    items = []
    for i, (k, s0, f0) in enumerate(its):
        W = (4 * N + 3, 6 * N + 17, 8 * N + 37)[i % 3]
        items.append((k, W, s0, f0, 0.05 * i, (i % 5 - 2) * 0.75, orc.CODE_RATE / 4e6))
    prns = [s["prn"] for s in rc.MANY_SATS]
    return _case("items_32_4MHz", 4e6, FMT_CI8, raw, rf, [orc.gold_code(p) for p in prns], prns, items, 2, 8, -4.0, 0.25, 33,
                 250.0, 12.5)


def noise_case():
    """A window of noise alone (no satellite): the map has no peak."""
    fs, N = 4e6, orc.samples_per_code(4e6)
    raw = orc.synth_iq(fs, 12 * N, [], rc.SIGMA, 31)
    item = (0, 8 * N + 37, 2 * N + 5, 1500.0, 0.2, 0.0, orc.CODE_RATE / fs)
    return _case("noise_4MHz", fs, FMT_CI8, raw, orc.iq_to_complex(raw), [orc.gold_code(rc.PRN)], [rc.PRN], [item], 2, 8, -4.0,
                 0.25, 33, 250.0, 12.5)


_cases = None


def parity_cases():
    global _cases
    if _cases is not None:
        return _cases
    cs = []
    for fs, tag in ((4e6, "4MHz"), (10e6, "10MHz")):               # 4 MHz: the per-sample form; 10 MHz: the chip-run form
        for row in range(3):
            B, S = SHAPES[row]
            cs.append(_acquired_case(f"acq_{tag}_row{row}_B{B}_S{S}", fs, row, B, S, lambda N: 8 * N + 37, REM_CODES[row]))
    # a segment of 12 501 samples: several tiles, the accumulators carried across them
    cs.append(_acquired_case("tiles_25MHz_B1_S4", 25e6, 2, 1, 4, lambda N: 2 * N + 5, 0.5, first=-2.0, step=0.125))
    # segments of 2 and 3 samples
    cs.append(_acquired_case("tiny_W131_B8_S8", 4e6, 0, 8, 8, lambda N: 131, 0.25, first=-1.0, step=0.5, T=5, span=2000.0,
                             step_hz=500.0))
    # taps 1030 chips out, a window across the ring's end, start_sample five turns high
    cs.append(_acquired_case("far_taps_wrapped_4MHz", 4e6, 0, 2, 8, lambda N: 4 * N + 11, -700.3, first=-1030.0, step=7.5, T=33,
                             start_turns=5, start=lambda c, cap: cap - (4 * c["N"] + 11) // 3))
    cs.append(_acquired_case("one_bin_S1_4MHz", 4e6, 1, 4, 1, lambda N: 8 * N + 37, 0.5, span=5.0, step_hz=12.5))   # K = 1
    cs.append(_acquired_case("taps_1_4MHz", 4e6, 1, 2, 8, lambda N: 8 * N + 37, 0.0, first=0.0, step=0.25, T=1))
    cs.append(_acquired_case("taps_1024_4MHz", 4e6, 0, 1, 4, lambda N: N, 1.5, first=-8.0, step=1.0 / 64, T=1024))
    for fmt, tag in ((FMT_CI16, "ci16"), (FMT_CF32, "cf32"), (FMT_CF64, "cf64")):
        cs.append(_acquired_case(f"fmt_{tag}_4MHz", 4e6, 0, 2, 8, lambda N: 8 * N + 37, 1.5, fmt=fmt))
    cs.append(_many_case())
    _cases = {c["name"]: c for c in cs}
    assert len(_cases) == len(cs)
    return _cases


_models = {}


def case_model(case):
    """-> [ddm_model(...) per item], cached and left unchanged."""
    if case["name"] not in _models:
        _models[case["name"]] = [ddm_model(case["rf"], case["codes"][it[0]], case["fs"], it, case["B"], case["S"], case["first"],
                                           case["step"], case["T"], case["span"], case["step_hz"]) for it in case["items"]]
    return _models[case["name"]]
