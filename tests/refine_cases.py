"""What tests/test_refine.py (CPU) and tests/test_gpu_refine.py (MI355X) share: the NumPy statement of sdr_acq_refine
(include/sydr_amd.h) on top of the oracle's EPL, and the inputs both run it on -- the CPU file proves on the model that
the inputs are fair (the maximum is distinct, the truth is recovered), the GPU file holds the device to the model.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sydr_oracle as orc


def refine_model(rf, s0, code, fs, f0, M, S, span, step, code_hz=orc.CODE_RATE):
    """-> (fine_hz, bit_edge, fine_idx, P[M][K], z[M][S]).  `rf`: complex samples, indexed periodically (a ring)."""
    L = len(code)
    N = int(np.rint(fs * L / code_hz))
    cstep = code_hz / fs
    pc = orc.pad_code(code)
    z = np.zeros((M, S), complex)
    tau = np.zeros((M, S))
    for m in range(M):
        for s in range(S):
            a, b = m * N + (s * N) // S, m * N + ((s + 1) * N) // S
            remc = (-(f0 * 2.0 * np.pi * a / fs)) % (2 * np.pi)
            x = rf[(s0 + np.arange(a, b)) % len(rf)]
            c = orc.epl(x, pc, fs, f0, remc, ((s * N) // S) * cstep, cstep, [0.0])
            z[m, s] = c[0] + 1j * c[1]
            tau[m, s] = (a + b - 1) / 2.0 / fs
    K = 2 * int(np.floor(span / step)) + 1
    d = (np.arange(K) - (K - 1) // 2) * step
    rot = np.exp(-2j * np.pi * d[None, None, :] * tau[:, :, None])
    per = (z[:, :, None] * rot).sum(axis=1)          # Z[m][k]
    P = np.empty((M, K))
    for h in range(M):
        sg = np.where(np.arange(M) < h, 1.0, -1.0) if h else np.ones(M)
        P[h] = np.abs((sg[:, None] * per).sum(axis=0)) ** 2
    h, k = np.unravel_index(P.argmax(), P.shape)     # first maximum in row-major order
    return f0 + d[k], int(h), int(k), P, z


def margin(P):
    """(maximum - the largest other entry) / maximum."""
    flat = np.sort(P.ravel())
    return (flat[-1] - flat[-2]) / flat[-1]


def hypothesis_ratio(P):
    """Best hypothesis over the second best (each at its own best frequency)."""
    rows = np.sort(P.max(axis=1))
    return rows[-1] / rows[-2] if len(rows) > 1 else np.inf


ALTERNATING = np.ones(60, int)
ALTERNATING[1::2] = -1

# (seed, true Doppler, code periods between the acquisition result and the window): Dopplers off the half-step points
# of a 5 Hz grid, windows that hold a data-bit edge or none
SATELLITES = ((1, 1630.0, 0), (2, -2381.0, 7), (3, 4120.0, 13), (4, 877.0, 16), (5, -3499.0, 3))
RECOVERY = SATELLITES[:4]      # the recovery cases: windows 0, 7, 13 and 16 periods behind the acquisition (the fifth row serves parity)
RATES = (4e6, 10e6, 25e6)
CODE_PHASE, PRN, SIGMA = 300.25, 7, 20.0


def amplitude(fs):
    return 8.0 if fs == 4e6 else 6.0


_cache = {}


def acquired(fs, seed, dop, periods_later, dtype=np.int8):
    """An oracle-synthesised satellite (alternating data bits), acquired by the oracle's PCPS on its first millisecond.
    -> dict(raw, rf, code, s0 = the sample tracking would start at + periods_later periods, f0 = the PCPS bin's carrier,
    true_edge(M))."""
    key = (fs, seed, dop, periods_later, np.dtype(dtype).name)
    if key in _cache:
        return _cache[key]
    N = orc.samples_per_code(fs)
    raw = orc.synth_iq(fs, 40 * N, [dict(prn=PRN, doppler=dop, code_phase=CODE_PHASE, phase=0.3, amp=amplitude(fs),
                                         data=ALTERNATING)], SIGMA, seed, dtype=dtype)
    rf = orc.iq_to_complex(raw)
    code = orc.gold_code(PRN)
    cmap = orc.pcps_map(rf[:N].reshape(1, -1), 0.0, fs, orc.code_spectrum(code, fs), 5000.0, 250.0, N)
    peak, _ = orc.two_peak_compare(cmap, N, round(fs / orc.CODE_RATE))
    f0, _, cs = orc.post_acquisition(0.0, 5000.0, 250.0, peak, 0, N, orc.required_samples(0.0, orc.CODE_RATE / fs))
    s0 = cs + periods_later * N
    cstep = orc.CODE_RATE * (1 + dop / 1575.42e6) / fs
    period0 = int(np.floor((CODE_PHASE + s0 * cstep) / orc.CODE_CHIPS + 0.5))    # code period that begins at the window's start
    edge = (-period0) % orc.MS_PER_BIT                                           # bits change every 20 periods

    def true_edge(M):
        return int(edge) if edge < M else 0
    out = dict(raw=raw, rf=rf, code=code, s0=int(s0), f0=float(f0), true_edge=true_edge, fs=fs, doppler=dop, N=N)
    _cache[key] = out
    return out


def code_start(fs, code_phase, dop, L=orc.CODE_CHIPS, code_hz=orc.CODE_RATE):
    """First sample at which a code period begins, for a satellite synthesised with `code_phase` chips at sample 0."""
    cstep = code_hz * (1.0 + dop / 1575.42e6) / fs
    return int(np.ceil((L - code_phase) / cstep))


MANY_SATS = tuple(dict(prn=p, doppler=d, code_phase=c, phase=0.1 * k, amp=7.0, data=ALTERNATING) for k, (p, d, c) in enumerate(
    ((3, 1630.0, 100.5), (7, -2381.0, 300.25), (11, 4120.0, 612.75), (14, 877.0, 17.5),
     (19, -3499.0, 900.0), (22, 2244.0, 455.5), (27, -1113.0, 250.25), (31, 3368.0, 777.0))))


def many_items(fs=4e6, seed=11):
    """Eight satellites in one recording and 32 items on them: every satellite from four different code periods on.
    -> (raw, rf, [(prn index, s0, f0)] * 32)."""
    key = ("many", fs, seed)
    if key not in _cache:
        N = orc.samples_per_code(fs)
        raw = orc.synth_iq(fs, 40 * N, list(MANY_SATS), SIGMA, seed)
        items = []
        for later in (0, 5, 11, 18):
            for k, s in enumerate(MANY_SATS):
                f0 = 250.0 * np.round(s["doppler"] / 250.0)
                items.append((k, code_start(fs, s["code_phase"], s["doppler"]) + later * N, float(f0)))
        _cache[key] = (raw, orc.iq_to_complex(raw), items)
    return _cache[key]


LONG_CHIPS, LONG_DOPPLER, LONG_PHASE = 4092, 1630.0, 1000.5


def long_code_case(fs=4e6, seed=21):
    """A 4092-chip +-1 code at 1.023 Mchip/s (4 ms periods), no data bits: -> (raw, rf, code, s0, f0)."""
    key = ("long", fs, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        code = rng.integers(0, 2, LONG_CHIPS) * 2.0 - 1.0
        N = int(np.rint(fs * LONG_CHIPS / orc.CODE_RATE))
        n = np.arange(8 * N, dtype=np.float64)
        cstep = orc.CODE_RATE * (1.0 + LONG_DOPPLER / 1575.42e6) / fs
        chips = LONG_PHASE + n * cstep
        x = 8.0 * code[np.floor(chips).astype(np.int64) % LONG_CHIPS] * np.exp(2j * np.pi * (LONG_DOPPLER / fs * n + 0.2))
        x += SIGMA * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
        raw = np.empty(2 * n.size, dtype=np.int8)
        raw[0::2] = np.clip(np.rint(x.real), -127, 127)
        raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
        s0 = code_start(fs, LONG_PHASE, LONG_DOPPLER, LONG_CHIPS)
        _cache[key] = (raw, orc.iq_to_complex(raw), code, s0, 1750.0)
    return _cache[key]
