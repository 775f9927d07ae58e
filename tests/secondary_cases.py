"""What tests/test_secondary.py (CPU) and tests/test_gpu_secondary.py (MI355X) share: the NumPy statement of
sdr_acq_secondary (include/sydr_amd.h) on top of the oracle's EPL, and the inputs both run it on -- the CPU file proves on
the model that the inputs are fair (the maximum is distinct, phase and frequency are recovered), the GPU file holds the
device to the model.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sydr_oracle as orc
from refine_cases import hypothesis_ratio, margin  # noqa: F401  (the two figures mean here what they mean there)
from sydr_amd.dsp.signalsearch import NH10, NH20

SPAN, STEP = 125.0, 5.0
L1 = 1575.42e6


def segment_sums(rf, s0, code, fs, f0, M, S, code_hz=orc.CODE_RATE):
    """Stage 1, sdr_acq_refine's word for word (refine_cases.refine_model) -> (z[M][S], tau[M][S])."""
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
    return z, tau


def search(z, tau, sec, f0, span, step, mode=0):
    """Stage 2 on given segment sums -> (fine_hz, sec_phase, fine_idx, P[Ls][K], X[h*][k*] or 0j)."""
    M = z.shape[0]
    sec = np.asarray(sec, dtype=np.float64)
    Ls = len(sec)
    K = 2 * int(np.floor(span / step)) + 1
    d = (np.arange(K) - (K - 1) // 2) * step
    rot = np.exp(-2j * np.pi * d[None, None, :] * tau[:, :, None])
    per = (z[:, :, None] * rot).sum(axis=1)          # Z[m][k]
    P = np.empty((Ls, K))
    X = np.zeros((Ls, K), complex)
    for h in range(Ls):
        w = sec[(h + np.arange(M)) % Ls]
        if mode == 0:
            X[h] = (w[:, None] * per).sum(axis=0)
            P[h] = np.abs(X[h]) ** 2
        else:
            g = (h + np.arange(M)) // Ls
            P[h] = sum(np.abs((w[g == gg, None] * per[g == gg]).sum(axis=0)) ** 2 for gg in np.unique(g))
    h, k = np.unravel_index(P.argmax(), P.shape)     # first maximum in row-major order
    return f0 + d[k], int(h), int(k), P, complex(X[h, k])


def secondary_model(rf, s0, code, sec, fs, f0, M, S, span=SPAN, step=STEP, mode=0, code_hz=orc.CODE_RATE):
    """-> (fine_hz, sec_phase, fine_idx, P[Ls][K], z[M][S], prompt).  `rf`: complex samples, indexed periodically (a ring)."""
    z, tau = segment_sums(rf, s0, code, fs, f0, M, S, code_hz)
    fine, h, k, P, x = search(z, tau, sec, f0, span, step, mode)
    return fine, h, k, P, z, x


def power_other(P, h):
    return np.delete(P, h, axis=0).max()


_rng = np.random.default_rng(20261021)
SEC25 = (_rng.integers(0, 2, 25) * 2 - 1).astype(np.int8)      # seeded stand-ins, no signal's tables
SEC100 = (_rng.integers(0, 2, 100) * 2 - 1).astype(np.int8)
SEC128 = (np.random.default_rng(20261022).integers(0, 2, 128) * 2 - 1).astype(np.int8)
LONG_CODE = np.random.default_rng(21).integers(0, 2, 4092) * 2.0 - 1.0

CODE_PHASE, PRN, SIGMA = 300.25, 7, 20.0
SATELLITES = ((1, 1630.0, 0), (2, -2381.0, 7), (3, 4120.0, 13), (4, 877.0, 16))     # refine's first four: (seed, dop, later)
FAMILIES = {"A": (NH20, 40, 0, 6.0), "B": (NH10, 40, 1, 6.0), "D": (SEC100, 32, 0, 6.0), "E": (NH20, 12, 0, 8.0)}   # sec, M, mode, amp
LONG = {"C": (5, 1630.0, 50, 4), "C'": (6, -877.0, 30, 2)}                          # seed, dop, M, S
CASE_NAMES = [f + str(i + 1) for f in FAMILIES for i in range(4)] + list(LONG)

_cache = {}


def synth(seed, dop, code, sec, fs, code_hz, code_phase, n, amp, mode, sigma=SIGMA):
    """The recording of the issue: a primary code under a secondary code (mode 1: and a data symbol per secondary period),
    made on the host -> int8 IQ, interleaved."""
    rng = np.random.default_rng(seed)
    L, Ls = len(code), len(sec)
    t = np.arange(n)
    cstep = code_hz * (1 + dop / L1) / fs
    chips = code_phase + t * cstep
    per = np.floor(chips / L).astype(np.int64) + 3
    x = amp * np.asarray(code, dtype=np.float64)[np.floor(chips).astype(np.int64) % L] * np.asarray(sec, dtype=np.float64)[per % Ls]
    if mode == 1:
        data = rng.integers(0, 2, per.max() // Ls + 2) * 2 - 1
        x = x * data[per // Ls]
    x = x * np.exp(2j * np.pi * (dop / fs * t + 0.2))
    x = x + sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    raw = np.empty(2 * n, dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return raw


def window(code_phase, dop, L, fs, code_hz, later, Ls):
    """-> (s0 = the sample a code period begins at, `later` periods behind the first, the secondary chip that period carries)."""
    N = int(np.rint(fs * L / code_hz))
    cstep = code_hz * (1 + dop / L1) / fs
    s0 = int(np.ceil((L - code_phase) / cstep)) + later * N
    return s0, int(np.floor((code_phase + s0 * cstep) / L + 0.5) + 3) % Ls


def make_case(seed, dop, later, code, sec, fs, code_hz, code_phase, M, S, mode, amp, extra_periods=2):
    key = (seed, dop, later, len(code), bytes(np.asarray(sec, dtype=np.int8)), fs, code_hz, code_phase, M, S, mode, amp, extra_periods)
    if key not in _cache:
        L = len(code)
        N = int(np.rint(fs * L / code_hz))
        n = (later + M + extra_periods) * N // 8 * 8
        raw = synth(seed, dop, code, sec, fs, code_hz, code_phase, n, amp, mode)
        s0, phase = window(code_phase, dop, L, fs, code_hz, later, len(sec))
        assert s0 + M * N <= n
        _cache[key] = dict(raw=raw, rf=orc.iq_to_complex(raw), code=np.asarray(code), sec=np.asarray(sec, dtype=np.int8), s0=s0,
                           f0=float(250.0 * np.round(dop / 250.0)), fs=fs, code_hz=code_hz, M=M, S=S, mode=mode, doppler=dop, N=N,
                           true_phase=phase, later=later)
    return _cache[key]


def case(name):
    """A1..A4, B1..B4, D1..D4, E1..E4 (C/A PRN 7 at 4 MHz), C and C' (4092 chips at 4.092 MHz, 25-chip secondary)."""
    if name in LONG:
        seed, dop, M, S = LONG[name]
        c = make_case(seed, dop, 1, LONG_CODE, SEC25, 4.092e6, orc.CODE_RATE, 1000.5, M, S, 0, 8.0)
        assert c["f0"] == {"C": 1750.0, "C'": -1000.0}[name]
        return c
    sec, M, mode, amp = FAMILIES[name[0]]
    seed, dop, later = SATELLITES[int(name[1]) - 1]
    return make_case(seed, dop, later, orc.gold_code(PRN), sec, 4e6, orc.CODE_RATE, CODE_PHASE, M, 4, mode, amp)


_models = {}


def model(name, span=SPAN, step=STEP):
    """secondary_model of a named case, computed once."""
    key = (name, span, step)
    if key not in _models:
        c = case(name)
        _models[key] = secondary_model(c["rf"], c["s0"], c["code"], c["sec"], c["fs"], c["f0"], c["M"], c["S"], span, step, c["mode"],
                                       c["code_hz"])
    return _models[key]


# ---- further inputs of the GPU tests: the edges of the grouping, of the frequency tiles and of a call's batch
SEC2 = np.array([1, -1], dtype=np.int8)
SEC3 = np.array([1, 1, -1], dtype=np.int8)
ROW_B = (np.random.default_rng(20261023).integers(0, 2, 20) * 2 - 1).astype(np.int8)     # a second 20-chip row beside NH20
EXTRA_NAMES = ["M2", "M128", "L3h0", "L3h1", "L3h2", "K1", "K401first", "K401last"]


def extra(name):
    """-> (case, span, step).  M2: M = Ls = 2 (its two hypotheses are each other's negation: P[0] == P[1], and the first
    maximum lies in row 0); M128: M = Ls = 128, S = 16 at N = 2046; L3h*: Ls = 3, M = 7, data mode, partial groups at both
    ends, one window per true phase; K1: one frequency; K401*: 26 frequency tiles with the coarse carrier a whole span off, so
    that the maximum lies in the first / the last tile."""
    code = orc.gold_code(PRN)
    if name == "M2":
        return make_case(1, 1630.0, 0, code, SEC2, 4e6, orc.CODE_RATE, CODE_PHASE, 2, 4, 0, 8.0), SPAN, STEP
    if name == "M128":
        return make_case(7, 1630.0, 0, code, SEC128, 2.046e6, orc.CODE_RATE, CODE_PHASE, 128, 16, 0, 6.0), SPAN, STEP
    if name.startswith("L3h"):
        later = {0: 0, 1: 1, 2: 2}[int(name[3])]
        c = make_case(3, 4120.0, later, code, SEC3, 4e6, orc.CODE_RATE, CODE_PHASE, 7, 4, 1, 8.0, extra_periods=4 - later)
        return c, SPAN, STEP
    if name == "K1":
        return case("A2"), 0.0, STEP
    c = dict(case("A1"))
    c["f0"] = c["doppler"] + (1000.0 if name == "K401first" else -1000.0)
    return c, 1000.0, STEP


def extra_model(name):
    key = ("extra", name)
    if key not in _models:
        c, span, step = extra(name)
        _models[key] = secondary_model(c["rf"], c["s0"], c["code"], c["sec"], c["fs"], c["f0"], c["M"], c["S"], span, step, c["mode"],
                                       c["code_hz"])
    return _models[key]


def batch32():
    """Four recordings (two under NH20, two under ROW_B) behind each other in one ring, eight windows of each, a period apart:
    -> (raw, rf, secs[2][20], [(sec_row, s0, f0)] * 32, M, S), the rows mixed through the list."""
    key = "batch32"
    if key not in _cache:
        code = orc.gold_code(PRN)
        secs = np.stack([NH20, ROW_B])
        raws, items, at = [], [], 0
        for r, (seed, dop, later) in enumerate(SATELLITES):
            row = r % 2
            c = make_case(seed, dop, later, code, secs[row], 4e6, orc.CODE_RATE, CODE_PHASE, 16, 4, 0, 7.0, extra_periods=9)
            raws.append(c["raw"])
            items += [(row, at + c["s0"] + w * c["N"], c["f0"], (c["true_phase"] + w) % 20, dop) for w in range(8)]
            at += c["raw"].size // 2
        order = np.random.default_rng(5).permutation(32)
        raw = np.concatenate(raws)
        _cache[key] = (raw, orc.iq_to_complex(raw), secs, [items[i] for i in order], 16, 4)
    return _cache[key]
