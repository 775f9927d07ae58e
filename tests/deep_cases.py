"""What tests/test_deep.py (CPU) and tests/test_gpu_deep.py (MI355X) share: the inputs of the deep search's cases, the
statement's results in the form sdr_acq_deep returns them, and the margin every parity case must have.  The statement
itself is the product's plain NumPy text (sydr_amd/dsp/deepsearch.py: deep_map, deep_shift)."""
import functools

import numpy as np

from oracle import sydr_oracle as orc
from sydr_amd.dsp.deepsearch import deep_code_end, deep_map, deep_shift  # noqa: F401  (re-exported)

MARGIN = 1e-6        # the statement's two largest map values must differ by more than this, relative
L1 = 1575.42e6

FMT_NAMES = {0: "ci8", 1: "ci16", 2: "cf32", 3: "cf64"}
_RAW = {0: np.int8, 1: np.int16}


def spc(fs):
    return round(fs / orc.CODE_RATE)


def top2_margin(m):
    """Relative distance of the two largest values of a map."""
    flat = np.asarray(m).reshape(-1)
    i = np.argpartition(flat, -2)[-2:]
    lo, hi = sorted(flat[i])
    return (hi - lo) / hi


def statement_results(m, fs, cfg):
    """(peak_group, peak_bin, peak_code, peak_code_end, peak_value, peak_ratio) of one PRN's statement map [G][bins][N]."""
    G, nbins, N = m.shape
    g, b, n = np.unravel_index(int(np.argmax(m)), m.shape)          # first maximum, row-major (g, b, n)
    peak, ratio = orc.two_peak_compare(m[g], N, spc(fs))
    assert peak == [int(b), int(n)]
    end = deep_code_end(b, n, cfg["R"], cfg["S"], N, cfg["C"], cfg["K"], cfg["rf"])
    return int(g), int(b), int(n), int(end), float(m[g, b, n]), float(ratio)


def statement_maps(rf, fs, if_hz, prns, cfg):
    N = orc.samples_per_code(fs)
    return [deep_map(rf, if_hz, fs, orc.code_spectrum(orc.gold_code(p), fs), cfg["R"], cfg["S"], N, cfg["C"], cfg["K"],
                     cfg["G"], cfg["rf"]) for p in prns]


# ------------------------------------------------------------------------------------------------ parity cases
# name -> fs, ring format, IF, PRNs searched (the first is present), Doppler, code phase, (R, S), C, K, G, carrier_rf_hz,
# ring offset of the window / ring capacity (None: the window starts at 0 in a ring of its size) and engine options.
# Smallest shapes that still take every path: radix passes / register-resident four-step kernels (N = 4000), the 125 x 200
# four-step kernels (N = 25 000: 2 PRNs x 41 bins x C = 2 x K = 4), chirp-z (N = 4006 = 2 x 2003); the four ring formats;
# a window across the ring's end; C in {1, 2, 10, 20} (the fold kernel's compiled period bounds 1, 2, 5, 10, 20: C = 3 runs
# the bound 5 with two idle rounds); (K, G) in {(1,1), (2,2), (3,2), (5,1)}; a one-bin grid; one PRN per inverse sweep and
# the general kernels in place of the register-resident ones.
def _case(fs=4e6, fmt=0, if_hz=0.0, prns=(7, 21), doppler=1750.0, cp=300.25, R=1000.0, S=250.0, C=2, K=3, G=2, rf=0.0,
          start=None, capacity=None, options=()):
    return dict(fs=fs, fmt=fmt, if_hz=if_hz, prns=prns, doppler=doppler, cp=cp, R=R, S=S, C=C, K=K, G=G, rf=rf, start=start,
                capacity=capacity, options=options)


PARITY = {
    "ci8_c2_k3_g2": _case(),
    "ci16_c1_k1_g1": _case(fmt=1, C=1, K=1, G=1, doppler=-750.0, cp=17.5),
    "cf32_c10_k2_g2_l1": _case(fmt=2, C=10, K=2, G=2, rf=L1, doppler=500.0, cp=900.0, if_hz=1000.0),
    "cf64_c20_k5_g1": _case(fmt=3, C=20, K=5, G=1, doppler=-250.0, cp=511.75, R=500.0),
    "ci8_c3_k2_g1": _case(C=3, K=2, G=1, prns=(7,)),
    "wrap": _case(start=20000, capacity=24008, doppler=250.0),
    "n25000": _case(fs=25e6, prns=(5, 30), doppler=-2250.0, cp=100.5, R=5000.0, S=250.0, C=2, K=4, G=2, rf=L1),
    "chirpz_4006": _case(fs=4.006e6, prns=(9,), doppler=250.0, cp=40.0, R=500.0, S=250.0, C=2, K=2, G=1),
    "one_bin": _case(R=0.0, S=250.0, doppler=0.0, C=1, K=2, G=2, prns=(7,)),
    "one_prn_per_sweep": _case(options=(("pcps_prn_chunk", 1),)),
    "general_kernels": _case(options=(("pcps_general_kernels", 1),), C=1, K=2, G=1),
}


@functools.lru_cache(maxsize=None)
def parity_input(name):
    """-> (case, raw ring image in the ring's format, ring capacity, start, the window as complex128)."""
    c = PARITY[name]
    fs, N = c["fs"], orc.samples_per_code(c["fs"])
    n = c["C"] * c["K"] * N
    sats = [dict(prn=c["prns"][0], doppler=c["doppler"], code_phase=c["cp"], phase=0.1, amp=6.0)]
    seed = 20260000 + sorted(PARITY).index(name)
    raw = orc.synth_iq(fs, n, sats, 20.0, seed, dtype=_RAW.get(c["fmt"], np.int16))
    win = orc.iq_to_complex(raw).astype(np.complex128)
    if c["fmt"] == 2:
        win = (win * 0.37).astype(np.complex64).astype(np.complex128)        # (values a float32 ring holds exactly)
    elif c["fmt"] == 3:
        win = win * 0.123456789
    start = c["start"] or 0
    cap = c["capacity"] or (n + 7) // 8 * 8
    assert start + n > cap if c["start"] else True
    ring = np.zeros(cap, dtype=np.complex128)
    ring[(start + np.arange(n)) % cap] = win
    if c["fmt"] in _RAW:
        image = np.empty(2 * cap, dtype=_RAW[c["fmt"]])
        image[0::2], image[1::2] = ring.real, ring.imag
    else:
        image = ring.astype(np.complex64 if c["fmt"] == 2 else np.complex128)
    return c, image, cap, start, win


@functools.lru_cache(maxsize=None)
def parity_statement(name):
    c, _, _, _, win = parity_input(name)
    maps = statement_maps(win, c["fs"], c["if_hz"], c["prns"], c)
    for m in maps:
        m.setflags(write=False)
    return maps


# ------------------------------------------------------------------------------------------------ shifts
# carrier_rf_hz = 1e6 on a 4 MHz grid of +-5000 Hz: q = d * i*C*N / 1e6 = +-400 i samples on the outer bins (C = 20), up to
# +-8000 = two code periods at i = 20: shifts >= N, negative shifts, q = 0 (mod N) at i = 10 and 20.  The input has NO code
# Doppler (a periodic replica), so every block's peak sits at the same n0 and the map's peaks at (n0 - q) mod N: in group 0
# of G = 2 (even i: q mod N = 0, 800, 1600, 2400, 3200, 0, ...) three blocks meet at n0 and two elsewhere.  PRN 7 on
# Doppler -5000 (bin d = +5000, positive shifts) with n0 = 0, PRN 21 on +5000 (negative shifts) with n0 = N - 1.
SHIFT = dict(fs=4e6, if_hz=0.0, prns=(7, 21), R=5000.0, S=2500.0, C=20, K=21, G=2, rf=1e6)


@functools.lru_cache(maxsize=None)
def shift_input():
    c = SHIFT
    fs, N = c["fs"], orc.samples_per_code(c["fs"])
    n = c["C"] * c["K"] * N
    t = np.arange(n)
    rng = np.random.default_rng(20260777)
    x = 4.0 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for prn, dop, n0 in ((7, -5000.0, 0), (21, 5000.0, N - 1)):
        up = orc.upsample_code(orc.gold_code(prn), fs)
        x += 6.0 * up[(t - n0) % N] * np.exp(2j * np.pi * (dop / fs * t + 0.1))
    raw = np.empty(2 * n, dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    return c, raw, orc.iq_to_complex(raw).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def shift_statement():
    c, _, win = shift_input()
    maps = statement_maps(win, c["fs"], c["if_hz"], c["prns"], c)
    for m in maps:
        m.setflags(write=False)
    return maps


# ------------------------------------------------------------------------------------------------ the bit-edge scenario
# 4 MHz, PRN 7, Doppler +4800 Hz, 30 dB-Hz, data alternating every 20 periods, the window starting 5 periods into a bit;
# C = 10, K = 20, +-5 kHz by 50 Hz.  Blocks 1, 3, 5, ... (group 1) hold a bit edge in their middle and cancel; group 0 holds
# none.
BIT_EDGE = dict(fs=4e6, prn=7, doppler=4800.0, cn0=30.0, C=10, K=20, R=5000.0, S=50.0, code_start=1000.25)


def bit_edge_signal(seed=0):
    c = BIT_EDGE
    fs, N = c["fs"], 4000
    n = c["C"] * c["K"] * N
    sigma = 30.0
    amp = sigma * np.sqrt(2 * 10 ** (c["cn0"] / 10) / fs)
    rng = np.random.default_rng(seed)
    nn = np.arange(n, dtype=np.float64)
    code = orc.gold_code(c["prn"])
    chips = (1023 - c["code_start"]) + nn * orc.CODE_RATE * (1 + c["doppler"] / L1) / fs
    per = np.floor(chips / 1023).astype(np.int64)
    idx = np.floor(chips).astype(np.int64) % 1023
    bits = (np.arange(per.max() // 20 + 3) % 2) * 2 - 1
    data = bits[(per + 5) // 20]
    x = amp * code[idx] * data * np.exp(2j * np.pi * (c["doppler"] / fs * nn + 0.1))
    x += sigma * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    true_bin = int(round((-c["doppler"] + c["R"]) / c["S"]))
    true_code = int(np.ceil(c["code_start"] * fs / orc.CODE_RATE))
    return x, true_bin, true_code
