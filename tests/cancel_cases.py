"""What tests/test_cancel.py (CPU) and tests/test_gpu_cancel.py (MI355X) share: the seeded inputs of sdr_iq_cancel's cases,
the statement's results (sydr_amd/signal/cancel.py: cancel_statement), computed once and read-only, the derived bound and
the margins every integer-ring case must keep from a rounding tie and from a rail."""
import functools

import numpy as np

from oracle import sydr_oracle as orc
from sydr_amd.engine import make_items
from sydr_amd.signal import cancel as cn

PHI = (1.0 + np.sqrt(5.0)) / 2.0
L1 = 1575.42e6
FMT_NAMES = {0: "ci8", 1: "ci16", 2: "cf32", 3: "cf64"}
FMTS = (0, 1, 2, 3)
_RAW = {0: np.int8, 1: np.int16, 2: np.float32, 3: np.float64}
RAIL = {0: 127.0, 1: 32767.0}
# per format: the budget sum_ch |A_ch| of a case and the level of the ring's own samples -- together under the rails
_BUDGET = {0: 25.0, 1: 6000.0, 2: 3.0, 3: 3.0}
_LEVEL = {0: 50, 1: 9000, 2: 1.0, 3: 1.0}


def _chain(slot, n_list, start, carrier_hz, rem_carrier, rem_code, code_step, fs, gaps=None, L=1023):
    """Items of one channel, one after the other: the NCO state carried from epoch to epoch as a tracking loop does
    (rem_code by n * code_step - L chips, rem_carrier by -w * n / fs), `gaps[k]` samples left out in front of epoch k."""
    rows = []
    for k, n in enumerate(n_list):
        start += int(gaps[k]) if gaps is not None else 0
        rows.append((slot, n, start, carrier_hz, rem_carrier, rem_code, code_step))
        start += n
        rem_code = rem_code + n * code_step - L * round(n * code_step / L)
        rem_carrier = float(np.remainder(rem_carrier - carrier_hz * 2.0 * np.pi * n / fs, 2.0 * np.pi))
    return make_items(*[np.array(c) for c in zip(*rows)])


def _pad(items, n_epochs):
    out = np.zeros(n_epochs, dtype=items.dtype)
    out[:len(items)] = items
    out["code_step"][len(items):] = 1.0
    return out


def _unit_amps(n_ch, n_epochs):
    """Irrational (golden-ratio) phases and magnitudes in 1 .. 1 + 0.4 phi, signs flipping like data bits."""
    ch, k = np.meshgrid(np.arange(n_ch), np.arange(n_epochs), indexing="ij")
    mag = 1.0 + ((ch * 7 + k * 3) % 5) * PHI / 10.0
    sign = 1.0 - 2.0 * ((ch + k * k) % 2)
    ang = PHI * (ch + 1) + 0.7 * k
    return np.stack([sign * mag * np.cos(ang), sign * mag * np.sin(ang)], axis=-1)


def _gps(prns):
    return [("gps", int(p)) for p in prns]


def _case_stagger():
    fs, cap, w0 = 4e6, 32768, 20000
    rows = []
    for slot, (n, dop, first) in enumerate(((3999, 2500.0, 0), (4000, -1250.0, 1234), (4001, 4750.0, 2777))):
        step = orc.CODE_RATE * (1.0 + dop / L1) / fs
        rows.append(_chain(slot, [n] * 5, w0 + 100 + first, dop, 0.3 * (slot + 1), 0.1 + 0.2 * slot, step, fs))
    items = np.stack(rows)
    W = 100 + 2777 + 5 * 4001 + 100
    return dict(fs=fs, capacity=cap, w0=w0, W=W, slots=_gps((3, 11, 27)), items=items)


def _case_short():
    fs, cap, w0 = 1e6, 4096, 1001
    rng = np.random.default_rng(20260301)
    code = (rng.integers(0, 2, 31) * 2 - 1).astype(np.int8)
    rows = []
    for ch in range(4):
        real = 40 if ch % 2 == 0 else 37                    # channels 1 and 3: three epochs of trailing padding
        gaps = np.where(rng.random(real) < 0.3, rng.integers(1, 8, real), 0)
        gaps[0] = 3 + 5 * ch
        rows.append(_pad(_chain(0, [62] * real, w0, 1700.0 * (ch + 1), 0.2 * ch, 0.0, 0.5, fs, gaps=gaps, L=31), 40))
    items = np.stack(rows)
    live = items[items["n_samples"] > 0]
    W = int((live["start_sample"] + live["n_samples"]).max()) - w0 + 5
    W += (W % 8 == 0)
    assert W % 8 and w0 % 2 and W <= cap
    return dict(fs=fs, capacity=cap, w0=w0, W=W, slots=[("custom", code)], items=items)


def _case_multi():
    fs, cap, w0 = 4e6, 40960, 7
    step = orc.CODE_RATE * (1.0 + 1500.0 / L1) / fs
    items = _chain(0, [16000, 16000], w0 + 50, 1500.0, 1.0, -0.5, step, fs)[None, :]
    items["rem_code"][0, 0] = -0.5                           # the first index is ceil(-0.5) = 0: (idx - 1) mod L of -1
    return dict(fs=fs, capacity=cap, w0=w0, W=32100, slots=_gps((19,)), items=items)


def _case_many():
    fs, cap, w0 = 4e6, 16384, 12000                          # (crosses the ring's end as well)
    rows = []
    for ch in range(64):
        dop = -5000.0 + 156.25 * ch
        step = orc.CODE_RATE * (1.0 + dop / L1) / fs
        rows.append(_chain(ch, [4000 + ch % 3, 4000 - ch % 2], w0 + 13 * ch, dop, 0.05 * ch, 0.01 * ch, step, fs))
    return dict(fs=fs, capacity=cap, w0=w0, W=9000, slots=_gps([1 + ch % 32 for ch in range(64)]), items=np.stack(rows))


_BUILDERS = {"stagger": _case_stagger, "short": _case_short, "multi": _case_multi, "many": _case_many}
CASES = tuple(sorted(_BUILDERS))


def slot_code(entry):
    kind, what = entry
    return orc.gold_code(what).astype(np.int8) if kind == "gps" else np.asarray(what, dtype=np.int8)


def stage_codes(engine, slots):
    engine.code_slots(max(2, len(slots)))
    for s, (kind, what) in enumerate(slots):
        if kind == "gps":
            engine.load_gps_code(s, what)
        else:
            engine.set_code(s, what)


@functools.lru_cache(maxsize=None)
def geometry(name):
    c = _BUILDERS[name]()
    c["items"].setflags(write=False)
    c["unit_amps"] = _unit_amps(*c["items"].shape)
    return c


def ring_image(name, fmt, seed_extra=0):
    """The whole ring in its storage type (interleaved I, Q), seeded per (case, format)."""
    c = geometry(name)
    rng = np.random.default_rng([20260400 + seed_extra, CASES.index(name), fmt])
    n = 2 * c["capacity"]
    if fmt in RAIL:
        return rng.integers(-_LEVEL[fmt], _LEVEL[fmt] + 1, n).astype(_RAW[fmt])
    return (_LEVEL[fmt] * rng.standard_normal(n)).astype(_RAW[fmt])


def noise_image(n_samples, fmt, seed):
    """A ring of n_samples of seeded values in its storage type (canaries, a destination ring's former content)."""
    rng = np.random.default_rng([20260499, seed, fmt])
    if fmt in RAIL:
        return rng.integers(-_LEVEL[fmt], _LEVEL[fmt] + 1, 2 * n_samples).astype(_RAW[fmt])
    return (_LEVEL[fmt] * rng.standard_normal(2 * n_samples)).astype(_RAW[fmt])


def to_complex(image):
    v = np.asarray(image, dtype=np.float64)
    return v[0::2] + 1j * v[1::2]


def to_image(values, fmt):
    """complex128 values a ring of `fmt` holds exactly -> its storage type, interleaved."""
    out = np.empty(2 * len(values), dtype=_RAW[fmt])
    out[0::2], out[1::2] = values.real, values.imag
    return out


def window_of(ring, w0, W):
    return ring[(w0 + np.arange(W)) % len(ring)]


def amps_of(name, fmt, scale=1.0):
    c = geometry(name)
    return c["unit_amps"] * (scale * _BUDGET[fmt] / (1.0 + 0.4 * PHI) / c["items"].shape[0])


def channels_of(name, amps, order=None):
    c = geometry(name)
    order = range(len(c["items"])) if order is None else order
    return [(c["items"][ch], amps[ch], slot_code(c["slots"][int(c["items"][ch]["code_slot"][0])])) for ch in order]


@functools.lru_cache(maxsize=None)
def statement(name, fmt, scale=1.0):
    """-> (CancelResult of the case in this format, read-only; the ring image it starts from)."""
    c = geometry(name)
    image = ring_image(name, fmt)
    image.setflags(write=False)
    win = window_of(to_complex(image), c["w0"], c["W"])
    res = cn.cancel_statement(win, fmt, channels_of(name, amps_of(name, fmt, scale)), c["fs"], c["w0"], c["capacity"])
    for a in (res.window, res.pre, res.covered):
        a.setflags(write=False)
    return res, image


@functools.lru_cache(maxsize=None)
def bound(name, fmt, scale=1.0):
    """The derived per-component distance the device may keep from the statement (cancel.parity_bound), with the case's
    own sum of |a_re| + |a_im| over the channels (the largest over the epochs), largest |theta| and largest partial sum."""
    c = geometry(name)
    amps = amps_of(name, fmt, scale)
    amp_sum = float(np.abs(amps).sum(axis=-1).max(axis=-1).sum())
    it = c["items"][c["items"]["n_samples"] > 0]
    theta_max = float((np.abs(it["carrier_hz"]) * 2.0 * np.pi * it["n_samples"] / c["fs"] + np.abs(it["rem_carrier"])).max())
    res, image = statement(name, fmt, scale)
    y_max = float(np.abs(to_complex(image)).max()) + amp_sum
    return cn.parity_bound(fmt, amp_sum, theta_max, y_max, len(c["items"]))


def tie_and_rail_margins(name, fmt, scale=1.0):
    """(distance of the nearest covered pre-rounding component from a rounding tie, from a rail's clipping threshold)."""
    res, _ = statement(name, fmt, scale)
    v = np.concatenate([res.pre.real[res.covered], res.pre.imag[res.covered]])
    tie = np.abs(np.abs(v - np.floor(v)) - 0.5).min()
    rail = np.abs(np.abs(v) - (RAIL[fmt] + 0.5)).min()
    return float(tie), float(rail)


RAIL_SCALE = 4.0     # the rails case: `stagger` in ci8 with amplitudes four times the budget


# ------------------------------------------------------------------------------------------------ near-far
# 4 MHz, 10 ms.  PRN A is built from its own items (the statement's replica: what a loop that tracks it perfectly would
# report), amplitude 30 times B's, its data sign flipping between epochs, Doppler +1000 Hz on the search grid (+-5 kHz by
# 250 Hz).  B: Doppler -1750 Hz (bin 27), code start 300.25 chips.  C is absent.  The search: coh = 1, noncoh = 5 from sample 0.
NEAR_FAR = dict(fs=4e6, n=40000, prn_a=5, prn_b=17, prn_c=29, dop_a=1000.0, dop_b=-1750.0, code_start_b=300.25, ratio=30.0,
                R=5000.0, S=250.0, coh=1, noncoh=5)
NEAR_FAR_AMP = {3: 1.0, 0: 3.0}     # B's amplitude: cf64 (noise-free), ci8 (A = 90 LSB, B = 3 LSB)


@functools.lru_cache(maxsize=None)
def near_far(fmt):
    """-> dict(image, items [1][10], slots, truth (bin, code) of B, amps_truth)."""
    c = NEAR_FAR
    fs, n = c["fs"], c["n"]
    b_amp = NEAR_FAR_AMP[fmt]
    step = orc.CODE_RATE * (1.0 + c["dop_a"] / L1) / fs
    items = _chain(0, [4000] * 10, 0, c["dop_a"], 0.4, 0.0, step, fs)[None, :]
    signs = np.array([1, 1, -1, 1, -1, -1, 1, -1, 1, 1], dtype=np.float64)
    a = c["ratio"] * b_amp * signs[:, None] * np.array([np.cos(PHI), np.sin(PHI)])
    x = np.zeros(n, dtype=np.complex128)
    code_a = orc.gold_code(c["prn_a"])
    for it, amp in zip(items[0], a):
        r_re, r_im, _ = cn.replica(it, amp, code_a, fs)
        x[int(it["start_sample"]):int(it["start_sample"]) + 4000] += r_re + 1j * r_im
    nn = np.arange(n, dtype=np.float64)
    chips = (1023 - c["code_start_b"]) + nn * orc.CODE_RATE * (1 + c["dop_b"] / L1) / fs
    x += b_amp * orc.gold_code(c["prn_b"])[np.floor(chips).astype(np.int64) % 1023] * np.exp(2j * np.pi * (c["dop_b"] / fs * nn + 0.1))
    if fmt == 0:
        x = np.clip(np.rint(x.real), -127, 127) + 1j * np.clip(np.rint(x.imag), -127, 127)
    truth = (int(round((-c["dop_b"] + c["R"]) / c["S"])), int(np.ceil(c["code_start_b"] * fs / orc.CODE_RATE)))
    image = to_image(x, fmt)
    image.setflags(write=False)
    return dict(image=image, items=items, slots=_gps((c["prn_a"], c["prn_b"], c["prn_c"])), truth=truth, amps_truth=a[None, :, :])


def oracle_prompt_amps(x, items, codes, fs):
    """amplitudes_from_prompts of the oracle's EPL prompt of every item on the samples x (ring index = array index)."""
    amps = np.zeros(items.shape + (2,))
    for idx in np.ndindex(items.shape):
        it = items[idx]
        n, s = int(it["n_samples"]), int(it["start_sample"])
        if n:
            p = orc.epl(x[s:s + n], orc.pad_code(codes[int(it["code_slot"])]), fs, float(it["carrier_hz"]), float(it["rem_carrier"]),
                        float(it["rem_code"]), float(it["code_step"]), (0.0,))
            amps[idx] = cn.amplitudes_from_prompts(np.array(p), n)
    return amps


def oracle_search(x, prn, c=NEAR_FAR):
    """([bin, code], ratio) of the oracle's PCPS for one PRN over x from sample 0."""
    n_code = orc.samples_per_code(c["fs"])
    m = orc.pcps_map(x[:c["coh"] * c["noncoh"] * n_code], 0.0, c["fs"], orc.code_spectrum(orc.gold_code(prn), c["fs"]), c["R"], c["S"],
                     n_code, c["coh"], c["noncoh"])
    return orc.two_peak_compare(m, n_code, round(c["fs"] / orc.CODE_RATE))


@functools.lru_cache(maxsize=None)
def near_far_expected(fmt):
    """The CPU's verdicts: B and C searched on the original and on the statement's cancelled samples (amplitudes from the
    oracle's prompts).  -> dict(before_b, after_b, before_c, after_c) of ([bin, code], ratio), and the cancelled samples."""
    nf = near_far(fmt)
    c = NEAR_FAR
    x = to_complex(nf["image"])
    codes = [slot_code(s) for s in nf["slots"]]
    amps = oracle_prompt_amps(x, nf["items"], codes, c["fs"])
    res = cn.cancel_statement(x, fmt, [(nf["items"][0], amps[0], codes[0])], c["fs"], 0, len(x))
    return dict(before_b=oracle_search(x, c["prn_b"]), after_b=oracle_search(res.window, c["prn_b"]),
                before_c=oracle_search(x, c["prn_c"]), after_c=oracle_search(res.window, c["prn_c"]), cancelled=res.window,
                amps=amps, stats=res.stats)
