"""What tests/test_corr_profile.py (CPU) and tests/test_gpu_corr_profile.py (MI355X) share: the NumPy statement of
sdr_corr_profile (include/sydr_amd.h) -- the oracle's EPL, unchanged, on the grid first + step * arange(T) -- and the
inputs both run it on.  The CPU file proves on the model that the inputs are fair (one wrong chip of one sample of one tap
shows far above the tolerance), the GPU file holds the device to the model.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from oracle import sydr_oracle as orc

FMT_CI8, FMT_CI16, FMT_CF32, FMT_CF64 = 0, 1, 2, 3
CAP = 1e-9            # of the item's max_j hypot(I_j, Q_j): the project's cap for accumulators
RATES = (4e6, 4.092e6, 10e6, 16.368e6, 25e6, 50e6)
BOUNDS_RATES = (1e6, 2.046e6) + RATES


def grid(first, step, n_taps):
    """s_j exactly as the header states it: one multiply, one add."""
    return first + step * np.arange(n_taps)


def profile_model(rf_ring, code, fs, item, first, step, n_taps):
    """-> [n_taps][2] of one item (slot, n, start, carrier_hz, rem_carrier, rem_code, code_step); `rf_ring`: the ring's
    samples as complex128, indexed modulo its length."""
    _, n, start, f, rc, rk, cstep = item
    x = rf_ring[(int(start) + np.arange(int(n))) % len(rf_ring)]
    out = orc.epl(x, orc.pad_code(np.asarray(code, dtype=np.float64)), fs, f, rc, rk, cstep, grid(first, step, n_taps))
    return np.array(out).reshape(n_taps, 2)


# ---------------------------------------------------------------------------------------------------------- streams
SATS = ((3, 1630.0, 100.5), (7, -2381.0, 300.25), (11, 4120.0, 612.75), (14, 877.0, 17.5),
        (19, -3499.0, 900.0), (22, 2244.0, 455.5), (27, -1113.0, 250.25), (31, 3368.0, 777.0))
REM_CODES = (0.25, -0.3, 0.9999999, 1e-12, 0.0, 0.61803)


def _code_step(fs, dop):
    return orc.CODE_RATE * (1.0 + dop / 1575.42e6) / fs


def _aligned_start(fs, code_phase, dop, rem_code, L=orc.CODE_CHIPS):
    """First sample at which the satellite's code phase has passed `rem_code` chips into a period: an epoch that starts
    there with that rem_code has its prompt tap on the peak (to a sample)."""
    return int(np.ceil((L - code_phase + rem_code) / _code_step(fs, dop)))


def _ring_of(raw, fmt):
    """(the ring's interleaved array in its element type, the same samples as complex128) of int8 / int16 I,Q."""
    if fmt in (FMT_CI8, FMT_CI16):
        return raw, orc.iq_to_complex(raw)
    if fmt == FMT_CF32:     # not whole numbers: every value the float32 it is stored as
        f = raw.astype(np.float32) * np.float32(0.37) + np.float32(0.11)
        return f, f[0::2].astype(np.float64) + 1j * f[1::2].astype(np.float64)
    f = raw.astype(np.float64) * 0.37 + 0.11
    return f, f[0::2] + 1j * f[1::2]


_streams = {}


def _stream(fs, n_sats, amp, sigma, seed, periods, dtype=np.int8):
    key = (fs, n_sats, amp, sigma, seed, periods, np.dtype(dtype).name)
    if key not in _streams:
        N = orc.samples_per_code(fs)
        cap = (periods * N + 7) // 8 * 8
        sats = [dict(prn=p, doppler=d, code_phase=c, phase=0.1 * k, amp=amp) for k, (p, d, c) in enumerate(SATS[:n_sats])]
        _streams[key] = orc.synth_iq(fs, cap, sats, sigma, seed, dtype=dtype)
    return _streams[key]


def _gold_case(name, fs, first, step, n_taps, n_items=4, fmt=FMT_CI8, n_sats=2, amp=20.0, sigma=25.0, seed=1, wrap=False,
               periods=5, max_periods=1):
    dtype = np.int16 if fmt == FMT_CI16 else np.int8
    raw = _stream(fs, n_sats, amp * (100.0 if fmt == FMT_CI16 else 1.0), sigma * (100.0 if fmt == FMT_CI16 else 1.0), seed,
                  periods, dtype)
    ring, rf = _ring_of(raw, fmt)
    cap = len(rf)
    N = orc.samples_per_code(fs)
    items = []
    for k in range(n_items):
        prn, dop, phase = SATS[k % n_sats]
        rk = REM_CODES[k % len(REM_CODES)]
        cstep = _code_step(fs, dop)
        n = orc.required_samples(rk, cstep)
        start = _aligned_start(fs, phase, dop, rk) + ((k // n_sats) % (periods - 3)) * N
        if wrap:    # the window crosses the ring's end (the stream is not continuous there: the model reads the same ring);
            start = cap - n // 3 - 5 * k + (k % 2) * 7 * cap     # some starts revolutions on
        items.append((k % n_sats, n, start, dop + 3.5 * k - 2.0, 0.1 + 0.37 * k, rk, cstep))
    return dict(name=name, fs=fs, fmt=fmt, ring=ring, rf=rf, capacity=cap, codes=[orc.gold_code(p) for p, _, _ in SATS[:n_sats]],
                prns=[p for p, _, _ in SATS[:n_sats]], max_chips=orc.CODE_CHIPS, max_periods=max_periods, items=items,
                first=first, step=step, n_taps=n_taps)


LONG_CHIPS = 4092


def _long_code_case(name, fs, first, step, n_taps, seed=21):
    """A 4092-chip +-1 code at 1.023 Mchip/s: one epoch is 4 ms, four C/A periods' worth of chips."""
    rng = np.random.default_rng(seed)
    code = rng.integers(0, 2, LONG_CHIPS) * 2.0 - 1.0
    dop, phase = 1630.0, 1000.5
    cstep = _code_step(fs, dop)
    N = int(np.rint(fs * LONG_CHIPS / orc.CODE_RATE))
    cap = (3 * N + 7) // 8 * 8
    n = np.arange(cap, dtype=np.float64)
    x = 20.0 * code[np.floor(phase + n * cstep).astype(np.int64) % LONG_CHIPS] * np.exp(2j * np.pi * (dop / fs * n + 0.2))
    x += 25.0 * (rng.standard_normal(cap) + 1j * rng.standard_normal(cap))
    raw = np.empty(2 * cap, dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    items = []
    for k, rk in enumerate((0.25, -0.3)):
        m = int(np.ceil((LONG_CHIPS - rk) / cstep))
        items.append((0, m, _aligned_start(fs, phase, dop, rk, LONG_CHIPS), dop + 1.5 * k, 0.4 * k, rk, cstep))
    return dict(name=name, fs=fs, fmt=FMT_CI8, ring=raw, rf=orc.iq_to_complex(raw), capacity=cap, codes=[code], prns=[None],
                max_chips=LONG_CHIPS, max_periods=1, items=items, first=first, step=step, n_taps=n_taps)


def _exact_phase_case():
    """4.092 MHz: code_step is exactly 1/4, rem_code 0, dyadic spacings -- every fourth sample's phase is a whole number
    (the trap of SURVEY H3: ceil of an exact integer)."""
    fs = 4.092e6
    c = _gold_case("exact_phase_4.092MHz", fs, -2.0, 1.0 / 16, 65, n_items=4, seed=9)
    items = []
    for k, it in enumerate(c["items"]):
        prn, dop, phase = SATS[k % 2]
        cstep = orc.CODE_RATE / fs
        assert cstep == 0.25
        n = orc.required_samples(0.0, cstep)
        items.append((it[0], n, _aligned_start(fs, phase, 0.0, 0.0) + (k // 2) * n, dop, 0.2 * k, 0.0, cstep))
    c["items"] = items
    return c


_cases = None


def parity_cases():
    """Every case the GPU parity test runs (and the CPU fairness test checks): name -> case."""
    global _cases
    if _cases is not None:
        return _cases
    cs = []
    for fs in RATES:                                       # every rate, the usual multi-correlator: +-2 chips at 1/16
        cs.append(_gold_case(f"rate_{fs / 1e6:g}MHz_65", fs, -2.0, 1.0 / 16, 65, seed=2))
    cs.append(_gold_case("taps_1_10MHz", 10e6, 0.25, 0.5, 1, seed=3))
    cs.append(_gold_case("taps_3_10MHz", 10e6, -0.5, 0.5, 3, seed=3))
    cs.append(_gold_case("taps_3_25MHz", 25e6, -0.5, 0.5, 3, seed=3))
    cs.append(_gold_case("taps_129_10MHz", 10e6, -2.0, 1.0 / 32, 129, seed=3))
    cs.append(_gold_case("taps_129_25MHz", 25e6, -2.0, 1.0 / 32, 129, seed=3))
    cs.append(_gold_case("taps_1024_25MHz", 25e6, -8.0, 1.0 / 64, 1024, n_items=2, seed=4))
    cs.append(_gold_case("taps_1024_4MHz", 4e6, -8.0, 1.0 / 64, 1024, n_items=2, seed=4))
    cs.append(_gold_case("grid_pm1_at_1_32_16.368MHz", 16.368e6, -1.0, 1.0 / 32, 65, seed=5))
    cs.append(_gold_case("grid_non_dyadic_16.368MHz", 16.368e6, -1.05, 0.07, 31, seed=5))
    cs.append(_gold_case("grid_non_dyadic_4MHz", 4e6, -1.05, 0.07, 31, seed=5))
    cs.append(_gold_case("grid_negative_step_25MHz", 25e6, 2.0, -1.0 / 16, 65, seed=5))
    cs.append(_gold_case("grid_step_0_10MHz", 10e6, 0.3, 0.0, 5, seed=5))
    for fmt, tag in ((FMT_CI16, "ci16"), (FMT_CF32, "cf32"), (FMT_CF64, "cf64")):
        cs.append(_gold_case(f"fmt_{tag}_25MHz", 25e6, -2.0, 1.0 / 16, 65, fmt=fmt, seed=6))
        cs.append(_gold_case(f"fmt_{tag}_4MHz", 4e6, -2.0, 1.0 / 16, 65, fmt=fmt, seed=6))
    for fmt, tag in ((FMT_CI8, "ci8"), (FMT_CI16, "ci16"), (FMT_CF32, "cf32"), (FMT_CF64, "cf64")):
        cs.append(_gold_case(f"wrap_{tag}_25MHz", 25e6, -2.0, 1.0 / 16, 65, fmt=fmt, seed=7, wrap=True))
    cs.append(_gold_case("wrap_ci8_4MHz", 4e6, -2.0, 1.0 / 16, 65, seed=7, wrap=True))
    # 32 items in one call: eight slots, different starts, carriers and rem_code
    cs.append(_gold_case("items_32_10MHz", 10e6, -2.0, 1.0 / 16, 65, n_items=32, n_sats=8, amp=3.0, sigma=30.0, seed=8, periods=8))
    cs.append(_gold_case("items_32_25MHz", 25e6, -1.0, 1.0 / 8, 17, n_items=32, n_sats=8, amp=3.0, sigma=30.0, seed=8, periods=8))
    cs.append(_long_code_case("long_code_4ms_4.092MHz", 4.092e6, -2.0, 1.0 / 16, 65))
    cs.append(_long_code_case("long_code_4ms_25MHz", 25e6, -2.0, 1.0 / 16, 65))
    cs.append(_gold_case("far_taps_pm40_25MHz", 25e6, -40.0, 1.25, 65, seed=10))      # one staged period, taps 40 chips out
    cs.append(_gold_case("far_taps_pm40_4MHz", 4e6, -40.0, 1.25, 65, seed=10))
    cs.append(_exact_phase_case())
    _cases = {c["name"]: c for c in cs}
    assert len(_cases) == len(cs)
    return _cases


_models = {}


def case_model(case):
    """-> float64[n_items][n_taps][2], cached."""
    if case["name"] not in _models:
        _models[case["name"]] = np.array([profile_model(case["rf"], case["codes"][it[0]], case["fs"], it, case["first"],
                                                        case["step"], case["n_taps"]) for it in case["items"]])
    return _models[case["name"]]


def worst_error(got, ref):
    """Per item: max over taps and I / Q of |got - ref| over the item's max_j hypot(I_j, Q_j).  -> array[n_items]"""
    peak = np.hypot(ref[..., 0], ref[..., 1]).max(axis=1)
    return np.abs(got - ref).reshape(len(ref), -1).max(axis=1) / peak
