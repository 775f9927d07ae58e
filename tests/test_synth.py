"""The statement of the on-device IQ synthesiser (tests/synth_cases.py) on its own: the noise it defines has the moments it
claims, the signal is amp * code * data * carrier, a stream cut into pieces is the stream, and the data bits are those the
full-size closed-loop test expects.  No GPU; tests/test_gpu_synth.py holds sdr_iq_synth to this statement."""
import numpy as np
import pytest

import synth_cases as sc

N_NOISE = 1 << 20


@pytest.fixture(scope="module")
def noise():
    re, im = sc.statement(4e6, 0, N_NOISE, [], sc.SIGMA, sc.SEED)
    return re, im


def test_noise_statistics(noise):
    """Bounds from the distribution, 5 standard errors each: mean sigma / sqrt(N); variance sigma^2 sqrt(2 / N); correlation
    coefficients 1 / sqrt(N).  u1 >= 2^-24 truncates the radius at sigma sqrt(2 ln 2^24) = 5.77 sigma."""
    n, s = N_NOISE, sc.SIGMA
    for x in noise:
        assert abs(x.mean()) <= 5 * s / np.sqrt(n)
        assert abs(x.var() - s * s) <= 5 * s * s * np.sqrt(2.0 / n)
        assert abs(np.mean(x[1:] * x[:-1])) / (s * s) <= 5 / np.sqrt(n)
        assert np.max(np.abs(x)) <= s * np.sqrt(2.0 * np.log(2.0 ** 24)) * (1 + 1e-7)
    re, im = noise
    assert abs(np.mean(re * im)) / (s * s) <= 5 / np.sqrt(n)
    assert np.max(np.hypot(re, im)) > 4.5 * s                    # (the tail is there: P(r > 4.5 sigma) = 4e-5 per sample)


def test_signal_plus_noise_power():
    """Three satellites of amplitudes 8 / 5 / 6 plus sigma = 12: per-axis variance 144 + (64 + 25 + 36) / 2."""
    n = 1 << 19
    re, im = sc.statement(4e6, 0, n, sc.satellites()[:3], sc.SIGMA, sc.SEED)
    want = sc.SIGMA ** 2 + 62.5
    for x in (re, im):
        assert abs(x.var() - want) <= 5 * want * np.sqrt(2.0 / n)


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_signal_model(which):
    """sigma = 0, one satellite: the statement times the conjugate carrier and the code is amp * d(n), and d changes only
    where the code period count passes a multiple of 20 (1023 chips) or of 1 (4092 chips)."""
    fs, n_s = 4e6, 1 << 18
    sat = sc.satellites()[which]
    code = sc.chips_of(sat)
    re, im = sc.statement(fs, 0, n_s, [sat], 0.0, sc.SEED)
    n = np.arange(n_s, dtype=np.int64)
    chip, frac, period, _, _ = sc.sat_geometry(fs, n, sat, len(code))
    cycles = sat["phase"] + n * (sat["doppler"] / fs)
    carrier = np.exp(2j * np.pi * (cycles - np.floor(cycles)))
    c = code[chip].astype(np.float64)
    if sat.get("boc"):
        c = np.where(frac >= 0.5, -c, c)
    d = (re + 1j * im) * np.conj(carrier) * c / sat["amp"]
    assert np.max(np.abs(d.imag)) < 1e-12
    assert np.max(np.abs(np.abs(d.real) - 1.0)) < 1e-12
    d = np.sign(d.real)
    edges = np.flatnonzero(d[1:] != d[:-1]) + 1
    per_bit = 20 if len(code) == 1023 else 1
    assert len(edges) >= (1 if per_bit == 20 else 5)             # (65 ms: three 20 ms bits, or sixteen 4 ms code periods)
    assert np.all(period[edges] != period[edges - 1]) and np.all(period[edges] % per_bit == 0)
    # and the bits are the hash's, keyed by the PRN or by slot + 1000
    ident = sat["slot"] + 1000 if "slot" in sat else sat["prn"]
    assert np.array_equal(d, sc.data_sign(sc.SEED, ident, np.floor(period / per_bit).astype(np.int64)))


def test_negative_code_phase_starts_in_bit_minus_one():
    """Code phase -3.5: period -1, bit index -1, for the first 14 samples at 4 MHz -- with a sign of its own for this seed."""
    sat = sc.satellites()[3]
    _, _, period, bit_index, _ = sc.sat_geometry(4e6, np.arange(30, dtype=np.int64), sat, 1023)
    assert np.array_equal(period[:14], np.full(14, -1.0)) and period[14] == 0 and bit_index[0] == -1 and bit_index[14] == 0
    assert sc.data_sign(sc.SEED, sat["prn"], -1) != sc.data_sign(sc.SEED, sat["prn"], 0)
    boc = sc.case("negative_phase")[4][1]
    assert boc["boc"] and boc["code_phase"] == -0.5              # (sample 0 exactly on the half-chip edge: the flip is ">=")
    chip, frac, period, bit_index, _ = sc.sat_geometry(4e6, np.arange(4, dtype=np.int64), boc, 4092)
    assert chip[0] == 4091 and frac[0] == 0.5 and period[0] == -1 and bit_index[1] == -1 and bit_index[2] == 0
    assert sc.data_sign(sc.SEED, 1000 + sc.BOC_SLOT, -1) != sc.data_sign(sc.SEED, 1000 + sc.BOC_SLOT, 0)


@pytest.mark.parametrize("ft", [np.float64, np.float32])
def test_piecewise_is_the_stream(ft):
    first, a, b = 12345, 257, 100001
    sats = sc.satellites()
    whole = sc.statement(4e6, first, a + b, sats, sc.SIGMA, sc.SEED, ft=ft)
    one = sc.statement(4e6, first, a, sats, sc.SIGMA, sc.SEED, ft=ft)
    two = sc.statement(4e6, first + a, b, sats, sc.SIGMA, sc.SEED, ft=ft)
    for w, p, q in zip(whole, one, two):
        assert w.dtype == ft and np.array_equal(w, np.concatenate([p, q]))


def test_data_signs_are_those_of_the_fullsize_test():
    """tests/test_gpu_fullsize.py expects bit j of PRN p to be mix64(seed ^ mix64(p * 0x100000001B3 + j)) & 1."""
    seed = 20260003
    j = np.arange(3008, dtype=np.uint64)
    for prn in (1, 7, 32, 210):
        sent = (sc.mix64(np.uint64(seed) ^ sc.mix64(np.uint64(prn) * np.uint64(0x100000001B3) + j)) & np.uint64(1)).astype(np.int64)
        assert np.array_equal(2 * sent - 1, sc.data_sign(seed, prn, j.astype(np.int64)))
        assert 0.45 < sent.mean() < 0.55
    # splitmix64's first outputs from state 0 (the published test vector of the generator mix64 finalises)
    states = np.arange(3, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    assert [int(v) for v in sc.mix64(states)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_float32_emulation_is_close_and_integers_nearly_equal():
    """What float32 arithmetic alone costs: the figure the device's float tolerance is a multiple of, and the integer rings
    it implies -- never more than 1 LSB off, in a few values per million."""
    eps = sc.eps_ref()
    print(f"eps_ref = {eps:.3e}")
    assert 2.0 ** -25 < eps < 2.0 ** -20                          # a few float32 roundings of values up to S
    _, fs, first, count, sats, sigma = sc.case("main_4000000")
    re, im = sc.reference("main_4000000")
    re32, im32 = sc.statement(fs, first, count, sats, sigma, sc.SEED, ft=np.float32)
    for fmt in (0, 1):
        worst, share = sc.integer_difference(sc.quantise(re32, im32, fmt), re, im, fmt)
        print(f"{sc.FMT_NAMES[fmt]}: float32 emulation differs in {share:.2e} of the values, by at most {worst}")
        assert worst <= sc.INT_MAX_LSB and share <= sc.INT_MAX_SHARE / 10


def test_quantise():
    re = np.array([0.5, 1.5, 2.5, -0.5, -126.5, 127.4, 127.6, -127.5, -200.0, 4e4, -4e4, 32767.5])
    q8 = sc.quantise(re, -re, 0)
    assert q8.dtype == np.int8 and list(q8[0::2]) == [0, 2, 2, 0, -126, 127, 127, -127, -127, 127, -127, 127]
    assert np.array_equal(q8[1::2], -q8[0::2])
    q16 = sc.quantise(re, -re, 1)
    assert q16.dtype == np.int16 and list(q16[0::2][-3:]) == [32767, -32767, 32767] and q16.min() == -32767
    x = np.array([1.0 + 2.0 ** -30, np.pi])
    assert np.array_equal(sc.quantise(x, x, 3), sc.quantise(x, x, 2).astype(np.float64))
    assert sc.quantise(x, x, 2).dtype == np.float32 and sc.quantise(x, x, 3)[0] == 1.0
