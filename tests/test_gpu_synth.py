"""sdr_iq_synth on the device against its statement (tests/synth_cases.py), sample by sample: every ring format at two rates,
the formats against each other, the rails, the ring's end and sample numbers beyond it, the cut of a stream into calls, the
calls it refuses, and all 210 Gold codes.  The bounds are those of docs/notes/synth.md: float rings within 8 x eps_ref of the
float64 statement (eps_ref: what ideal float32 arithmetic costs, computed here on the CPU), integer rings never more than
1 LSB off and in at most 1e-4 of their values."""
import numpy as np
import pytest

import synth_cases as sc
from sydr_amd import SdrError

pytestmark = pytest.mark.gpu

FMTS = (0, 1, 2, 3)


def stage(engine, fmt, cap=sc.CAP):
    """A ring of `cap` samples holding the pattern, the 4092-chip code staged in slot BOC_SLOT, slot 1 empty."""
    engine.iq_alloc(cap, fmt)
    engine.iq_upload(sc.pattern(fmt, cap), 0)
    engine.code_slots(2, 4092)
    engine.set_code(sc.BOC_SLOT, sc.staged_code())


def split(raw, first, count, cap=sc.CAP):
    """(the window first .. first + count - 1, everything else) of a whole downloaded ring, both interleaved."""
    inside = np.zeros(cap, dtype=bool)
    idx = (first + np.arange(count)) % cap
    inside[idx] = True
    pairs = raw.reshape(cap, 2)
    return pairs[idx].reshape(-1), pairs[~inside].reshape(-1)


def synthesised(engine, fmt, fs, first, count, sats, sigma, seed=sc.SEED, cap=sc.CAP):
    """The window the device wrote, after checking that it wrote nowhere else."""
    stage(engine, fmt, cap)
    engine.iq_synth(sats, fs, sigma, seed, first, count)
    got, rest = split(engine.iq_download(cap, 0), first, count, cap)
    _, untouched = split(sc.pattern(fmt, cap), first, count, cap)
    assert np.array_equal(rest, untouched), "samples outside the window changed"
    return got


def assert_matches(got, fmt, re, im, sats, sigma, tag):
    if fmt in sc.RAIL:
        worst, share = sc.integer_difference(got, re, im, fmt)
        print(f"{tag} {sc.FMT_NAMES[fmt]}: {share:.3e} of the values differ, by at most {worst} LSB")
        assert worst <= sc.INT_MAX_LSB and share <= sc.INT_MAX_SHARE
    else:
        assert got.dtype == sc.NP_OF_FMT[fmt] and np.all(np.isfinite(got))
        err, eps = sc.float_error(got, re, im, sats, sigma), sc.eps_ref()
        print(f"{tag} {sc.FMT_NAMES[fmt]}: error {err:.3e} of S, eps_ref {eps:.3e}, allowed {sc.FLOAT_MARGIN * eps:.3e}")
        assert err <= sc.FLOAT_MARGIN * eps


@pytest.fixture(scope="module")
def main_rings(engine):
    """The main window in every format at both rates: synthesised once, shared, read-only."""
    out = {}
    for fs in sc.RATES:
        _, _, first, count, sats, sigma = sc.case(f"main_{int(fs)}")
        for fmt in FMTS:
            out[fmt, fs] = synthesised(engine, fmt, fs, first, count, sats, sigma)
            out[fmt, fs].flags.writeable = False
    return out


# ------------------------------------------------------------------------------------------------ against the statement
@pytest.mark.parametrize("fs", sc.RATES)
@pytest.mark.parametrize("fmt", FMTS)
def test_ring_matches_statement(main_rings, fmt, fs):
    """Four satellites (two GPS PRNs, a staged 4092-chip BOC code, one at a negative code phase) under sigma = 12, from sample
    12345 on, a count that leaves the last workgroup partial."""
    name, _, _, _, sats, sigma = sc.case(f"main_{int(fs)}")
    re, im = sc.reference(name)
    assert_matches(main_rings[fmt, fs], fmt, re, im, sats, sigma, name)


@pytest.mark.parametrize("fs", sc.RATES)
def test_formats_agree_bit_for_bit(main_rings, fs):
    """One float32 value per sample, whatever the ring: cf64 is cf32 widened, the integer rings are cf32 rounded to even and
    clipped."""
    cf32 = main_rings[2, fs]
    assert np.array_equal(main_rings[3, fs], cf32.astype(np.float64))
    for fmt in (0, 1):
        assert np.array_equal(main_rings[fmt, fs], sc.quantise(cf32[0::2], cf32[1::2], fmt)), sc.FMT_NAMES[fmt]


@pytest.mark.parametrize("fmt", [0, 1])
def test_rails(engine, fmt):
    """Values beyond the rails stop at +-127 / +-32767 (never -128 / -32768), and as many of them as the statement says.
    (At amplitude 40000 a float32 is 2^-8 wide, so the unclipped ci16 values may round the other way far more often than
    1e-4: there the test holds the values to 1 LSB and to the cf32 ring, and the clipped ones to the statement.)"""
    fs, first, count, sats, sigma = sc.rail_cases()[fmt]
    re, im = sc.statement(fs, first, count, sats, sigma, sc.SEED)
    got = synthesised(engine, fmt, fs, first, count, sats, sigma)
    rail = sc.RAIL[fmt]
    assert got.min() == -rail and got.max() == rail
    want = sc.quantise(re, im, fmt)
    worst, share = sc.integer_difference(got, re, im, fmt)
    clipped, want_clipped = np.abs(got.astype(np.int64)) == rail, np.abs(want.astype(np.int64)) == rail
    print(f"rails {sc.FMT_NAMES[fmt]}: {clipped.mean():.4%} clipped ({want_clipped.mean():.4%} in the statement), "
          f"{share:.3e} of the values differ, by at most {worst} LSB")
    assert want_clipped.mean() > 0.001
    assert worst <= sc.INT_MAX_LSB
    assert np.count_nonzero(clipped != want_clipped) <= sc.INT_MAX_SHARE * got.size
    assert abs(clipped.mean() - want_clipped.mean()) <= sc.INT_MAX_SHARE
    if fmt == 0:
        assert share <= sc.INT_MAX_SHARE
    cf32 = synthesised(engine, 2, fs, first, count, sats, sigma)
    assert np.array_equal(got, sc.quantise(cf32[0::2], cf32[1::2], fmt))


@pytest.mark.parametrize("name", ["ring_end", "beyond", "negative_phase"])
@pytest.mark.parametrize("fmt", FMTS)
def test_ring_end_and_sample_numbers_beyond_it(engine, fmt, name):
    """ring_end: first = capacity - 1000, count = 5000 lands in slots capacity - 1000 .. capacity - 1 and 0 .. 3999; beyond:
    first = 5 * capacity + 77 lands at slot 77 with the signal of sample 5 * capacity + 77; negative_phase: sample 0 lies in
    code period -1 and data bit -1.  Everything outside the window keeps what was uploaded before."""
    _, fs, first, count, sats, sigma = sc.case(name)
    re, im = sc.reference(name)
    assert_matches(synthesised(engine, fmt, fs, first, count, sats, sigma), fmt, re, im, sats, sigma, name)


@pytest.mark.parametrize("fmt", FMTS)
def test_deterministic_in_seed_and_sample_number(engine, fmt):
    """The stream in three calls cut at odd places is the stream in one call, byte for byte; so is the same call again; another
    seed is another stream."""
    _, fs, first, count, sats, sigma = sc.case("main_4000000")
    stage(engine, fmt)
    engine.iq_synth(sats, fs, sigma, sc.SEED, first, count)
    whole = engine.iq_download(sc.CAP, 0)
    engine.iq_synth(sats, fs, sigma, sc.SEED, first, count)
    assert engine.iq_download(sc.CAP, 0).tobytes() == whole.tobytes()
    engine.iq_upload(sc.pattern(fmt), 0)
    a, b = 1, 255
    engine.iq_synth(sats, fs, sigma, sc.SEED, first, a)
    engine.iq_synth(sats, fs, sigma, sc.SEED, first + a, b)
    engine.iq_synth(sats, fs, sigma, sc.SEED, first + a + b, count - a - b)
    assert engine.iq_download(sc.CAP, 0).tobytes() == whole.tobytes()
    engine.iq_synth(sats, fs, sigma, sc.SEED + 1, first, count)
    other = engine.iq_download(sc.CAP, 0)
    differ = np.mean(split(other, first, count)[0] != split(whole, first, count)[0])
    assert differ > (0.9 if fmt else 0.5)          # (another noise stream and other data bits: nearly every value)


@pytest.mark.parametrize("fmt", FMTS)
def test_no_satellites(engine, fmt):
    """No satellites and sigma = 0: zeros.  No satellites and sigma = 12: the statement's noise.  count = 0: nothing."""
    _, fs, first, count, sats, sigma = sc.case("noise_only")
    got = synthesised(engine, fmt, fs, first, count, [], 0.0)
    assert got.dtype == sc.NP_OF_FMT[fmt] and not got.any()
    re, im = sc.reference("noise_only")
    assert_matches(synthesised(engine, fmt, fs, first, count, [], sigma), fmt, re, im, [], sigma, "noise_only")
    before = engine.iq_download(sc.CAP, 0)
    engine.iq_synth(sc.satellites(), fs, sigma, sc.SEED, first, 0)
    assert engine.iq_download(sc.CAP, 0).tobytes() == before.tobytes()


def test_refusals_leave_the_ring_alone(engine):
    fmt, cap = 0, 1 << 12
    stage(engine, fmt, cap)
    ok = dict(doppler=0.0, code_phase=0.0, phase=0.0, amp=5.0)
    good = [dict(ok, prn=7)]
    bad_calls = [([dict(ok, prn=0)], 4e6, 0, 100),
                 ([dict(ok, prn=211)], 4e6, 0, 100),
                 ([dict(ok, prn=7), dict(ok, prn=211)], 4e6, 0, 100),
                 ([dict(ok, slot=1)], 4e6, 0, 100),              # allocated, nothing staged
                 ([dict(ok, slot=2)], 4e6, 0, 100),              # no such slot
                 ([dict(ok, slot=-1)], 4e6, 0, 100),
                 (good, 4e6, 0, cap + 1),
                 (good, 4e6, -1, 100),
                 (good, 0.0, 0, 100),
                 (good, 4e6, 0, -1)]
    for sats, fs, first, count in bad_calls:
        with pytest.raises(SdrError):
            engine.iq_synth(sats, fs, 12.0, sc.SEED, first, count)
        assert np.array_equal(engine.iq_download(cap, 0), sc.pattern(fmt, cap)), (sats, fs, first, count)
    engine.iq_synth(good, 4e6, 12.0, sc.SEED, 0, cap)             # (and the whole ring in one call is no refusal)
    assert not np.array_equal(engine.iq_download(cap, 0), sc.pattern(fmt, cap))


# ------------------------------------------------------------------------------------------------ all 210 Gold codes
def test_every_gold_code_on_device(engine):
    chips = sc.all_gold_codes()
    engine.code_slots(210)
    for prn in range(1, 211):
        engine.load_gps_code(prn - 1, prn)
    for prn in range(1, 211):
        assert np.array_equal(engine.read_code(prn - 1), chips[prn - 1]), f"PRN {prn}"


@pytest.mark.parametrize("prn", [38, 100, 209])
def test_synthesiser_generates_the_gold_code_itself(engine, prn):
    """The synthesiser makes the code of a PRN on its own (no slot is staged): one satellite, no noise, cf32, 2 ms at 4 MHz --
    the ring times the conjugate carrier has the sign of the reference's chip, for every chip of the code."""
    fs, n_s = 4e6, 8000
    sat = dict(prn=prn, doppler=1000.0, code_phase=0.125, phase=0.2, amp=10.0)
    engine.iq_alloc(n_s, 2)
    engine.iq_synth([sat], fs, 0.0, sc.SEED, 0, n_s)
    raw = engine.iq_download(n_s, 0).astype(np.float64)
    chip, _, _, bit_index, cyc = sc.sat_geometry(fs, np.arange(n_s, dtype=np.int64), sat, 1023)
    z = (raw[0::2] + 1j * raw[1::2]) * np.exp(-2j * np.pi * cyc) / sat["amp"]
    assert np.max(np.abs(z.imag)) < 1e-5 and np.max(np.abs(np.abs(z.real) - 1.0)) < 1e-5
    assert set(chip) == set(range(1023))
    want = sc.all_gold_codes()[prn - 1][chip] * sc.data_sign(sc.SEED, prn, bit_index)
    assert np.array_equal(np.sign(z.real), want)
