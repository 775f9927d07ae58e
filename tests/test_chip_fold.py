"""The folded half-block sums of the straight-line correlators (correlator_chip.h: ChipFold, chip_fold_constants and the
kStatic sample loop) on the CPU.  A half block is summed about the centre of the run of samples that is always summed:
the samples d before and d after it meet conjugate rotations, so a pair costs c (a + b) + 1j s (a - b) with the sums and
differences of the bytes formed by v_perm_b32 / v_dot4_u32_u8 as exact doubles 8448 + (xa + xb), 8447 + (xa - xb); the
optional last sample and an odd run's centre stay single biased samples 4224 + x.

tests/csrc/chip_fold_dump.hip is a HOST build of the plan's constants function and an emulation of one block in the
kernels' own order (integer perm / dot4, fp64 fma, the offsets' shares taken out).  Held against NumPy here:
  * the rotations to 4e-16 (the bound tests/test_plan_geometry.py uses), with the angle rounded as the plan rounds it;
  * the offsets' shares to 1e-10 of their size (likewise);
  * the block sums -- the first half before and with its last sample, the block of KM and of KM + 1 samples, all about the
    first half's centre -- against an evaluation in long double from the integer samples.
Bound of the block sums: every running sum stays below 2^17 (six pairs of at most 8448 + 8447 and two singles of 4224 per
component), so one rounding is at most 2^-37 = 7.3e-12; a component of a block's sum goes through 14 + 12 fused
multiply-adds, two subtractions of shares that were themselves summed in about 28 roundings, and the turn of the second
half (operands below 2^12: 2^-42 each): under 60 roundings, 4.4e-10.  Asserted: 5e-10 absolute, on sums of up to ~3000.

Covered: random bytes and rail bytes (every u = 0 or 255: sums and differences of 0 / 510 before the offset), carriers of
0, +-5 kHz and +-4 MHz at 25 MHz, every (block length, half) the kernels are instantiated for."""
import re
import subprocess

import numpy as np
import pytest

import host_check

FS = 25e6
CARRIERS = (0.0, 5e3, -5e3, 4e6, -4e6)
# (KM, half, taps switching inside the block): the KS forms (KS = KM // 2, half = KS + 1) and the whole-chip-tap forms
FORMS = [(km, km // 2 + 1, 1) for km in range(16, 26)] + [(km, (km + 2) // 2, 0) for km in range(15, 26)]
BLOCK_BOUND = 5e-10

pytestmark = host_check.requires_hipcc


@pytest.fixture(scope="module")
def exe():
    return host_check.build("chip_fold_dump")


def _run(exe, km, half, ks, carrier, mode, n_blocks, seed):
    out = subprocess.check_output([exe, str(km), str(half), str(ks), repr(carrier), repr(FS), mode, str(n_blocks), str(seed)], text=True)
    lines = out.splitlines()
    assert lines[0].startswith("const ")
    const = {k: (int(v) if k in ("n0", "n1") else float(v)) for k, v in re.findall(r"(\w+)=(\S+)", lines[0])}
    blocks = []
    for line in lines[1:]:
        w = line.split()
        assert w[0] == "b"
        u = np.frombuffer(bytes.fromhex(w[1]), dtype=np.uint8).astype(np.int64)
        blocks.append((u, np.array([float(x) for x in w[2:]])))
    assert len(blocks) == n_blocks
    return const, blocks


def _check_constants(const, km, half, ks):
    d = const["dphi"]
    counts = (half - 1 if ks else half, km - half)
    assert (const["n0"], const["n1"]) == counts
    firsts = (0, half)
    shares = []
    for h, count in enumerate(counts):
        re_, im_ = (4224.0, 4224.0) if count % 2 else (0.0, 0.0)
        for i in range(count // 2):
            ang = 0.5 * (count - 1 - 2 * i) * d                      # (the plan's own product: half-integers are exact)
            assert abs(const[f"pc{h}_{i}"] - np.cos(ang)) < 4e-16 and abs(const[f"ps{h}_{i}"] - np.sin(ang)) < 4e-16, (h, i)
            re_ += 8448.0 * np.cos(ang) - 8447.0 * np.sin(ang)
            im_ += 8448.0 * np.cos(ang) + 8447.0 * np.sin(ang)
        ang = -0.5 * (count + 1) * d
        assert abs(const[f"sc{h}"] - np.cos(ang)) < 4e-16 and abs(const[f"ss{h}"] - np.sin(ang)) < 4e-16, h
        shares.append((re_, im_, count // 2 * (8448 + 8447) + (count % 2) * 4224))
        shares.append((re_ + 4224.0 * (np.cos(ang) - np.sin(ang)), im_ + 4224.0 * (np.cos(ang) + np.sin(ang)), shares[-1][2] + 4224))
    for i, (re_, im_, size) in enumerate(shares):
        assert abs(const[f"shc{i}"] - re_) < 1e-10 * size and abs(const[f"shs{i}"] - im_) < 1e-10 * size, i
    turn = firsts[1] + 0.5 * (counts[1] - 1) - 0.5 * (counts[0] - 1)
    assert abs(const["tc"] - np.cos(-turn * d)) < 4e-16 and abs(const["ts"] - np.sin(-turn * d)) < 4e-16


def _exact(u, km, half, ks, dphi):
    """The four sums in long double from the integer samples x = u - 128, about the first half's centre."""
    x = (u[0::2] - 128).astype(np.longdouble) + 1j * (u[1::2] - 128).astype(np.longdouble)
    centre = np.longdouble(0.5) * ((half - 1 if ks else half) - 1)
    ang = -(np.arange(km + 1).astype(np.longdouble) - centre) * np.longdouble(dphi)
    terms = x * (np.cos(ang) + 1j * np.sin(ang))
    n_before = half - 1 if ks else half
    sums = (terms[:n_before].sum(), terms[:half].sum(), terms[:km].sum(), terms[:km + 1].sum())
    return np.array([v for z in sums for v in (z.real, z.imag)], dtype=np.longdouble)


@pytest.mark.parametrize("mode", ["random", "rail"])
def test_folded_block_sums(exe, mode):
    worst = 0.0
    checked = 0
    for km, half, ks in FORMS:
        for c, carrier in enumerate(CARRIERS):
            const, blocks = _run(exe, km, half, ks, carrier, mode, 24, 20260000 + 100 * km + c)
            _check_constants(const, km, half, ks)
            for u, got in blocks:
                assert u.size == 2 * (km + 1)
                if mode == "rail":
                    assert set(np.unique(u)) <= {0, 255}
                err = float(np.max(np.abs(got.astype(np.longdouble) - _exact(u, km, half, ks, const["dphi"]))))
                worst = max(worst, err)
                assert err < BLOCK_BOUND, (km, half, ks, carrier, err)
                checked += 1
    print(f"{mode}: {checked} blocks, worst error of a block sum {worst:.3g}")
    assert checked == len(FORMS) * len(CARRIERS) * 24


def test_rail_blocks_hit_both_extremes(exe):
    """All-low and all-high bytes: every pair's sum is 0 / 510 and its difference 255 before the offsets."""
    const, blocks = _run(exe, 24, 13, 1, 4e6, "rail", 2, 1)
    assert set(np.unique(blocks[0][0])) == {0} and set(np.unique(blocks[1][0])) == {255}
    for u, got in blocks:
        assert np.max(np.abs(got.astype(np.longdouble) - _exact(u, 24, 13, 1, const["dphi"]))) < BLOCK_BOUND
