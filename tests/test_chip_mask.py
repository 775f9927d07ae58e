"""The half-block sums of the straight-line correlators with their optional samples masked (correlator_chip.h:
chip_mask_shares and the kStatic sample loop of correlate_epoch_chip) on the CPU.

A block is summed in two halves.  Each has samples that only some lanes sum: the block's sample KM where the lane's block is
M + 1 long (flag dn) and, where the taps switch inside the block (KS), sample KS -- it ends the first half where the lane's
taps switch a sample late (flag sw) and opens the second half otherwise, so that the first half is exactly the taps' part of
the block in front of their switch and the block's sum is first half + second half in every lane.  A lane takes such a
sample's raw dword or 0x80808080 (x = 0) by its flag, each half starts from MINUS the offsets' share of all its samples, and
nothing is captured or selected on the way.

tests/csrc/chip_mask_dump.hip is a HOST build of the shares and an emulation of one block in the kernels' own order (integer
perm / dot4, fp64 fma), folded and direct.  Held here against an evaluation in long double from the integer samples: the
first half's sum `ps` (KS + sw samples; whole-chip taps: the half) and the block's sum `ptot` (KM + dn samples), for all four
flag combinations (whole-chip taps: two) -- i.e. the block with and without each optional sample.

Bound: the one tests/test_chip_fold.py derives for the order with captures, 5e-10 absolute (running sums below 2^17, one
rounding at most 2^-37 = 7.3e-12, under 60 roundings per component of a block's sum).  This order has fewer roundings per
sum, not more: the shares go in once, at the start, instead of being taken out of four sums at the end; the folded KS forms
add one pair (four fused multiply-adds) and two roundings in their second share.

The three-tap forms turn a block's two sums by its phasor once (X = ph ptot, Y = ph ps) and accumulate P, E - P and L - P:
`chip_mask_dump turn` combines a handful of blocks with random flags and random +-1 chips both ways; the recombined E / P / L
agree with the per-tap combination to the bound times the number of blocks (the tap weights are 0 and +-2, exact).

Covered: random bytes and rail bytes, carriers of 0, +-5 kHz and +-4 MHz at 25 MHz, every (block length, half) the kernels
are instantiated for, each both folded and direct (a build chooses per form: chip_folds())."""
import subprocess

import numpy as np
import pytest

import host_check

FS = 25e6
CARRIERS = (0.0, 5e3, -5e3, 4e6, -4e6)
# (KM, half, taps switching inside the block): the KS forms (KS = KM // 2, half = KS + 1) and the whole-chip-tap forms
FORMS = [(km, km // 2 + 1, 1) for km in range(16, 26)] + [(km, (km + 2) // 2, 0) for km in range(15, 26)]
BLOCK_BOUND = 5e-10
N_BLOCKS = 12

pytestmark = host_check.requires_hipcc


@pytest.fixture(scope="module")
def exe():
    return host_check.build("chip_mask_dump")


def _run(exe, km, half, ks, fold, carrier, mode, n_blocks, seed):
    out = subprocess.check_output([exe, str(km), str(half), str(ks), str(fold), repr(carrier), repr(FS), mode, str(n_blocks), str(seed)],
                                  text=True)
    lines = out.splitlines()
    assert lines[0].startswith("const ")
    const = {kv.split("=")[0]: float(kv.split("=")[1]) for kv in lines[0].split()[1:]}
    blocks = []
    for line in lines[1:]:
        w = line.split()
        assert w[0] == "b"
        u = np.frombuffer(bytes.fromhex(w[1]), dtype=np.uint8).astype(np.int64)
        blocks.append((u, np.array([float(x) for x in w[2:]]).reshape(-1, 4)))
    assert len(blocks) == n_blocks
    return const, blocks


def _exact(u, km, half, ks, dphi, ref):
    """[(ps re, ps im, ptot re, ptot im)] per flag combination, in the dump's order, in long double from x = u - 128."""
    x = (u[0::2] - 128).astype(np.longdouble) + 1j * (u[1::2] - 128).astype(np.longdouble)
    ang = -(np.arange(km + 1).astype(np.longdouble) - np.longdouble(ref)) * np.longdouble(dphi)
    terms = x * (np.cos(ang) + 1j * np.sin(ang))
    rows = []
    for sw in ((0, 1) if ks else (0,)):
        for dn in (0, 1):
            ps = terms[:(half - 1 + sw) if ks else half].sum()
            ptot = terms[:km + dn].sum()
            rows.append((ps.real, ps.imag, ptot.real, ptot.imag))
    return np.array(rows, dtype=np.longdouble)


def _check_shares(const, km, half, ks, fold):
    """Each half's share is the sum of its samples' offsets times their rotations, optional samples included."""
    d, ref = const["dphi"], const["ref"]
    if fold:
        n0, n1 = (half - 1 if ks else half), km - half
        assert ref == 0.5 * (n0 - 1)
        c1 = 0.5 * (n0 - 1)                                         # the halves' centres
        c2 = half + 0.5 * (n1 - 1)

        def run(centre, first, count, singles, pairs):
            z = 4224.0 * (1 + 1j) if count % 2 else 0.0
            for i in range(count // 2 + pairs):
                dist = 0.5 * (count - 1) - i + pairs                # (an extra pair lies one step outside the run)
                z += np.cos(dist * d) * 8448.0 * (1 + 1j) + 1j * np.sin(dist * d) * 8447.0 * (1 + 1j)
            for k in singles:
                z += 4224.0 * (1 + 1j) * np.exp(-1j * (k - centre) * d)
            return z
        z1 = run(c1, 0, n0, [half - 1] if ks else [], 0)
        z2 = run(c2, half, n1, [] if ks else [km], 1 if ks else 0)
    else:
        assert ref == 0.0
        z1 = sum(4224.0 * (1 + 1j) * np.exp(-1j * k * d) for k in range(half))
        z2 = sum(4224.0 * (1 + 1j) * np.exp(-1j * j * d) for j in range(-1 if ks else 0, km + 1 - half))
    for got, want in ((const["c1"], z1.real), (const["s1"], z1.imag), (const["c2"], z2.real), (const["s2"], z2.imag)):
        assert abs(got - want) < 1e-10 * 8448 * 2 * 7, (km, half, ks, fold)


@pytest.mark.parametrize("fold", [1, 0], ids=["folded", "direct"])
@pytest.mark.parametrize("mode", ["random", "rail"])
def test_masked_block_sums(exe, mode, fold):
    worst = 0.0
    checked = 0
    for km, half, ks in FORMS:
        for c, carrier in enumerate(CARRIERS):
            const, blocks = _run(exe, km, half, ks, fold, carrier, mode, N_BLOCKS, 20260000 + 100 * km + c)
            _check_shares(const, km, half, ks, fold)
            for u, got in blocks:
                assert u.size == 2 * (km + 1)
                if mode == "rail":
                    assert set(np.unique(u)) <= {0, 255}
                want = _exact(u, km, half, ks, const["dphi"], const["ref"])
                assert got.shape == want.shape == (4 if ks else 2, 4)
                err = float(np.max(np.abs(got.astype(np.longdouble) - want)))
                worst = max(worst, err)
                assert err < BLOCK_BOUND, (km, half, ks, fold, carrier, err)
                checked += 1
    print(f"{mode}, fold={fold}: {checked} blocks, worst error of a sum {worst:.3g}")
    assert checked == len(FORMS) * len(CARRIERS) * N_BLOCKS


def test_optional_samples_matter(exe):
    """The four flag combinations of one block differ by exactly the optional samples (no lane sums a sample twice or drops
    one): ps(sw = 1) - ps(sw = 0) is sample KS, ptot(dn = 1) - ptot(dn = 0) sample KM, and ptot does not depend on sw."""
    km, half = 24, 13
    for fold in (1, 0):
        const, blocks = _run(exe, km, half, 1, fold, 4e6, "random", 8, 7)
        for u, got in blocks:
            x = (u[0::2] - 128) + 1j * (u[1::2] - 128)
            rot = lambda k: np.exp(-1j * (k - const["ref"]) * const["dphi"])
            ps = got[:, 0] + 1j * got[:, 1]
            pt = got[:, 2] + 1j * got[:, 3]                          # rows: (sw, dn) = (0, 0), (0, 1), (1, 0), (1, 1)
            assert abs(ps[2] - ps[0] - x[half - 1] * rot(half - 1)) < 2 * BLOCK_BOUND
            assert abs(pt[1] - pt[0] - x[km] * rot(km)) < 2 * BLOCK_BOUND
            assert abs(pt[2] - pt[0]) < 2 * BLOCK_BOUND and abs(pt[3] - pt[1]) < 2 * BLOCK_BOUND
            assert abs(x[half - 1]) > 0 or abs(x[km]) > 0


@pytest.mark.parametrize("n_blocks", [1, 5, 16])
def test_shared_turn_recombines_to_the_per_tap_combination(exe, n_blocks):
    for c, carrier in enumerate(CARRIERS):
        out = subprocess.check_output([exe, "turn", str(n_blocks), repr(carrier), repr(FS), str(31 + c)], text=True).splitlines()
        direct = np.array([float(x) for x in out[0].split()[1:]])
        turned = np.array([float(x) for x in out[1].split()[1:]])
        assert out[0].startswith("direct") and out[1].startswith("turned") and direct.size == turned.size == 6
        assert np.max(np.abs(direct)) > 1.0
        assert np.max(np.abs(direct - turned)) < BLOCK_BOUND * n_blocks, (n_blocks, carrier, direct, turned)
