"""The block walk of the straight-line correlators (correlator_chip.h: ChipWalk -- a lane carries the first sample S of its
block and the 32-bit fraction f of that boundary, and takes the block's length flag dn, the taps' switch flags ds, the distance
flag dd to its next block and the 2^-16 window test from 32-bit adds onto f and their carries) against the 64-bit formulation
the kernels used before and tests/test_plan_geometry.py holds against the reference's chip indices:

    uS = U + (q - 1) T + 2^32,   S = hi(uS),   dn = hi(uS + T) - S - M,   ds_t = hi(uS + delta_t) - S - m_t,
    dd = S(next round) - S - Dmin,   near = some fraction of uS, uS + T, uS + delta_t within 2^-16 of a sample

A HOST build of the same __host__ __device__ functions walks every lane and round of random epochs of three geometries --
25 MHz and 20 MHz with taps half a chip either side, the half-chip view of 50 MHz with five taps whole (half-)chips apart --
the last round's clamp included, and a grid of crafted fractions (0, 2^32 - 1, both edges of the window).  Every block is
compared, inside the window as well: the walk is integer arithmetic and has to agree everywhere.  Away from the window the
block starts are also the reference's own (oracle: ceil(linspace))."""
import subprocess

import numpy as np
import pytest

import host_check
from oracle import sydr_oracle as orc

NEAR = 1 << 16
TWO32 = 1 << 32
STRIDE = 64

pytestmark = host_check.requires_hipcc


def _exe():
    return host_check.build("chip_walk_dump")


def _near(u):
    return (u + NEAR) % TWO32 < 2 * NEAR


def _items(text):
    items = []
    for line in text.splitlines():
        w = line.split()
        if w[0] == "item":
            it = {}
            for kv in w[1:]:
                k, v = kv.split("=")
                it[k] = float(v) if ("." in v or "e" in v) else int(v)
            it["blocks"] = []
            items.append(it)
        else:
            assert w[0] == "b"
            items[-1]["blocks"].append(tuple(int(x) for x in w[1:]))
    return items


# geometry, block length M, (m of the first and last tap), whole-chip taps, taps in chips, view factor
GEOMETRIES = {"25": (24, 12, False, (-0.5, 0.0, 0.5), 1), "20": (19, 9, False, (-0.5, 0.0, 0.5), 1),
              "50h": (24, None, True, (-1.0, -0.5, 0.0, 0.5, 1.0), 2)}


@pytest.mark.parametrize("geometry", ["25", "20", "50h"])
def test_walk_equals_the_64_bit_line(geometry):
    M, m_tap, whole, spacing, view = GEOMETRIES[geometry]
    items = _items(subprocess.check_output([_exe(), geometry, "24", "2027"], text=True))
    assert len(items) == 24
    checked = clamped = in_window = against_reference = 0
    for it in items:
        T, U, q0, F, Dmin = it["Tfx"], it["Ufx"], it["q0"], it["F"], it["Dmin"]
        assert it["bad"] == 0 and T >> 32 == M and Dmin == (STRIDE * T) >> 32
        deltas = (it["d0"], it["d2"])
        if whole:
            # (a tap a whole number of (half-)chips off switches with the block: at its first sample, or not before its end)
            assert all(m == 0 or m >= M for m in (it["m0"], it["m2"]))
        else:
            assert (it["m0"], it["m2"]) == (m_tap, m_tap)
        rounds = (F + STRIDE - 1) // STRIDE
        assert len(it["blocks"]) == rounds * STRIDE            # every lane, every round
        # the reference's first sample of each chip of the anchor tap
        a = orc.epl_indices(it["n"], it["rem_code"], it["code_step"], spacing[len(spacing) // 2] * view)
        first = {int(q): int(np.searchsorted(a, q, side="left")) for q in range(q0, int(a[-1]) + 2)}
        S_of = {}
        for r, lane, S, dn, ds0, ds2, dd, near, inside in it["blocks"]:
            idx = r * STRIDE + lane
            assert inside == (1 if idx <= F - 1 else 0)
            assert inside or r == rounds - 1                    # only the last round has lanes without a chip
            k = idx if inside else F - 1                        # ... which re-do the last whole chip
            q = q0 + 1 + k
            uS = U + (q - 1) * T + TWO32
            assert S == uS >> 32, (r, lane)
            assert dn == ((uS + T) >> 32) - S - M, (r, lane)
            want_near = _near(uS) or _near(uS + T)
            if whole:
                assert (ds0, ds2) == (0, 0)
            else:
                for ds, d, m in ((ds0, deltas[0], it["m0"]), (ds2, deltas[1], it["m2"])):
                    assert ds == ((uS + d) >> 32) - S - m, (r, lane)
                    want_near = want_near or _near(uS + d)
            assert near == (1 if want_near else 0), (r, lane)
            if r > 0 and inside:
                assert dd == S - S_of[(r - 1, lane)] - Dmin, (r, lane)
            S_of[(r, lane)] = S
            checked += 1
            clamped += 0 if inside else 1
            if want_near:
                in_window += 1
            else:                                               # the prediction must be the reference's own boundary
                assert S == first[q] and S + M + dn == first[q + 1], (q, S, first[q])
                against_reference += 1
    print(f"{geometry}: {checked} blocks, {clamped} clamped, {in_window} inside the 2^-16 window, "
          f"{against_reference} held against the reference")
    assert checked > 20000 and clamped > 0 and against_reference > 20000


def test_crafted_fractions():
    out = subprocess.check_output([_exe(), "crafted"], text=True)
    seen_f, n = set(), 0
    for line in out.splitlines():
        w = line.split()
        assert w[0] == "c"
        f, T_lo, d0, d2, stride_lo, dn, ds0, ds2, near, dd, f_next = (int(x) for x in w[1:])
        # any integer parts do: the flags are the carries out of the low words
        S, Th, dh, Dmin = 1000, 24, 12, 1561
        uS = (S << 32) | f
        assert dn == ((uS + (Th << 32) + T_lo) >> 32) - S - Th
        assert ds0 == ((uS + (dh << 32) + d0) >> 32) - S - dh
        assert ds2 == ((uS + (dh << 32) + d2) >> 32) - S - dh
        assert near == (1 if any(_near(uS + x) for x in (0, T_lo, d0, d2)) else 0)
        u_next = uS + (Dmin << 32) + stride_lo
        assert dd == (u_next >> 32) - S - Dmin and f_next == u_next % TWO32
        seen_f.add(f)
        n += 1
    # zero, all ones, and both edges of the window on either side of a sample
    assert {0, 0xFFFFFFFF, 0xFFFF, 0x10000, 0xFFFF0000, 0xFFFEFFFF} <= seen_f
    assert not _near(0x10000) and _near(0xFFFF) and _near(0xFFFF0000) and not _near(0xFFFEFFFF)
    assert n > 2000
