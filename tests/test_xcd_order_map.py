"""The order in which the workgroups of an E/P/L launch take its items (sydr_amd/csrc/xcd_order.h: runs of R consecutive
items per XCD, the device dealing workgroup b to XCD b % 8) -- here a HOST build of the same __host__ __device__ function,
for every run length of the sweep in docs/notes/K1.md and every launch size n = 0 .. 3 * 8 * R + 9:
  - the map is a permutation of [0, n);
  - inside a full tile of 8 * R the ids with the same b % 8 -- one XCD's -- map, in ascending order of b, to ONE contiguous
    ascending run of R items, XCD x to the tile's x-th run;
  - the partial last tile, a launch shorter than a tile and R = 0 keep the linear order."""
import subprocess

import numpy as np
import pytest

import host_check

XCDS = 8
SWEEP = (0, 8, 16, 32, 64, 128)

pytestmark = host_check.requires_hipcc


@pytest.fixture(scope="module")
def exe():
    return host_check.build("xcd_order_dump")


def _maps(exe, R, n_max):
    """[the map of a launch of n workgroups for n = 0 .. n_max]"""
    flat = np.frombuffer(subprocess.check_output([exe, str(R), str(n_max)]), dtype=np.uint32).astype(np.int64)
    assert len(flat) == n_max * (n_max + 1) // 2
    ends = np.cumsum(np.arange(n_max + 1))
    return [flat[ends[n] - n:ends[n]] for n in range(n_max + 1)]


@pytest.mark.parametrize("R", SWEEP)
def test_map_is_a_permutation_with_one_run_per_xcd(exe, R):
    n_max = 3 * XCDS * R + 9
    T = XCDS * R
    for n, m in enumerate(_maps(exe, R, n_max)):
        assert len(m) == n
        assert np.array_equal(np.sort(m), np.arange(n)), (R, n)
        if R == 0 or n < T:
            assert np.array_equal(m, np.arange(n)), (R, n)
            continue
        full = (n // T) * T
        assert np.array_equal(m[full:], np.arange(full, n)), (R, n)          # the partial last tile: linear
        b = np.arange(full)
        for t in range(n // T):
            for x in range(XCDS):
                mine = m[:full][(b // T == t) & (b % XCDS == x)]             # XCD x's workgroups of tile t, in launch order
                assert np.array_equal(mine, t * T + x * R + np.arange(R)), (R, n, t, x)


def test_run_length_zero_is_the_identity_at_any_size(exe):
    for n, m in enumerate(_maps(exe, 0, 300)):
        assert np.array_equal(m, np.arange(n))
