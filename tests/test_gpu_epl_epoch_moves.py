"""What an epoch of the straight-line E/P/L kernels pays once -- how the plan's per-epoch setup (ChipSetup) and the kernel's
arguments reach the registers, how the 2 * NT sums are reduced and stored -- can be rearranged without touching a single
floating-point operation: the same bits along another path.  The bar for such a change is BYTE EQUALITY with what the
commit before it computed (tests/golden/epl_epoch_moves.npz, made by tools/make_epl_epoch_golden.py, which names the commit)
and -- to keep the fixture itself checked -- the oracle at 1e-9 of max(|prompt|, 1), as tests/test_gpu_epl_mask.py holds it.
(docs/notes/K1.md, "What an epoch pays once": reduce_taps_scatter without scratch is held to it, and so were the vector loads
of the setup and the tail read again behind the rounds, which passed and were taken out for their time.)

The lists (tests/epl_epoch_cases.py; rings of seeded NumPy noise through iq_upload) are the smallest at which this code can
go wrong: 64 items at 25 MHz (setups made on the host); 4160 (made by chip_setup_kernel); epochs of 1, 63, 64, 65 and 130
whole chips (rounds = 1, 1, 1, 2, 3: an odd round count, the clamped last round, lanes without a block on the zero replica
words); items on the exact path; epochs that wrap the ring's end or end in its slack (base < 0: the per-sample fallback, which
takes `spacing`, `fs` and constants of its own) and one that starts a ring later; 20 MHz (blocks of 19, direct sums, four waves
per SIMD); five taps at 50 MHz on long replicas (four waves per workgroup, launched as ranges that leave waves without an
item).  Every case asserts the instantiation it ran on."""
import numpy as np
import pytest

import epl_epoch_cases as cases
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("epl_epoch_moves.npz")


def test_the_fixture_names_its_seeds_and_commit(golden):
    assert dict(zip(golden["seed_names"].tolist(), golden["seeds"].tolist())) == cases.SEEDS
    assert len(str(golden["commit"])) >= 7


@pytest.mark.parametrize("name", list(cases.CASES))
def test_bytes_of_the_parent_and_the_oracle(engine, golden, name):
    build, kernel = cases.CASES[name]
    case = build(engine)
    assert case.kernel == kernel, (case.variant, case.kernel)
    assert case.variant == int(golden[name + "_variant"])
    want = golden[name]
    assert case.got.shape == want.shape and case.got.dtype == want.dtype == np.float64
    differ = np.flatnonzero(np.any(case.got.view(np.uint64) != want.view(np.uint64), axis=1))
    err = cases.worst_error(case)
    print(f"{name}: {len(case.items)} items, {len(differ)} rows differ from the recorded bytes (first: {differ[:8].tolist()}), "
          f"worst error against the oracle {err:.3g} ({len(case.which)} rows)")
    assert case.got.tobytes() == want.tobytes()
    assert err <= cases.RTOL
