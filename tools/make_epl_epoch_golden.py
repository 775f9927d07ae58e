#!/usr/bin/env python3
"""Record what THIS build's E/P/L kernels compute for the lists of tests/epl_epoch_cases.py, as the fixture of
tests/test_gpu_epl_epoch_moves.py:

    python tools/make_epl_epoch_golden.py --commit <hash of the checked-out commit> [--out tests/golden/epl_epoch_moves.npz]

The committed tests/golden/epl_epoch_moves.npz was made at commit c621245 ("Test the on-device IQ synthesiser sample by sample
against a statement"), the parent of the change that takes reduce_taps_scatter's slot list out of scratch memory: such a change
moves the same bits along another path, so its outputs must equal the parent's byte for byte.  Make the file again only from a
build whose outputs are meant to become the new reference (a change of the arithmetic, with its own tolerance argument).

The file holds, per list: the fp64 outputs, the plan's variant word; and the seeds of the rings and codes and the commit.  Every
row of every list is held against the oracle (1e-9 of max(|prompt|, 1)) before anything is written.  Needs a GPU."""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the library was built from (recorded in the file)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "epl_epoch_moves.npz"))
    args = ap.parse_args()

    import epl_epoch_cases as cases
    from sydr_amd.engine import Engine

    arrays = {"commit": np.array(args.commit), "seed_names": np.array(sorted(cases.SEEDS)),
              "seeds": np.array([cases.SEEDS[k] for k in sorted(cases.SEEDS)], dtype=np.int64)}
    e = Engine(0)
    try:
        for name, (build, kernel) in cases.CASES.items():
            case = build(e)
            assert case.kernel == kernel, (name, case.variant, case.kernel)
            err = cases.worst_error(case, np.arange(len(case.items)))
            print(f"{name}: {len(case.items)} items, variant {case.variant}, {case.kernel}, worst error against the oracle {err:.3g}", flush=True)
            assert err <= cases.RTOL, name
            arrays[name] = case.got
            arrays[name + "_variant"] = np.array(case.variant, dtype=np.int64)
    finally:
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **arrays)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
