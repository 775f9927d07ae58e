#!/usr/bin/env python3
"""An int8 / int16 I,Q recording to a packed one of 1, 2 or 4 bits per component (sydr_amd/signal/packing.py), and back.

    python tools/pack_recording.py IN OUT --bits 2 --threshold 12.5            # quantise + pack (int8 in; --int16 for int16)
    python tools/pack_recording.py IN OUT --bits 2 --unpack                    # packed -> int8 of the table's levels
    python tools/pack_recording.py IN OUT --bits 2 --threshold 20 --real       # a REAL int8 / int16 file: every field one sample

Quantising: the table's levels, sorted, are the outputs of a uniform quantiser of step --threshold (2 bits: +-1 below the
threshold in magnitude, +-3 above -- a threshold of one standard deviation of the recording is the textbook choice;
--threshold 0 measures it on the first chunk).  A file whose values are the table's levels already is packed as it is
with --exact.  The file is streamed a chunk at a time; a receiver.ini then names OUT with `data_size = <bits>` (and
`sample_levels` / `bit_order = msb` when --levels / --msb were given).  A real recording packed with --real goes through the
down-converter: `sample_format = packed` beside `decimation`, `is_complex` empty (sydr_amd/signal/iqsource.py)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sydr_amd.signal.packing import Packing, pack, quantise, unpack  # noqa: E402

CHUNK_SAMPLES = 1 << 22       # a multiple of every samples-per-byte


def convert(src, dst, packing, threshold=1.0, int16=False, exact=False, unpack_it=False, chunk=CHUNK_SAMPLES, real=False):
    """-> (samples converted, the threshold used).  real: the file holds one value per sample (a field each), not I,Q pairs."""
    done = 0
    per = 1 if real else 2                 # values of the file per sample
    with open(src, "rb") as fin, open(dst, "wb") as fout:
        while True:
            if unpack_it:
                block = np.fromfile(fin, dtype=np.uint8, count=chunk // packing.samples_per_byte)
                if not block.size:
                    break
                out = unpack(block, packing)
                done += out.size // per
            else:
                block = np.fromfile(fin, dtype=np.int16 if int16 else np.int8, count=2 * chunk)
                if not block.size:
                    break
                if block.size % packing.fields_per_byte:
                    raise SystemExit(f"{src}: {done + block.size // per} samples (and a bit) are not whole bytes at {packing.bits} bit(s)")
                if exact:
                    few = block.astype(np.int8)
                    if not np.array_equal(few, block):
                        raise SystemExit(f"{src}: values outside int8, --exact cannot apply")
                else:
                    if threshold <= 0:
                        threshold = float(block.astype(np.float64).std()) or 1.0
                    few = quantise(block, packing.bits, threshold, packing)
                out = pack(few, packing)
                done += block.size // per
            out.tofile(fout)
    return done, threshold


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src", metavar="IN")
    ap.add_argument("dst", metavar="OUT")
    ap.add_argument("--bits", type=int, required=True, choices=(1, 2, 4))
    ap.add_argument("--threshold", type=float, default=0.0, help="quantiser step in input units (0: the first chunk's standard deviation)")
    ap.add_argument("--levels", help="comma-separated table of 1 << bits int8 levels, written --levels=-3,-1,1,3 (default: the format's)")
    ap.add_argument("--msb", action="store_true", help="first field of a byte in its most significant bits")
    ap.add_argument("--int16", action="store_true", help="IN holds int16 I,Q")
    ap.add_argument("--exact", action="store_true", help="IN holds the table's levels already: pack without quantising")
    ap.add_argument("--unpack", action="store_true", help="IN is packed; OUT receives int8 I,Q of the table's levels")
    ap.add_argument("--real", action="store_true", help="IN holds real samples, one value each: every packed field is one sample")
    args = ap.parse_args(argv)
    levels = [int(v) for v in args.levels.split(",")] if args.levels else None
    packing = Packing(args.bits, levels, msb_first=args.msb)
    n, thr = convert(args.src, args.dst, packing, args.threshold, args.int16, args.exact, args.unpack, real=args.real)
    what = "unpacked" if args.unpack else "packed as it was" if args.exact else f"quantised at {thr:g} and packed"
    print(f"{n} samples {what}: {os.path.getsize(args.src)} -> {os.path.getsize(args.dst)} bytes ({packing})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
