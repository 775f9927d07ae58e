#!/bin/bash
# SQ instruction counters + plain timing of the E/P/L kernel for two builds on one box:
#   tools/pmc_ab.sh <tagA> <libA.so|-> <tagB> <libB.so|->       ("-" = the regular build)
# EXTRA="--epoch-major": further arguments of tools/epl_scaling.py (the list whose epochs share the ring, as the headline's do).
# L2=1: three more passes per build, each a run of its own -- TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum; FETCH_SIZE;
# GRBM_GUI_ACTIVE (/ 8 XCDs / the kernel's time = the clock the build held).  Every counter is summed over the tool's launches
# (--reps 5: six) and printed per wave and as the sum.  A pass that ends non-zero or at its time limit ends the script.
set -u
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$ROOT/gpurun_out/pmc_ab
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
EXTRA=${EXTRA:-}
pass() {
  name=$1; shift
  timeout -k 10 240 rocprofv3 --pmc "$@" --output-format csv -d "$OUT/$tag/$name" -- python3 "$ROOT/tools/epl_scaling.py" --only ${ONLY:-25000} $EXTRA > "$OUT/$tag.$name.log" 2>&1
  rc=$?
  if [ $rc -ne 0 ]; then echo "pass $name of $tag ended with $rc: stopping"; tail -3 "$OUT/$tag.$name.log"; exit $rc; fi
}
one() {
  tag=$1; lib=$2
  if [ "$lib" != "-" ]; then export SYDR_AMD_LIB=$ROOT/$lib; else unset SYDR_AMD_LIB; fi
  timeout -k 10 240 python3 "$ROOT/tools/epl_scaling.py" --only ${ONLY:-25000} --reps 40 $EXTRA > "$OUT/$tag.time.log" 2>&1 || { echo "timing run of $tag failed"; exit 1; }
  pass pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY
  if [ -n "${L2:-}" ]; then
    pass l2 TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum
    pass fetch FETCH_SIZE
    pass grbm GRBM_GUI_ACTIVE
  fi
  python3 - "$OUT/$tag" "$tag" <<'PY'
import sys, glob, csv, collections
acc = collections.defaultdict(float)
for f in glob.glob(sys.argv[1] + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "epl_kernel" in r["Kernel_Name"]:
            acc[r["Counter_Name"]] += float(r["Counter_Value"])
w = acc.get("SQ_WAVES", 1.0)
print(sys.argv[2], "per wave", {k: round(v / w, 2) for k, v in sorted(acc.items())})
print(sys.argv[2], "sums", {k: v for k, v in sorted(acc.items())})
PY
  grep "ms/launch" "$OUT/$tag.time.log"
}
one "$1" "$2"
one "$3" "$4"
[ -n "${L2:-}" ] || one "$1" "$2"
