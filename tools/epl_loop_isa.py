#!/usr/bin/env python3
"""Instruction counts of the round-pair loop of a straight-line E/P/L kernel, from the compiler's own assembly.  No GPU.

  tools/epl_loop_isa.py                      # the headline kernel epl_kernel<0,3,26,24,1,12,0,0> and the multignss one
  tools/epl_loop_isa.py 0,5,26,24,4,0,1,0    # a named instantiation (the template arguments, comma separated)
  tools/epl_loop_isa.py --asm old.s 0,3,26,24,1,12,0,0        # count in an assembly file made earlier
  tools/epl_loop_isa.py --unit epl_straight.hip 0,3,26,19,1,9,0,0

Compiles sydr_amd/csrc/<unit> to gfx950 assembly with the Makefile's flags (`--cuda-device-only -S`, about a minute), takes
the kernel's innermost loop with the most vector instructions -- the loop over pairs of rounds of correlate_epoch_chip; where
the last rounds are peeled off it, the first of the two copies -- and walks its FALL-THROUGH path from the loop's label to its backward branch: a conditional forward branch is not taken (the
exact re-evaluation of a block near a sample sits behind one), an unconditional one is followed.  Printed: VALU and SALU
per pair of blocks with a histogram by opcode, v_readlane / v_writelane and s_nop on the path, and the kernel's
NumVgprs / ScratchSize / Occupancy / code length as the compiler reports them."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "sydr_amd", "csrc")
DEFAULT = ["0,3,26,24,1,12,0,0", "0,5,26,24,4,0,1,0"]


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def compile_asm(unit, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, *makefile_flags(), "--cuda-device-only", "-S", os.path.join(CSRC, unit), "-o", out])


def kernel_body(lines, args):
    """The lines of epl_kernel<args> (label to .Lfunc_end) and its trailing resource comments."""
    mangled = "epl_kernelI" + "".join(f"Li{a}E" for a in args.split(",")) + "E"
    start = next((i for i, l in enumerate(lines) if l.startswith("_Z") and mangled in l.split(":")[0] and l.rstrip().find(":") > 0), None)
    if start is None:
        raise SystemExit(f"no epl_kernel<{args}> in this assembly")
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    info = {}
    for l in lines[end:end + 60]:
        m = re.match(r"\s*;\s*(NumVgprs|TotalNumSgprs|ScratchSize|Occupancy|codeLenInByte)\s*[:=]\s*(\d+)", l)
        if m and m.group(1) not in info:
            info[m.group(1)] = int(m.group(2))
    return lines[start + 1:end], info


def parse(body):
    """[(label or None, opcode, operands)] without directives and comments."""
    out = []
    for l in body:
        l = l.split(";")[0].strip()
        if not l or l.startswith("."):
            m = re.match(r"(\.LBB\d+_\d+):", l)
            if m:
                out.append((m.group(1), None, None))
            continue
        parts = l.split(None, 1)
        out.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def is_valu(op):
    return op.startswith("v_") and not op.startswith("v_nop")


def is_salu(op):
    return op.startswith("s_") and not op.startswith(("s_nop", "s_waitcnt", "s_barrier", "s_endpgm", "s_load", "s_buffer_load"))


def loops(ins):
    """(header index, back-branch index) of every backward branch."""
    at = {lab: i for i, (lab, op, _) in enumerate(ins) if lab}
    found = []
    for i, (lab, op, arg) in enumerate(ins):
        if op and (op.startswith("s_cbranch") or op == "s_branch"):
            t = at.get(arg.strip())
            if t is not None and t < i:
                found.append((t, i))
    return at, found


def fall_through(ins, at, head, back):
    path, i, steps = [], head, 0
    while i != back and steps < 200000:
        lab, op, arg = ins[i]
        steps += 1
        if op:
            path.append((op, arg))
            if op == "s_branch":
                t = at.get(arg.strip())
                if t is not None and head <= t <= back and t > i:
                    i = t
                    continue
        i += 1
    path.append((ins[back][1], ins[back][2]))
    return path


def pair_loops(ins, share=0.85):
    """The copies of the round-pair loop, in the order of the text: [(VALU on the fall-through path, header index, back-branch
    index, path)] of every innermost loop with at least `share` of the largest one's vector instructions."""
    at, found = loops(ins)
    cands = []
    for head, back in found:
        if any(head < h and b < back for h, b in found if (h, b) != (head, back)):
            continue                                   # not innermost
        path = fall_through(ins, at, head, back)
        cands.append((sum(is_valu(op) for op, _ in path), head, back, path))
    if not cands:
        raise SystemExit("no loop found")
    # the pair loop comes twice where the last rounds are peeled off it: first the plain one (all but the last two or three
    # rounds of an epoch), then the one that can clamp (run once or twice per epoch) -- the first is the one that counts
    top = max(c[0] for c in cands)
    return sorted((c for c in cands if c[0] >= share * top), key=lambda c: c[1])


def report(asm_lines, args, histogram):
    body, info = kernel_body(asm_lines, args)
    ins = parse(body)
    nv, head, _, path = pair_loops(ins)[0]
    ops = collections.Counter(op for op, _ in path)
    lanes = sum(n for op, n in ops.items() if op.startswith(("v_readlane", "v_writelane")))
    print(f"epl_kernel<{args}>  loop {ins[head][0]}")
    print(f"  VALU per pair of blocks: {nv}   SALU: {sum(n for op, n in ops.items() if is_salu(op))}   "
          f"v_readlane/v_writelane: {lanes}   s_nop: {ops.get('s_nop', 0)}   instructions on the path: {len(path)}")
    print("  " + "  ".join(f"{k}: {info.get(k, '?')}" for k in ("NumVgprs", "TotalNumSgprs", "ScratchSize", "Occupancy", "codeLenInByte")))
    if histogram:
        for kind, pred in (("VALU", is_valu), ("SALU", is_salu)):
            print(f"  {kind}: " + ", ".join(f"{op} {n}" for op, n in sorted(ops.items(), key=lambda kv: -kv[1]) if pred(op)))
        rest = {op: n for op, n in ops.items() if not is_valu(op) and not is_salu(op)}
        print("  other: " + ", ".join(f"{op} {n}" for op, n in sorted(rest.items(), key=lambda kv: -kv[1])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernels", nargs="*", default=DEFAULT, help="template arguments of epl_kernel, e.g. 0,3,26,24,1,12,0,0")
    ap.add_argument("--unit", default="epl.hip", help="translation unit under sydr_amd/csrc (default epl.hip)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly under this name")
    ap.add_argument("--no-histogram", action="store_true")
    a = ap.parse_args()
    if a.asm:
        path = a.asm
    else:
        path = a.keep or os.path.join(tempfile.mkdtemp(prefix="epl_isa_"), "unit.s")
        compile_asm(a.unit, path)
    lines = open(path).read().splitlines()
    for k in a.kernels:
        report(lines, k, not a.no_histogram)
    return 0


if __name__ == "__main__":
    sys.exit(main())
