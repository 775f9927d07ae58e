#!/usr/bin/env python3
"""Registers, scratch and occupancy of every epl_kernel instantiation in two sets of compiler assembly, side by side.  No GPU.

  tools/epl_isa_compare.py OLD_DIR NEW_DIR      # each holds epl.s and epl_straight.s (tools/epl_loop_isa.py --keep, or
                                                # `hipcc <the Makefile's flags> --cuda-device-only -S`)

One row per instantiation whose text changed (--all: every one): NumVgprs / ScratchSize / Occupancy old -> new and the
VALU + s_nop count of the round-pair loop's fall-through path (tools/epl_loop_isa.py); the kernels whose instructions are
the same in both are counted.  Exit status 1 if an instantiation lost occupancy or gained scratch."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epl_loop_isa as isa  # noqa: E402

UNITS = ("epl.s", "epl_straight.s")


def kernels(lines):
    """{template arguments: (body lines, resource info)} of every epl_kernel in an assembly file."""
    out = {}
    for l in lines:
        m = re.match(r"(_Z\w*epl_kernelI((?:Li\d+E)+)E\w*):", l)
        if m:
            args = ",".join(re.findall(r"Li(\d+)E", m.group(2)))
            if args not in out:
                out[args] = isa.kernel_body(lines, args)
    return out


def loop_valu(body):
    ins = isa.parse(body)
    at, found = isa.loops(ins)
    cands = []
    for head, back in found:
        if any(head < h and b < back for h, b in found if (h, b) != (head, back)):
            continue
        path = isa.fall_through(ins, at, head, back)
        cands.append((sum(isa.is_valu(op) for op, _ in path), head, sum(op == "s_nop" for op, _ in path)))
    if not cands:
        return None
    top = max(c[0] for c in cands)
    nv, _, nops = sorted((c for c in cands if c[0] >= 0.85 * top), key=lambda c: c[1])[0]   # (as tools/epl_loop_isa.py picks it)
    return nv, nops


def text(body):
    """Instructions alone, labels renumbered away: equal for two compilations of the same kernel."""
    return [(op, re.sub(r"\.L\w+", "L", arg or "")) for _, op, arg in isa.parse(body) if op]


def main():
    show_all = "--all" in sys.argv
    old_dir, new_dir = [a for a in sys.argv[1:] if a != "--all"][:2]
    worse = unchanged = 0
    print("| unit | epl_kernel<...> | VGPRs | scratch | waves | loop VALU + s_nop | text |")
    print("|---|---|---|---|---|---|---|")
    for unit in UNITS:
        old = kernels(open(os.path.join(old_dir, unit)).read().splitlines())
        new = kernels(open(os.path.join(new_dir, unit)).read().splitlines())
        assert sorted(old) == sorted(new), (unit, sorted(set(old) ^ set(new)))
        for args in sorted(old, key=lambda a: [int(x) for x in a.split(",")]):
            (bo, io), (bn, inn) = old[args], new[args]
            same = text(bo) == text(bn)
            lo, ln = loop_valu(bo), loop_valu(bn)
            loop = "-" if lo is None or ln is None else f"{lo[0]} + {lo[1]} -> {ln[0]} + {ln[1]}"
            bad = inn["Occupancy"] < io["Occupancy"] or inn["ScratchSize"] > io["ScratchSize"]
            worse += bad
            unchanged += same
            if same and not bad and not show_all:
                continue
            print(f"| {unit[:-2]} | {args} | {io['NumVgprs']} -> {inn['NumVgprs']} | {io['ScratchSize']} -> {inn['ScratchSize']} | "
                  f"{io['Occupancy']} -> {inn['Occupancy']} | {'same' if same else loop} | {'same' if same else 'changed'}{' WORSE' if bad else ''} |")
    print(f"\n{unchanged} instantiations compile to the same instructions in both.")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main())
