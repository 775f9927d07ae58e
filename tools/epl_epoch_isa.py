#!/usr/bin/env python3
"""Instruction counts of a straight-line E/P/L kernel OUTSIDE its round-pair loop -- what an epoch pays once: the prologue in
front of the loop and the tail behind it -- from the compiler's own assembly.  No GPU.  Beside tools/epl_loop_isa.py, whose
parsing it shares.

  tools/epl_epoch_isa.py                      # the headline kernel epl_kernel<0,3,26,24,1,12,0,0>
  tools/epl_epoch_isa.py 0,5,26,24,4,0,1,0    # a named instantiation
  tools/epl_epoch_isa.py --asm old.s 0,3,26,24,1,12,0,0
  tools/epl_epoch_isa.py --unit epl_straight.hip 0,3,26,19,1,9,0,0

The path of an epoch that the chip-aligned routine covers is taken as the CHEAPEST one (fewest vector instructions) through
the kernel's control flow, in three legs:
  before the loop      kernel entry -> the round-pair loop (tools/epl_loop_isa.py finds it);
  between the copies   a copy's exit -> the next copy in the text, where the compiler laid the loop out more than once (the copy
                       that may clamp, for the epoch's last one or two pairs; the five-tap forms have three); the copies
                       themselves are pairs of the loop and are not counted here;
  after the loop       the last copy's exit -> s_endpgm.
On that walk a branch on the execution mask is never a way round its region (s_cbranch_execz falls through, a forward
s_cbranch_execnz is taken: some lane does the work), a uniform branch (scc / vcc) goes whichever way is cheaper -- which keeps
the walk off the exact re-evaluation near a sample, the epochs of more than 64 edge samples and the per-sample fallback, all of
them behind uniform branches -- and a loop outside the round pairs (the replica's copy to LDS) is passed through once.  The tail
is taken through the edge samples (the only code outside a loop that reads a single ci8 sample, global_load_ushort): every epoch has them.  The
figures therefore compare two builds of one kernel; they are not an exact count of an epoch (SQ_INSTS_VALU is: tools/pmc_ab.sh).

Printed per leg: VALU and SALU, the basic blocks on the path with their VALU, a histogram by opcode, and -- called out -- the
moves (v_mov_b32 / v_mov_b64 / v_accvgpr), the lane reads and writes (v_readlane / v_writelane; v_readfirstlane on its own) and
scratch accesses; then the kernel's NumVgprs / TotalNumSgprs / ScratchSize / Occupancy as the compiler reports them."""
import argparse
import collections
import heapq
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epl_loop_isa as isa  # noqa: E402

DEFAULT = ["0,3,26,24,1,12,0,0"]
MOVES = ("v_mov_b32", "v_mov_b64", "v_accvgpr")
LANES = ("v_readlane", "v_writelane")


def successors(ins, at, i):
    """Where the walk may go from instruction i (see the module's text)."""
    lab, op, arg = ins[i]
    if op is None:
        return [i + 1]
    if op == "s_endpgm":
        return []
    if op == "s_branch":
        t = at.get(arg.strip())
        return [t] if t is not None else [i + 1]
    if op.startswith("s_cbranch"):
        t = at.get(arg.strip())
        if t is None or t <= i:
            return [i + 1]                              # (a loop's backward branch: passed through once)
        if op == "s_cbranch_execz":
            return [i + 1]
        if op == "s_cbranch_execnz":
            return [t]
        return [i + 1, t]
    return [i + 1]


def cheapest(ins, at, sources, is_goal, barred, through=None):
    """Dijkstra over instruction indices by (VALU, instructions); returns the path [indices] or None.  through: a predicate
    some instruction of the path must meet (the state carries whether one has been met)."""
    need = through is not None
    dist, prev, heap = {}, {}, []
    for s in sources:
        node = (s, not need or through(s))
        dist[node] = (0, 0)
        heapq.heappush(heap, ((0, 0), node))
    while heap:
        d, node = heapq.heappop(heap)
        if d != dist.get(node):
            continue
        i, met = node
        if met and is_goal(i):
            path = [node]
            while path[-1] in prev:
                path.append(prev[path[-1]])
            return [n[0] for n in path[::-1]]
        op = ins[i][1]
        nd = (d[0] + (1 if op and isa.is_valu(op) else 0), d[1] + (1 if op else 0))
        for j in successors(ins, at, i):
            if j >= len(ins) or barred(j):
                continue
            nxt = (j, met or through(j))
            if nxt not in dist or nd < dist[nxt]:
                dist[nxt], prev[nxt] = nd, node
                heapq.heappush(heap, (nd, nxt))
    return None


def exits(ins, at, head, back):
    """Targets outside [head, back] of the branches inside it."""
    out = set()
    for i in range(head, back + 1):
        op, arg = ins[i][1], ins[i][2]
        if op and (op.startswith("s_cbranch") or op == "s_branch"):
            t = at.get(arg.strip())
            if t is not None and not head <= t <= back:
                out.add(t)
    if back + 1 < len(ins):
        out.add(back + 1)
    return sorted(out)


def legs(ins):
    at = {lab: i for i, (lab, op, _) in enumerate(ins) if lab}
    by_head = {}
    # (0.8: the five-tap forms' plain copies have 332 - 362 vector instructions where the copy that may clamp has 411; a loop with
    # several backward branches comes once per branch)
    for nv, head, back, path in isa.pair_loops(ins, 0.8):
        first = by_head.setdefault(head, [nv, head, back, path])
        first[2] = max(first[2], back)
    copies = [tuple(c) for c in by_head.values()]
    regions = [(head, back) for _, head, back, _ in copies]
    # the edge samples -- the partial first and last chip, one sample per lane: per-sample arithmetic, which alone reads a
    # single ci8 sample (global_load_ushort) -- lie behind a branch on a lane mask that nothing in the text tells from a way
    # round them: the tail is taken THROUGH them.  (The per-sample fallback reads its samples inside a loop of its own: not meant.)
    _, every_loop = isa.loops(ins)
    every_loop = [(h, b) for h, b in every_loop if not any(h <= h2 and b2 <= b for h2, b2 in every_loop if (h2, b2) != (h, b))]   # innermost
    edge = {i for i, (_, op, _) in enumerate(ins)
            if op and op.startswith("global_load_ushort") and not any(h <= i <= b for h, b in every_loop)}
    inside = lambda r: (lambda i: regions[r][0] <= i <= regions[r][1])  # noqa: E731
    in_any = lambda i: any(h <= i <= b for h, b in regions)            # noqa: E731
    end = lambda i: ins[i][1] == "s_endpgm"                            # noqa: E731
    out = [("before the loop", cheapest(ins, at, [0], inside(0), lambda i: False))]
    for r in range(1, len(regions)):
        gone = regions[:r]
        out.append((f"between copies {r} and {r + 1}", cheapest(ins, at, exits(ins, at, *regions[r - 1]), inside(r),
                                                                 lambda i, gone=gone: any(h <= i <= b for h, b in gone))))
    out.append(("after the loop", cheapest(ins, at, exits(ins, at, *regions[-1]), end, in_any, (lambda i: i in edge) if edge else None)))
    return copies, out


def summary(ins, path):
    """(VALU, SALU, Counter of opcodes, [(block label, VALU)]) of a path; its last index (the goal) is not part of the leg
    unless it ends the program."""
    ops, blocks, label = collections.Counter(), [], "(entry)"
    body = path if ins[path[-1]][1] == "s_endpgm" else path[:-1]
    for i in body:
        lab, op, _ = ins[i]
        if lab:
            label = lab
            continue
        if not blocks or blocks[-1][0] != label:
            blocks.append([label, 0])
        ops[op] += 1
        blocks[-1][1] += 1 if isa.is_valu(op) else 0
    valu = sum(n for op, n in ops.items() if isa.is_valu(op))
    salu = sum(n for op, n in ops.items() if isa.is_salu(op))
    return valu, salu, ops, blocks


def called_out(ops):
    pick = lambda names: {op: n for op, n in sorted(ops.items()) if op.startswith(names)}  # noqa: E731
    moves, lanes = pick(MOVES), pick(LANES)
    return (f"moves {sum(moves.values())} ({', '.join(f'{k} {v}' for k, v in moves.items()) or '-'})   "
            f"lane reads and writes {sum(lanes.values())} ({', '.join(f'{k} {v}' for k, v in lanes.items()) or '-'})   "
            f"v_readfirstlane {sum(pick(('v_readfirstlane',)).values())}   scratch {sum(pick(('scratch_',)).values())}")


def report(asm_lines, args, histogram):
    body, info = isa.kernel_body(asm_lines, args)
    ins = isa.parse(body)
    copies, found = legs(ins)
    print(f"epl_kernel<{args}>  round-pair loop: " + ", ".join(f"{ins[h][0]} ({nv} VALU per pair)" for nv, h, _, _ in copies))
    total_v = total_s = 0
    total_ops = collections.Counter()
    for name, path in found:
        if path is None:
            print(f"  {name}: no path found")
            continue
        valu, salu, ops, blocks = summary(ins, path)
        total_v, total_s = total_v + valu, total_s + salu
        total_ops.update(ops)
        print(f"  {name}: VALU {valu}   SALU {salu}   instructions {sum(ops.values())}")
        print(f"    {called_out(ops)}")
        print("    blocks: " + "  ".join(f"{lab} {nv}" for lab, nv in blocks))
        if histogram:
            for kind, pred in (("VALU", isa.is_valu), ("SALU", isa.is_salu)):
                print(f"    {kind}: " + ", ".join(f"{op} {n}" for op, n in sorted(ops.items(), key=lambda kv: -kv[1]) if pred(op)))
            rest = {op: n for op, n in ops.items() if not isa.is_valu(op) and not isa.is_salu(op)}
            print("    other: " + ", ".join(f"{op} {n}" for op, n in sorted(rest.items(), key=lambda kv: -kv[1])))
    print(f"  outside the loop: VALU {total_v}   SALU {total_s}")
    print(f"    {called_out(total_ops)}")
    print("  " + "  ".join(f"{k}: {info.get(k, '?')}" for k in ("NumVgprs", "TotalNumSgprs", "ScratchSize", "Occupancy")))
    return total_v


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
        isa.compile_asm(a.unit, path)
    lines = open(path).read().splitlines()
    for k in a.kernels:
        report(lines, k, not a.no_histogram)
    return 0


if __name__ == "__main__":
    sys.exit(main())
