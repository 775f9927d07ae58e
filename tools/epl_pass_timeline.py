"""Timeline of the headline's segmented pass from a kernel trace:  where the time outside the epl_kernel launches goes.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --gpus 1 --steps 20 --warmup 5
    SDR_PLAN_TIMING=1 python3 bench.py --gpus 1 --steps 20 --warmup 5 2> plan_timing.txt        (a run of its own, no profiler)
    python3 tools/epl_pass_timeline.py DIR/.../*_kernel_trace.csv --plan-timing plan_timing.txt --steps 20

The timed region is the last steps x segments epl_kernel dispatches of the trace (bench.py's warm-up passes come first).
Printed for it:
  * the gap between the end of each epl_kernel dispatch and the start of the next: median, max, sum per pass;
  * every chip_setup_kernel / validate_items_kernel dispatch against the epl_kernel launch that runs when it starts: start and
    end relative to that launch's start, its duration, and whether it starts and ends INSIDE the launch, runs past its end, or
    lies in the gap behind it; the hardware queue each kind of kernel was dispatched on;
  * every chip_setup_kernel dispatch against the launch that NEEDED it (a plan's creation returns with its setups queued): how
    long before that launch's start, and before the end of the launch in front of it, the setups ended;
  * from the SDR_PLAN_TIMING lines, the median host time of each stage of sdr_epl_plan_create (the last field of a line is
    the wait that ends a creation, or "ready recorded at": the time from the call's begin to the setups being queued).
"""
import argparse
import csv
import re
import statistics as st
from collections import Counter


def load_trace(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?")))
    rows.sort(key=lambda r: r[1])
    return rows


def kind_of(name):
    for k in ("chip_setup_kernel", "chipn_setup_kernel", "validate_items_kernel", "double_items_kernel", "epl_kernel"):
        if k in name:
            return k
    return None


def quantiles(v):
    v = sorted(v)
    return v[0], st.median(v), v[-1]


def timeline(rows, steps, segments):
    epl = [r for r in rows if kind_of(r[0]) == "epl_kernel"]
    n = steps * segments
    if len(epl) < n + 1:
        raise SystemExit(f"the trace holds {len(epl)} epl_kernel dispatches, fewer than the {n} of the timed region plus one before it")
    timed = epl[-n:]
    t_first = timed[0][1]
    dur = [(e - s) * 1e-6 for _, s, e, _ in timed]
    print(f"timed region: {n} epl_kernel dispatches ({steps} passes x {segments} segments), queue(s) {dict(Counter(q for *_, q in timed))}")
    print("  epl_kernel duration ms: min %.4f median %.4f max %.4f" % quantiles(dur))
    gaps = [(timed[i + 1][1] - timed[i][2]) * 1e-6 for i in range(n - 1)]
    per_pass = [sum(gaps[p * segments:(p + 1) * segments]) for p in range(steps - 1)]   # (a pass's 12 gaps: the one into the next pass included)
    print("  gap end -> next start ms: min %.4f median %.4f max %.4f" % quantiles(gaps))
    print("  gaps per pass ms: min %.4f median %.4f max %.4f" % quantiles(per_pass))
    span = (timed[-1][2] - t_first) * 1e-6 / steps
    print(f"  first start -> last end: {span:.4f} ms per pass; launches {sum(dur) / steps:.4f} ms per pass; "
          f"outside the launches {span - sum(dur) / steps:.4f} ms per pass")
    for kind in ("validate_items_kernel", "chip_setup_kernel", "chipn_setup_kernel", "double_items_kernel"):
        ks = [r for r in rows if kind_of(r[0]) == kind and r[1] >= t_first]
        if not ks:
            continue
        where, rel_s, rel_e, d, late = Counter(), [], [], [], []
        j = 0
        for _, s, e, _ in ks:
            while j + 1 < n and timed[j + 1][1] <= s:
                j += 1
            ls, le = timed[j][1], timed[j][2]
            d.append((e - s) * 1e-6)
            if s >= le:
                where["in the gap behind the launch"] += 1
                late.append((s - le) * 1e-6)
                continue
            where["inside the launch" if e <= le else "starts inside, ends behind the launch"] += 1
            rel_s.append((s - ls) * 1e-6)
            rel_e.append((e - ls) * 1e-6)
        print(f"{kind}: {len(ks)} dispatches, queue(s) {dict(Counter(q for *_, q in ks))}: {dict(where)}")
        print("  duration ms: min %.4f median %.4f max %.4f" % quantiles(d))
        if rel_s:
            print("  start after the launch's start ms: min %.4f median %.4f max %.4f" % quantiles(rel_s))
            print("  end after the launch's start ms:   min %.4f median %.4f max %.4f" % quantiles(rel_e))
        if late:
            print("  (those in the gap) start after the launch's end ms: min %.4f median %.4f max %.4f" % quantiles(late))
    setups_against_their_launch(rows, epl, n)


def setups_against_their_launch(rows, epl, n):
    """A plan has one chip_setup_kernel dispatch and, in the headline's passes, one launch: counted from the trace's end the
    m-th setup belongs to the m-th epl_kernel dispatch, which reads what it wrote.  Per segment of the timed region: how long
    before that launch's START the setups ended (negative: the launch had to wait for them), and how long before the END of
    the launch in front of it (positive: they were done while that one still ran, so the next could follow it at once)."""
    setups = [r for r in rows if kind_of(r[0]) == "chip_setup_kernel"]
    m = min(n, len(setups), len(epl) - 1)
    if m == 0:
        return
    pairs = list(zip(setups[-m:], epl[-m:], epl[-m - 1:-1]))
    if any(su[1] > mine[1] for su, mine, _ in pairs):
        print("chip_setup_kernel against the launch that needed it: the dispatches do not pair one to one from the trace's end "
              "(a setup starts after its launch); not printed")
        return
    before_start = [(mine[1] - su[2]) * 1e-6 for su, mine, _ in pairs]
    before_prev_end = [(prev[2] - su[2]) * 1e-6 for su, _, prev in pairs]
    inside = sum(1 for v in before_prev_end if v >= 0)
    print(f"chip_setup_kernel against the launch that needed it ({m} segments):")
    print("  ended before that launch's start ms:            min %.4f median %.4f max %.4f" % quantiles(before_start))
    print("  ended before the end of the launch in front ms: min %.4f median %.4f max %.4f" % quantiles(before_prev_end))
    print(f"  done while the launch in front still ran: {inside} of {m}")


def plan_timing(path, n):
    stages = {}
    lines = [ln for ln in open(path) if ln.startswith("plan_create ")]
    for ln in lines[-n:]:
        for piece in ln.split(":", 1)[1].split(","):
            m = re.match(r"\s*(.+?)\s+(-?[0-9.]+)(?: ms)?\s*$", piece)
            if m:
                stages.setdefault(m.group(1), []).append(float(m.group(2)))
    print(f"sdr_epl_plan_create, host time per stage over the last {min(n, len(lines))} plans (ms):")
    total = 0.0
    for k, v in stages.items():
        lo, med, hi = quantiles(v)
        if k != "ready recorded at":      # (counted from the call's begin: the stages before it over again)
            total += med
        print(f"  {k:28s} min {lo:.3f} median {med:.3f} max {hi:.3f}")
    print(f"  sum of medians {total:.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", help="rocprofv3 kernel-trace CSV of a bench.py run")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--segments", type=int, default=12)
    ap.add_argument("--plan-timing", default=None, help="stderr of a run with SDR_PLAN_TIMING=1")
    a = ap.parse_args()
    timeline(load_trace(a.trace), a.steps, a.segments)
    if a.plan_timing:
        plan_timing(a.plan_timing, a.steps * a.segments)


if __name__ == "__main__":
    main()
