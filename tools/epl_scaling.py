"""Fixed-vs-proportional cost of epl_kernel: time per workgroup as a function of samples per item.

  --only N          one row of the table (samples per item)
  --reps K          launches per figure
  --xcd-run R[,R..] the "epl_xcd_run" option (runs of R consecutive items per XCD, 0 = linear order); several values: one
                    resident plan, the values alternating, --rounds times -- one line per value and round
  --epoch-major     the items of one epoch read the SAME stretch of the ring, as the channels of the headline's shared stream
                    do (item i: epoch i // 32, channel i % 32); without it every item starts at a random place of a 6.4 MB
                    ring, which no order of the workgroups can make more local"""
import sys, time
import numpy as np
import os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sydr_amd.engine import Engine, make_items, FMT_CI8
e = Engine(0)
if '--no-chip' in sys.argv:
    e.set_option('epl_no_chip_variant', 1)
n_items = 32000
only = int(sys.argv[sys.argv.index('--only') + 1]) if '--only' in sys.argv else None
reps = int(sys.argv[sys.argv.index('--reps') + 1]) if '--reps' in sys.argv else 5
runs = [int(r) for r in sys.argv[sys.argv.index('--xcd-run') + 1].split(',')] if '--xcd-run' in sys.argv else [None]
rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 1
epoch_major = '--epoch-major' in sys.argv
cap = 8 * 400000 if not epoch_major else 8 * (((n_items // 32) * (only or 100000) + 200000) // 8)
e.iq_alloc(cap, FMT_CI8)
e.iq_upload(np.random.default_rng(0).integers(-60, 60, 2 * cap).astype(np.int8), 0)
e.code_slots(32)
for s in range(32):
    e.load_gps_code(s, s + 1)
rng = np.random.default_rng(1)
for n, step in ((3125, 0.32), (6250, 0.16), (10000, 0.1023), (12500, 0.0818), (25000, 0.04092), (50000, 0.02046), (100000, 0.01023)):
    if only and n != only:
        continue
    start = rng.integers(0, cap, n_items)
    if epoch_major:
        start = (np.arange(n_items) // 32) * n + (np.arange(n_items) % 32) * 611        # (a channel's code phase: its own offset)
    items = make_items(np.arange(n_items) % 32, n, start, 1000.0, 0.3, 0.01, step)
    plan = e.epl_plan(items, (-0.5, 0.0, 0.5), 25e6 * 0.04092 / step if step != 0.1023 else 10e6)
    plan.run(); e.sync()
    for rnd in range(rounds):
        for run in runs:
            if run is not None:
                e.set_option('epl_xcd_run', run)
                plan.run(); e.sync()
            e.prof_reset(); e.prof_enable(True)
            for _ in range(reps):
                plan.run()
            ms, cnt = e.prof_read("epl_kernel"); e.prof_enable(False)
            t = ms / cnt
            tag = "" if run is None else f"xcd_run={run:3d} round {rnd + 1}  "
            print(f"{tag}n={n:6d} step={step:.5f} variant={16 if step<=0.06 else (8 if step<=0.125 else 0)}  {t:.4f} ms/launch  {t*1e6/n_items:.1f} ns/WG-slot  {t*1e6/(n_items*n)*1e3:.3f} ps/ch-sample")
    plan.close()
