"""bench.py's N > 1 path rehearsed on one GPU: two / four ranks (gloo, all on device 0) generate the SAME 32*N-satellite
stream, each tracks its shard of 32 channels, and rank 0 reports the job.  The driver's own 8-GPU run uses RCCL and
one device per rank; what is checked here is everything else -- the sharding, the reductions and the JSON contract."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 4])     # (a GPU box admits six processes on its card: eight ranks cannot be rehearsed here)
def test_rank_rehearsal_reports_one_self_verified_job(world):
    env = dict(os.environ, SYDR_BENCH_REHEARSE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(29533 + world), os.path.join(REPO, "bench.py"), "--gpus", str(world), "--steps", "3", "--warmup", "1",
           "--stream-seconds", "2.5", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=REPO)   # (the first `import torch` on a fresh box pages the image in: minutes)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1                                  # rank 0 alone prints
    r = json.loads(lines[0])
    assert r["n_gpus"] == world and r["steps"] == 3 and r["scaling"] == "weak"
    assert r["config"]["channels_total"] == 32 * world and r["config"]["channels_per_gpu"] == 32
    assert r["value"] > 0 and r["ms_per_step"] > 0 and r["roofline"]["launches"] == 3   # (one launch per pass over the stream)
    # the job's value counts every rank's channel-samples: `world` times what one rank's stream rate alone would give
    assert r["value"] == pytest.approx(world * r["x_realtime"] * 25.0, rel=2e-3)
    # the run verifies itself: every rank took part, and rank 0 re-tracked four channels of every other rank
    # on its own GPU with bitwise equal accumulators
    m = r["multi_gpu"]
    assert m["ranks_seen"] == world and m["bitwise_identical"] is True
    assert len(m["channels_recomputed_on_rank0"]) == 4 * (world - 1) and all(ok for _, _, ok in m["channels_recomputed_on_rank0"])
    assert sorted({c[0] for c in m["channels_recomputed_on_rank0"]}) == list(range(1, world))
    assert len(m["per_rank_ms_per_step"]) == world and min(m["per_rank_Msamples_per_s"]) > 0
    assert m["distinct_devices"] == 1 and len({d["pid"] for d in m["devices"]}) == world     # (a rehearsal: one card, `world` processes)


def test_gpus_2_without_a_launcher_spawns_its_own_ranks():
    """`python bench.py --gpus 2` started as the driver starts N = 1 (no torchrun): the process becomes the launcher, two
    fresh ranks run the job and rank 0's line reports two GPUs -- never an `n_gpus: 1` line for a `--gpus 2` command."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(SYDR_BENCH_REHEARSE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--stream-seconds", "2.5",
           "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["multi_gpu"]["ranks_seen"] == 2 and r["multi_gpu"]["bitwise_identical"] is True
    assert r["config"]["channels_total"] == 64


def test_more_ranks_than_devices_is_an_error_outside_rehearsal():
    """Two ranks on a one-GPU box without SYDR_BENCH_REHEARSE: every rank refuses (no two ranks on one device, no CPU
    path) and the launcher's exit code is non-zero; nothing is printed as a result line."""
    from sydr_amd._lib import device_count      # (never `import torch` in the test process: it brings its own HIP runtime,
    if device_count() >= 2:                     # and tests that open libamdhip64.so themselves would then talk to that one)
        pytest.skip("this box has two devices")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                              "SYDR_BENCH_REHEARSE")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--stream-seconds", "1"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=REPO)
    assert out.returncode != 0
    assert not [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert "needs 2 MI355X" in out.stderr


def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    """`bench.py --gpus 1` without --full: one line with the headline figures and none of the other legs; --dump-outputs
    writes what the last timed step computed -- float64, within the budget, equal from run to run and equal bit for bit
    to the one-launch pass over the same stream and items."""
    import bench
    from sydr_amd.engine import FMT_CI8, Engine
    dumps = []
    for k in range(2):
        out_dir = tmp_path / f"run{k}"
        cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
               "--stream-seconds", "2.5", "--dump-outputs", str(out_dir)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=REPO)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
        assert len(lines) == 1
        r = json.loads(lines[0])
        assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["value"] > 0 and r["roofline"]["launches"] == 2
        assert r["unit"] == "Msamples/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
        for key in ("cpu_baseline", "acquisition", "closed_loop", "host_fed", "rates", "per_tick", "multignss", "plan_reuse"):
            assert key not in r, key
        names = sorted(os.listdir(out_dir))
        assert names == ["epl_channel_sums.npy", "epl_row_index.npy", "epl_rows.npy"]
        arrays = {n[:-4]: np.load(out_dir / n) for n in names}
        assert all(a.dtype == np.float64 for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= bench.DUMP_MAX_BYTES
        dumps.append(arrays)
    a, b = dumps
    assert all(np.array_equal(a[n], b[n]) for n in a)
    # the same stream and items as bench.py builds them, through ONE plan in this process
    total = int(2.5 * bench.FS) // 8 * 8
    sats = bench.satellites()
    items, n_epochs = bench.truth_items(sats, bench.FS, total)
    eng = Engine(0)
    try:
        eng.iq_alloc(total, FMT_CI8)
        eng.code_slots(bench.N_CH)
        for s, sat in enumerate(sats):
            eng.load_gps_code(s, sat["prn"])
        eng.iq_synth(sats, bench.FS, 12.0, 20260003, 0, total)
        plan = eng.epl_plan(items, bench.SPACING, bench.FS)
        plan.run()
        want = plan.fetch()[:n_epochs * bench.N_CH]
        plan.close()
    finally:
        eng.close()
    assert len(want) <= bench.DUMP_SAMPLE_ROWS                 # (a short stream: every row is written)
    assert np.array_equal(a["epl_row_index"], np.arange(len(want)))
    assert a["epl_rows"].tobytes() == want.tobytes()
    assert np.array_equal(a["epl_channel_sums"], want.reshape(-1, bench.N_CH, want.shape[1]).sum(axis=0))
