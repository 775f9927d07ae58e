"""The lock role of the closed-loop kernel (track_kernel.h: PULL_IN / WIDE / NARROW, the bandwidth and tap hand-over,
CODE_LOCK by C/N0, BIT_SYNC, the 20-prompt bit decision) against the oracle, per epoch, over every edge of the state
machine and in every kernel form.

The cases are the seeded starts of tests/lock_edge_cases.py (the oracle's branches they take are pinned to the reference by
g6d_kaplan_edges.npz).  All cases of a rate run as channels of ONE launch with per-channel states and configurations, on a
stream the device synthesises; the oracle runs on the download, once per rate.  Integers, flags and bits must be equal;
correlators and loop quantities agree to RTOL = 1e-9 (tests/test_gpu_tracking.py's, with its scales); the end state is
compared field by field.  `track_replay.classify` proves which correlator core each (rate, form) ran on.  `-s` prints
the worst device-to-oracle ratio per quantity, rate and form (docs/notes/parity.md quotes them)."""
import concurrent.futures

import numpy as np
import pytest

import lock_edge_cases as lec
import track_replay as tr
from conftest import load_golden
from oracle import sydr_oracle as orc
from test_gpu_multignss import FIVE, general_cfg
from test_gpu_tracking import RTOL, loop_cfg

from sydr_amd._lib import LOOP_CFG_DTYPE, TRACK_STATE_DTYPE
from sydr_amd.engine import FMT_CF64, FMT_CI16, FMT_CI8

pytestmark = pytest.mark.gpu

NAMES = tuple(lec.CASES)
# the smallest set of rates that reaches every core (tests/test_gpu_track_cores.py: RATES)
CORES = {4e6: dict(W512="PS", C8="PS", D="PS"), 10e6: dict(W512="B8", C8="B8", D="B8"),
         20e6: dict(W512="B16", C8="SG", D="B16"), 25e6: dict(W512="B16", C8="SG", D="CH")}
N_DENSE = 260                                     # more channels than the MI355X has compute units
DENSE_SAMPLE = (0, 1, 2, 3, 4, 5, 6, 7, 129, 255, 259)
SPLITS = (1, 6, 150)                              # resumed launches: across the edge of epoch 1 and the later one
SCENES = {}
WORST = {}                                        # (fs, form, taps) -> {quantity: worst ratio}

STATE_EXACT = ("n_samples", "current_sample", "code_counter", "track_flags", "nav_sum_counter", "nav_bits_emitted")
STATE_EXACT_KAPLAN = ("accum_counter", "lock_state", "time_in_state", "spacing_sel", "fll_bw", "pll_bw")
STATE_RELATIVE = ("carrier_hz", "code_hz", "code_step", "i_prompt_prev", "q_prompt_prev", "nav_prompt_sum")
STATE_ABSOLUTE = ("rem_code", "dll_mem", "pll_mem")
STATE_ABSOLUTE_KAPLAN = ("fll_lock", "pll_lock", "cn0", "cn0_ratio_acc")


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    for (fs, form, taps), w in sorted(WORST.items()):
        print(f"\nworst device / oracle, {fs / 1e6:g} MHz {form} {taps} taps: " + " ".join(f"{k} {v:.1e}" for k, v in sorted(w.items())))


class Scene:
    """The stream of one rate: synthesised on the device, downloaded once; the acquisition and the oracle's trajectories."""

    def __init__(self, engine, fs):
        self.fs, self.n = fs, lec.stream_samples(fs)
        self.stage(engine)
        engine.iq_synth([lec.SAT], fs, lec.SIGMA, lec.SEED, 0, self.n)
        self.raw = engine.iq_download(self.n, 0).copy()
        self.stream = lec.Stream(self.raw)
        self.carrier, self.cur = lec.acquire(self.stream, fs)
        self.oracle = {}

    def stage(self, engine, fmt=FMT_CI8, raw=None, n=None):
        engine.iq_alloc(self.n if n is None else n, fmt)
        engine.code_slots(1)
        engine.load_gps_code(0, lec.PRN)
        if raw is not None:
            engine.iq_upload(raw, 0)

    def start(self, name, taps=3):
        """(state, configuration) of a case; five taps: VE/E/P/L/VL around the three-tap spacings, narrow = half of wide."""
        st = lec.seeded_state(name, self.fs, self.carrier, self.cur)
        kind, c = lec.CASES[name].kind, lec.case_cfg(name)
        if taps == 3:
            return st, loop_cfg(kind, self.fs, c)
        return st, general_cfg(kind, self.fs, c, list(FIVE), [0.5 * v for v in FIVE], 1023.0, 20, 1e-3)

    def reference(self, names, taps=3, epochs=lec.EPOCHS):
        """The oracle's (records, aux, end state, bits) per case: computed once, the cases side by side."""
        todo = [n for n in names if (n, taps, epochs) not in self.oracle]
        if todo:
            code = orc.gold_code(lec.PRN)
            with concurrent.futures.ThreadPoolExecutor(len(todo)) as pool:
                runs = pool.map(lambda n: lec.run_oracle(self.stream, *self.start(n, taps), code, epochs), todo)
                for n, run in zip(todo, runs):
                    assert lec.decision_margin(run[0], lec.case_cfg(n)) > lec.MARGIN, (self.fs, n)
                    self.oracle[(n, taps, epochs)] = run
        return {n: self.oracle[(n, taps, epochs)] for n in names}


def scene_for(engine, fs):
    if fs not in SCENES:
        SCENES[fs] = Scene(engine, fs)
    else:
        SCENES[fs].stage(engine, raw=SCENES[fs].raw)
    return SCENES[fs]


def launch(engine, form, states, cfgs, epochs):
    engine.track_cluster(tr.FORM_PARTS[form])       # W512 and D: one workgroup per channel (D: more channels than CUs)
    try:
        end, traj, bits, done = engine.track_closed_loop_ex(states, cfgs, epochs, want_bits=True)
    finally:
        engine.track_cluster(0)
    assert np.all(done == epochs), (form, done)
    return end, traj, bits


def channel_cases(form, names):
    """The case of every channel of a launch: one channel per case, or 260 channels cycling through the cases."""
    return [names[c % len(names)] for c in range(N_DENSE)] if form == "D" else list(names)


def check_against(got, ref, key, what):
    unequal, worst = lec.compare(got, ref)
    w = WORST.setdefault(key, {})
    for k, v in worst.items():
        w[k] = max(w.get(k, 0.0), v)
    assert not unequal, (what, unequal)
    assert max(worst.values()) <= RTOL, (what, worst)


def check_end_state(state, ref, kaplan, prompt, what):
    """The device's end sdr_track_state against the oracle's end attributes (`ref`: lock_edge_cases.run_oracle's row)."""
    got = lec.as_row(state, TRACK_STATE_DTYPE)
    for k in STATE_EXACT + (STATE_EXACT_KAPLAN if kaplan else ()):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in STATE_RELATIVE:
        scale = max(abs(ref[k]), prompt if "prompt" in k else 1e-300)
        assert abs(got[k] - ref[k]) <= RTOL * scale, (what, k, got[k], ref[k])
    for k in STATE_ABSOLUTE + (STATE_ABSOLUTE_KAPLAN if kaplan else ()):
        assert abs(got[k] - ref[k]) <= RTOL * max(abs(ref[k]), 1.0), (what, k, got[k], ref[k])
    two_pi = orc.GPS_TWO_PI if kaplan else 2 * np.pi
    d = (got["rem_carrier"] - ref["rem_carrier"] + two_pi / 2) % two_pi - two_pi / 2
    assert abs(d) <= RTOL * two_pi, (what, "rem_carrier", got["rem_carrier"], ref["rem_carrier"])


def check_launch(scene, form, names, taps, end, traj, bits, sample, core):
    cases = channel_cases(form, names)
    ref = scene.reference(names, taps)
    key = (scene.fs, form, taps)
    for ch in sample:
        name = cases[ch]
        recs, _, ref_end, ref_bits = ref[name]
        what = (scene.fs, form, taps, name, ch)
        ref_cols = lec.columns(recs)
        check_against(lec.columns(traj[ch], taps), ref_cols, key, what)
        assert np.array_equal(bits[ch], ref_bits), what
        assert np.array_equal(traj[ch]["nav_bit"][traj[ch]["nav_bit"] >= 0], ref_bits), what
        prompt = float(np.hypot(ref_cols["corr"][-1, taps - 1], ref_cols["corr"][-1, taps]))
        check_end_state(end[ch], ref_end, lec.CASES[name].kind == 1, prompt, what)
        # which correlator ran: a case must not pass on another core than the (rate, form) is there for
        cores = set(tr.classify(tr.columns(traj[ch]), form, "ci8", taps, scene.n))
        assert cores == {core}, (what, cores)


def golden_columns(ref):
    out = dict(start=ref[:, 0].astype(np.int64), n=ref[:, 1].astype(np.int64), corr=ref[:, 6:12])
    for k, col in dict(dll=12, pll=13, fll=14, carrier_hz=15, code_hz=16, carrier_err=17, code_err=18, cn0=19, pll_lock=20,
                       fll_lock=21).items():
        out[k] = ref[:, col]
    for k, col in dict(lock_state=22, flags=23, nav_bit=24).items():
        out[k] = ref[:, col].astype(np.int64)
    return out


# ------------------------------------------------------------------------------------------------ every edge, rate, form
@pytest.mark.parametrize("form", ["W512", "C8", "D"])
@pytest.mark.parametrize("fs", list(CORES))
def test_every_lock_edge_matches_the_oracle(engine, fs, form):
    scene = scene_for(engine, fs)
    cases = channel_cases(form, NAMES)
    states, cfgs = zip(*(scene.start(name) for name in cases))
    end, traj, bits = launch(engine, form, states, cfgs, lec.EPOCHS)
    sample = DENSE_SAMPLE if form == "D" else range(len(NAMES))
    check_launch(scene, form, NAMES, 3, end, traj, bits, sample, CORES[fs][form])
    if form == "D":                  # twins (channels 1 and 257 are both case B): same inputs, same kernel, the same bits
        assert traj[1].tobytes() == traj[257].tobytes() and bytes(end[1]) == bytes(end[257])
        assert traj[1].tobytes() != traj[2].tobytes()


@pytest.mark.parametrize("form", ["W512", "C8", "D"])
def test_seeded_reference_plugin_matches_the_device(engine, form):
    """4 MHz, the stream g6d was made on (uploaded; the device's synthesiser draws other noise): the device against the
    reference's own Kaplan plugin seeded alike, cases A-G -- no oracle in between."""
    g = load_golden("g6d_kaplan_edges.npz")
    raw, _, (carrier, cur) = lec.cpu_scene()
    fs = lec.FS_CPU
    engine.iq_alloc(raw.size // 2, FMT_CI8)
    engine.code_slots(1)
    engine.load_gps_code(0, lec.PRN)
    engine.iq_upload(raw, 0)
    cases = channel_cases(form, lec.GOLDEN_CASES)
    states = [lec.seeded_state(name, fs, carrier, cur) for name in cases]
    end, traj, bits = launch(engine, form, states, loop_cfg(1, fs, lec.EDGE_CFG), lec.EPOCHS)
    ring = 100 * int(fs * 1e-3)
    for ch in (DENSE_SAMPLE if form == "D" else range(len(lec.GOLDEN_CASES))):
        name = cases[ch]
        ref = g[f"{name}_epochs"]
        got = lec.columns(traj[ch])
        got["start"] = got["start"] % ring
        check_against(got, golden_columns(ref), (fs, form + " vs g6d", 3), (form, name, ch))
        assert np.array_equal(bits[ch], ref[ref[:, 24] >= 0, 24].astype(np.int8)), (form, name, ch)
        assert set(tr.classify(tr.columns(traj[ch]), form, "ci8", 3, raw.size // 2)) == {"PS"}


# ------------------------------------------------------------------------------------------------ five taps
@pytest.mark.parametrize("form", ["W512", "D"])
def test_tap_hand_over_with_five_taps(engine, form):
    """A general configuration (VE/E/P/L/VL, narrow = half of wide) at 25 MHz, cases A (narrow, wide, narrow) and C:
    all five taps of every epoch, so the outer ones move with the lock state too (the dense form's chip-aligned core is
    3-tap only: B16 there)."""
    scene = scene_for(engine, 25e6)
    names = ("A", "C")
    cases = channel_cases(form, names)
    states, cfgs = zip(*(scene.start(name, 5) for name in cases))
    end, traj, bits = launch(engine, form, states, cfgs, lec.EPOCHS)
    check_launch(scene, form, names, 5, end, traj, bits, DENSE_SAMPLE if form == "D" else (0, 1), "B16")
    recs = scene.reference(names, 5)["A"][0]
    assert {tuple(r["spacing"]) for r in recs} == {FIVE, tuple(0.5 * v for v in FIVE)}


# ------------------------------------------------------------------------------------------------ ring formats
@pytest.mark.parametrize("form", ["W512", "C8"])
def test_lock_edges_from_other_ring_formats(engine, form):
    """Case A at 25 MHz from ci16 and cf64 rings holding the ci8 stream's values: bit for bit the ci8 run (same values,
    same arithmetic), across both of its edges."""
    scene = scene_for(engine, 25e6)
    epochs = 200
    n = lec.stream_samples(25e6, epochs)
    raw = scene.raw[:2 * n]
    st, cfg = scene.start("A")
    runs = {}
    for fmt, dtype in ((FMT_CI8, np.int8), (FMT_CI16, np.int16), (FMT_CF64, np.float64)):
        scene.stage(engine, fmt, raw.astype(dtype), n)
        runs[fmt] = launch(engine, form, [st], [cfg], epochs)
    end, traj, bits = runs[FMT_CI8]
    lock = list(traj[0]["lock_state"])
    assert lock[0] == lec.WIDE and lock[-1] == lec.NARROW and len(bits[0]) >= 8       # 3>2 and 2>3 are in the run
    for fmt in (FMT_CI16, FMT_CF64):
        assert runs[fmt][1].tobytes() == traj.tobytes() and bytes(runs[fmt][0][0]) == bytes(end[0]), fmt
        assert np.array_equal(runs[fmt][2][0], bits[0])


# ------------------------------------------------------------------------------------------------ resume
def _resume_cases(form):
    return channel_cases(form, ("A", "D"))


@pytest.mark.parametrize("form", ["W512", "C8", "D"])
def test_resumed_launches_equal_the_single_launch(engine, form):
    """Cases A and D in launches of 1 + 6 + 150 + the rest, each resuming from the states the one before returned: the
    lock role's registers (the dense form's copy in LDS) are restored from and stored to sdr_track_state completely."""
    scene = scene_for(engine, 25e6)
    cases = _resume_cases(form)
    states, cfgs = zip(*(scene.start(name) for name in cases))
    end, traj, bits = launch(engine, form, states, cfgs, lec.EPOCHS)
    lock, flags = traj[0]["lock_state"], traj[1]["track_flags"]
    later = int(np.flatnonzero(lock == lec.NARROW)[0])
    assert lock[0] == lec.WIDE and sum(SPLITS[:2]) < later < sum(SPLITS)                # A: one edge per side of the splits
    assert flags[0] == 2 and np.any(flags[sum(SPLITS[:2]):sum(SPLITS)] == 3)            # D: cleared, set again
    cur, parts, part_bits = list(states), [], [[] for _ in cases]
    for k in SPLITS + (lec.EPOCHS - sum(SPLITS),):
        cur, t, b = launch(engine, form, cur, cfgs, k)
        parts.append(t)
        for ch in range(len(cases)):
            part_bits[ch].extend(b[ch])
    assert np.concatenate(parts, axis=1).tobytes() == traj.tobytes()
    for ch in range(len(cases)):
        assert bytes(cur[ch]) == bytes(end[ch]), ch
        assert part_bits[ch] == list(bits[ch]), ch


@pytest.mark.parametrize("parts", [1, 0])
def test_bank_in_uneven_steps_equals_the_single_launch(engine, parts):
    """The same run through the channel bank (states put by sdr_bank_put, kept on the device): blocks of uneven length
    mixed with one-epoch ticks.  A tick of a cluster is two launches cut at the exchange; the second adds the parts' sums
    in the order of the cooperative kernel, so every bit is the block launch's (parts = 0: the library's own cluster)."""
    scene = scene_for(engine, 25e6)
    names = ("A", "D")
    states, cfgs = zip(*(scene.start(name) for name in names))
    engine.track_cluster(parts)
    try:
        end, traj, _, done = engine.track_closed_loop_ex(states, cfgs, lec.EPOCHS)
        assert list(done) == [lec.EPOCHS] * 2
        bank = engine.bank(8)
        for ch, (st, cfg) in zip((5, 2), zip(states, cfgs)):
            bank.put(ch, lec.as_row(st, TRACK_STATE_DTYPE), lec.as_row(cfg, LOOP_CFG_DTYPE))
        got, left = [], lec.EPOCHS
        for k in (1, 0, 6, 0, 0, 150, 0, 37):        # 0: a receiver tick (one epoch, nothing to ingest)
            if k:
                rec, st, done, _ = bank.step([5, 2], k)
            else:
                rec, st, done = bank.tick(None, 0, [5, 2])
                rec = rec[:, None]
            assert list(done) == [max(k, 1)] * 2
            got.append(rec)
            left -= max(k, 1)
        rec, st, done, _ = bank.step([5, 2], left)
        got.append(rec)
        bank_end = [bank.get(5), bank.get(2)]
        bank.close()
    finally:
        engine.track_cluster(0)
    assert np.concatenate(got, axis=1).tobytes() == traj.tobytes()
    for ch in range(2):
        assert st[ch].tobytes() == bytes(end[ch]) == bank_end[ch].tobytes(), ch
