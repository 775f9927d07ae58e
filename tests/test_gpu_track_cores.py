"""Every correlator core of the closed-loop kernel against the oracle, epoch by epoch.

The closed-loop kernel picks one of five correlators per epoch (track_kernel.h): the per-sample core (PS), the 8- and
16-sample boundary variants (B8, B16), the single-round cluster core (SG) and the dense form's chip-aligned core (CH).
Which one runs depends on the kernel form (W512: one 512-thread workgroup per channel; C2 / C4 / C8: clusters of
256-thread workgroups; D: 256 threads, more channels than compute units), the ring format, the tap count, the code step,
the epoch length and where the epoch sits in the ring.  Each case below runs the closed loop on a seeded synthetic stream
(initial states from the synthesised satellites, not from an acquisition), replays every recorded epoch of a sample of
channels through the oracle's correlator (tests/track_replay.py) and requires |d(I + jQ)| <= 1e-11 * sum |x| per tap --
a rounding-error scale -- plus the NCO hand-over between records.  The classifier applied to the records proves which
(form, core) pairs a case reached.  `-s` prints the worst ratio per (form, core, format)."""
import collections

import numpy as np
import pytest

from oracle import sydr_oracle as orc
from test_gpu_multignss import FIVE, general_cfg
from test_gpu_tracking import loop_cfg
from test_oracle_golden import BORRE_CFG, KAPLAN_CFG

from sydr_amd._lib import TrackState
from sydr_amd.engine import FMT_CF32, FMT_CF64, FMT_CI16, FMT_CI8

import track_replay as tr

pytestmark = pytest.mark.gpu

FMT = {"ci8": FMT_CI8, "ci16": FMT_CI16, "cf32": FMT_CF32, "cf64": FMT_CF64}
DTYPE = {"ci8": np.int8, "ci16": np.int16, "cf32": np.float32, "cf64": np.float64}
PRNS = (3, 7, 11, 14, 19, 22, 27, 31)
EPOCHS = 25
MIN_EPOCHS = 20                      # replayed epochs per (form, core) pair a case claims
N_SMALL = 8                          # channels of a W512 / cluster launch (one per satellite)
SMALL_REPLAY = (0, 1, 2, 3)
N_DENSE = 260                        # more channels than the MI355X has compute units
DENSE_REPLAY = (0, 1, 2, 129, 255, 256, 257, 259)
TWINS = (7, 201)                     # identical inputs in the dense launch
KAPLAN_N = dict(KAPLAN_CFG, correlator_epl_narrow=0.25)
WORST = {}                           # (form, core, format) -> [worst err / sum|x|, epochs]


@pytest.fixture(scope="module", autouse=True)
def _worst_ratios():
    yield
    if WORST:
        print("\nworst |d(I+jQ)| / sum|x| per (form, core, format):")
        for (form, core, fmt), (w, k) in sorted(WORST.items()):
            print(f"  {form:5s} {core:4s} {fmt:5s} {w:9.2e}  ({k} epochs)")


def code_step(fs, dop):
    return orc.CODE_RATE * (1.0 + dop / 1575.42e6) / fs


def satellites(seed, sign=0):
    """Eight seeded satellites; sign = +1 / -1 puts every Doppler on that side."""
    rng = np.random.default_rng(seed)
    out = []
    for prn in PRNS:
        dop = float(np.round(rng.uniform(400.0, 4000.0) * (sign or rng.choice((-1, 1)))))
        out.append(dict(prn=prn, doppler=dop, code_phase=float(rng.uniform(0.0, 1023.0)), phase=float(rng.random()), amp=9.0))
    return out


class Scene:
    """A seeded ci8 stream of `sats` in a ring of `capacity` samples, its host copy, the codes staged per satellite."""

    def __init__(self, engine, fs, sats, seed, capacity):
        self.engine, self.fs, self.sats, self.capacity = engine, fs, sats, capacity
        engine.iq_alloc(capacity, FMT_CI8)
        self._codes()
        engine.iq_synth(sats, fs, 14.0, seed, 0, capacity)
        self.raw = engine.iq_download(capacity, 0).copy()
        self.ring = tr.ring_complex(self.raw)
        self.fmt = "ci8"

    def _codes(self):
        self.engine.code_slots(len(self.sats))
        for slot, s in enumerate(self.sats):
            self.engine.load_gps_code(slot, s["prn"])

    def reformat(self, fmt, data=None):
        """The same ring in another format (`data`: other interleaved samples to hold instead)."""
        data = self.raw if data is None else data
        self.engine.iq_alloc(self.capacity, FMT[fmt])
        self._codes()
        self.engine.iq_upload(np.asarray(data).astype(DTYPE[fmt]), 0)
        self.ring = tr.ring_complex(self.engine.iq_download(self.capacity, 0))
        self.fmt = fmt


def channels(scene, n_ch, seed, n_taps=3, dcode=None, twins=False):
    """Initial states from the synthesised satellites: channel c follows satellite c mod 8 with its own carrier (+-50 Hz)
    and code-phase (+-0.3 chip) offset; every 4th channel runs the Borre loop, every 3rd Kaplan channel starts in NARROW
    (narrow taps, lock indicators just above the threshold).  dcode(c) overrides the code-phase offset."""
    rng = np.random.default_rng(seed)
    fs = scene.fs
    states, cfgs, info = [], [], []
    for c in range(n_ch):
        j = c % len(scene.sats)
        sat = scene.sats[j]
        kind = 0 if c % 4 == 3 else 1
        narrow0 = kind == 1 and c % 3 == 1
        dc = rng.uniform(-0.3, 0.3) if dcode is None else dcode(c)
        dcarrier = rng.uniform(-50.0, 50.0)
        cstep = code_step(fs, sat["doppler"])
        start = int(np.ceil((2 * 1023.0 - sat["code_phase"]) / cstep)) + int(round(dc / cstep))
        c_loop = KAPLAN_N if kind == 1 else BORRE_CFG
        if n_taps == 3:
            cfg = loop_cfg(kind, fs, c_loop)
            wide = [cfg.spacing_wide[t] for t in range(3)]
            narrow = [cfg.spacing_narrow[t] for t in range(3)]
        else:
            wide = list(FIVE)
            narrow = [0.5 * v for v in FIVE] if kind == 1 else wide
            cfg = general_cfg(kind, fs, c_loop, wide, narrow, 1023.0, 20, 1e-3)
        st = TrackState()
        st.code_slot, st.current_sample = j, start
        st.code_step = orc.CODE_RATE / fs
        st.n_samples = orc.required_samples(0.0, st.code_step)
        st.carrier_hz, st.code_hz = sat["doppler"] + dcarrier, orc.CODE_RATE
        if kind == 1:
            if narrow0:
                st.lock_state, st.spacing_sel = orc.LOCK_NARROW, 1
                st.fll_bw, st.pll_bw = c_loop["fll_bandwidth_narrow"], c_loop["pll_bandwidth_narrow"]
                st.fll_lock = st.pll_lock = c_loop["fll_threshold_narrow"] + 0.003
            else:
                st.lock_state = orc.LOCK_PULL_IN
                st.fll_bw, st.pll_bw = c_loop["fll_bandwidth_pullin"], c_loop["pll_bandwidth_wide"]
        states.append(st)
        cfgs.append(cfg)
        info.append(dict(kind=kind, wide=wide, narrow=narrow, narrow0=narrow0, prn=sat["prn"], n0=st.n_samples))
    if twins:
        a, b = TWINS
        states[b], cfgs[b], info[b] = TrackState.from_buffer_copy(states[a]), cfgs[a], info[a]
    return states, cfgs, info


def run(engine, form, states, cfgs, epochs):
    engine.track_cluster(tr.FORM_PARTS[form])       # W512 and D: one workgroup per channel (D: more channels than CUs)
    try:
        _, traj, _, done = engine.track_closed_loop_ex(states, cfgs, epochs)
    finally:
        engine.track_cluster(0)
    assert np.all(done == epochs), (form, done)
    return traj


def replay_check(scene, form, traj, info, replay_ch, n_taps=3):
    """Replay the channels `replay_ch` epoch by epoch.  Returns ({(form, core): epochs}, [(channel, epoch, core, margin)])
    -- margin: samples between the epoch's end and the end of the ring (negative: the epoch wraps)."""
    cov = collections.Counter()
    where = []
    failures = []
    for ch in replay_ch:
        m = info[ch]
        cols = tr.columns(traj[ch])
        bad = tr.check_nco(cols, scene.fs, m["kind"], n0=m["n0"])
        if bad:
            failures.append((form, scene.fmt, ch, "nco", bad[:3]))
        taps = tr.spacings(cols, m["kind"], m["wide"], m["narrow"], m["narrow0"])
        expected, scale = tr.replay(cols, scene.ring, scene.fs, orc.gold_code(m["prn"]), taps)
        ratio = tr.tap_ratios(cols["corr"], expected, scale).max(axis=1)
        cores = tr.classify(cols, form, scene.fmt, n_taps, scene.capacity)
        for k, core in enumerate(cores):
            cov[(form, core)] += 1
            w = WORST.setdefault((form, core, scene.fmt), [0.0, 0])
            w[0], w[1] = max(w[0], float(ratio[k])), w[1] + 1
            pos = int(cols["start"][k]) % scene.capacity
            where.append((ch, k, core, scene.capacity - pos - int(cols["n"][k])))
            if not ratio[k] <= tr.BAR:
                failures.append((form, scene.fmt, ch, k, core, float(ratio[k])))
    assert not failures, failures[:8]
    return cov, where


def check_cores(cov, form, want, minimum=MIN_EPOCHS):
    got = {core: k for (f, core), k in cov.items() if f == form}
    assert set(got) == set(want) and all(k >= minimum for k in got.values()), (form, got, want)


def scene_for(engine, fs, seed, sign=0, epochs=EPOCHS, extra=0):
    capacity = (int((epochs + 3) * 1e-3 * fs) + extra + 7) // 8 * 8
    return Scene(engine, fs, satellites(seed, sign), seed, capacity)


# ------------------------------------------------------------------------------------------------ rates, ci8, 3 taps
FORMS = ("W512", "C2", "C4", "C8", "D")
RATES = {
    4e6: dict(W512={"PS"}, C2={"PS"}, C4={"PS"}, C8={"PS"}, D={"PS"}),
    10e6: dict(W512={"B8"}, C2={"B8"}, C4={"B8"}, C8={"B8"}, D={"B8"}),
    # D: the chip-aligned core is tried from 15.5 to 25.9 samples per chip, but the closed loop compiles its block length
    # in (tr.CHIP_BLOCK = 24): at 16.0 (16.368 MHz) and 20 samples per chip it declines, and B8 / B16 run
    16.368e6: dict(W512={"B8"}, C2={"B8"}, C4={"B8"}, C8={"B8"}, D={"B8"}),
    20e6: dict(W512={"B16"}, C2={"B16"}, C4={"B16"}, C8={"SG"}, D={"B16"}),
    25e6: dict(W512={"B16"}, C2={"B16"}, C4={"B16"}, C8={"SG"}, D={"CH"}),
    50e6: dict(W512={"B16"}, C2={"B16"}, C4={"B16"}, C8={"B16"}, D={"B16"}),
}


@pytest.mark.parametrize("fs", list(RATES))
def test_every_form_at_each_rate(engine, fs):
    seed = 7100 + int(fs // 1e5)
    scene = scene_for(engine, fs, seed)
    for form in FORMS:
        dense = form == "D"
        states, cfgs, info = channels(scene, N_DENSE if dense else N_SMALL, seed + 1, twins=dense)
        traj = run(engine, form, states, cfgs, EPOCHS)
        cov, _ = replay_check(scene, form, traj, info, DENSE_REPLAY if dense else SMALL_REPLAY)
        check_cores(cov, form, RATES[fs][form])
        if dense:
            assert traj[TWINS[0]].tobytes() == traj[TWINS[1]].tobytes()      # same inputs, same kernel: the same bits
            assert traj[TWINS[0]].tobytes() != traj[TWINS[0] + 1].tobytes()


# ------------------------------------------------------------------------------------------------ thresholds
# The nominal code step of each rate is the threshold itself; the DLL moves s (or n) off it, up for the channels that
# start with the replica late (+0.3 chip), down for the others -- both sides among the epochs of one launch.
THRESHOLD_ROWS = {
    "8.184MHz_s0.125": (8.184e6, dict(W512={"B8", "PS"}, C8={"B8", "PS"}, D={"B8", "PS"})),
    "17.05MHz_s0.06": (17.05e6, dict(W512={"B16", "B8"}, C8={"SG", "B8"})),
    "26.4957MHz_s1/25.9": (26.4957e6, dict(D={"B16"})),       # tried above 1/25.9, declined: 25-sample blocks
    "25.575MHz_M24/25": (25.575e6, dict(D={"CH", "B16"})),    # s = 1/25: the block length leaves the compiled-in 24
    "32.768MHz_n32768": (32.768e6, dict(C8={"SG", "B16"})),
}


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("row", list(THRESHOLD_ROWS))
def test_both_sides_of_each_threshold(engine, row, sign):
    fs, want = THRESHOLD_ROWS[row]
    seed = 7300 + int(fs // 1e5) + (sign > 0)
    scene = scene_for(engine, fs, seed, sign=sign)
    rng = np.random.default_rng(seed)
    jitter = rng.uniform(-0.05, 0.05, N_DENSE)
    for form, sides in want.items():
        dense = form == "D"
        n_ch = N_DENSE if dense else 2 * N_SMALL
        dcode = lambda c: (0.35 if c % 2 == 0 else -0.35) + jitter[c]
        states, cfgs, info = channels(scene, n_ch, seed + 1, dcode=dcode)
        traj = run(engine, form, states, cfgs, EPOCHS)
        cov, _ = replay_check(scene, form, traj, info, DENSE_REPLAY if dense else range(n_ch))
        got = {core: k for (f, core), k in cov.items() if f == form}
        assert set(got) == sides and min(got.values()) >= 3, (row, sign, form, got)
        if fs == 26.4957e6:     # both sides of s = 1/25.9 (where the chip-aligned core is tried) were reached
            steps = traj[list(DENSE_REPLAY)]["code_step_in"].ravel()
            assert np.any(steps >= tr.THRESHOLDS["kChipMinCodeStep"]) and np.any(steps < tr.THRESHOLDS["kChipMinCodeStep"])


# ------------------------------------------------------------------------------------------------ ring formats
@pytest.mark.parametrize("fmt", ["ci16", "cf32", "cf64"])
@pytest.mark.parametrize("fs", [10e6, 25e6])
def test_ring_formats(engine, fs, fmt):
    """ci16 / cf32 / cf64 rings holding the ci8 stream's values: each run passes the replay bar and is bitwise the ci8
    run -- except in the dense form at 25 MHz, where ci8 takes the chip-aligned core and the others B16."""
    seed = 7500 + int(fs // 1e5)
    scene = scene_for(engine, fs, seed)
    runs = {}
    for form in ("W512", "C8", "D"):
        dense = form == "D"
        runs[form] = (channels(scene, N_DENSE if dense else N_SMALL, seed + 1), DENSE_REPLAY if dense else SMALL_REPLAY)
    base = {form: run(engine, form, s, c, EPOCHS) for form, ((s, c, _), _) in runs.items()}
    scene.reformat(fmt)
    for form, ((states, cfgs, info), replay_ch) in runs.items():
        traj = run(engine, form, states, cfgs, EPOCHS)
        cov, _ = replay_check(scene, form, traj, info, replay_ch)
        ci8_core = RATES[fs][form]
        want = {"B16"} if ci8_core == {"CH"} else ci8_core
        check_cores(cov, form, want)
        if ci8_core != {"CH"}:
            assert traj.tobytes() == base[form].tobytes(), form


@pytest.mark.parametrize("fmt", ["cf32", "cf64"])
@pytest.mark.parametrize("fs", [10e6, 25e6])
def test_float_rings_with_gaussian_samples(engine, fs, fmt):
    """Float rings holding non-integer samples (the stream plus seeded Gaussian noise): replay only."""
    seed = 7700 + int(fs // 1e5)
    scene = scene_for(engine, fs, seed)
    noisy = scene.raw.astype(np.float64) + np.random.default_rng(seed).normal(0.0, 6.3, scene.raw.size)
    scene.reformat(fmt, noisy)
    assert np.any(scene.ring.real != np.round(scene.ring.real))
    for form in ("W512", "C8", "D"):
        dense = form == "D"
        states, cfgs, info = channels(scene, N_DENSE if dense else N_SMALL, seed + 1)
        traj = run(engine, form, states, cfgs, EPOCHS)
        cov, _ = replay_check(scene, form, traj, info, DENSE_REPLAY if dense else SMALL_REPLAY)
        check_cores(cov, form, {"B16"} if RATES[fs][form] == {"CH"} else RATES[fs][form])


# ------------------------------------------------------------------------------------------------ five taps
@pytest.mark.parametrize("fs", [10e6, 25e6])
def test_five_taps(engine, fs):
    """A general configuration (VE/E/P/L/VL at -1, -0.5, 0, 0.5, 1 chip; 1023 chips per epoch): the single-round core with
    NT = 5 in C8, the boundary variants elsewhere -- the dense form included (the chip-aligned core is 3-tap only)."""
    seed = 7900 + int(fs // 1e5)
    scene = scene_for(engine, fs, seed)
    want = {10e6: dict(W512={"B8"}, C8={"B8"}, D={"B8"}), 25e6: dict(W512={"B16"}, C8={"SG"}, D={"B16"})}[fs]
    for form, cores in want.items():
        dense = form == "D"
        states, cfgs, info = channels(scene, N_DENSE if dense else N_SMALL, seed + 1, n_taps=5)
        traj = run(engine, form, states, cfgs, EPOCHS)
        cov, _ = replay_check(scene, form, traj, info, DENSE_REPLAY if dense else SMALL_REPLAY, n_taps=5)
        check_cores(cov, form, cores)


# ------------------------------------------------------------------------------------------------ ring guards
# First epoch of channel i ends GUARD_D[i] samples before the end of the ring (negative: wraps around it).  The list
# crosses the end of the ring (-1 / 0), the single-round core's whole groups at 25 MHz (7 / 8), epoch_wraps' 16 samples
# (15 / 16) and the chip-aligned core's 32 (31 / 32), with every start mod 8.
GUARD_D = (-17, -1, 0, 1, 7, 8, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 31, 32, 33, 48)
GUARD_EPOCHS = 4


@pytest.mark.parametrize("fs", [10e6, 25e6])
def test_epochs_at_the_ring_guards(engine, fs):
    seed = 8100 + int(fs // 1e5)
    n0 = orc.required_samples(0.0, orc.CODE_RATE / fs)
    capacity = (int(8e-3 * fs) // 16) * 16 + 8                 # a multiple of 8, not of 16
    sats = satellites(seed)
    scene = Scene(engine, fs, sats, seed, capacity)
    starts = [capacity - n0 - d for d in GUARD_D]
    assert {s % 8 for s in starts} == set(range(8))
    seen = collections.defaultdict(set)
    for form in ("W512", "C8", "D"):
        n_ch = N_DENSE if form == "D" else len(GUARD_D)
        states, cfgs, info = channels(scene, n_ch, seed + 1)
        for c, st in enumerate(states):
            st.current_sample = starts[c % len(GUARD_D)]
        traj = run(engine, form, states, cfgs, GUARD_EPOCHS)
        _, where = replay_check(scene, form, traj, info, range(len(GUARD_D)))
        first = {margin: core for ch, k, core, margin in where if k == 0}
        assert sorted(first) == sorted(GUARD_D)
        for margin, core in first.items():
            seen[(form, core)].add(margin)
        assert sum(margin < 0 for ch, k, core, margin in where) >= 2          # epochs that wrap the ring
    # the guards from both sides, as the kernel's rule puts them
    if fs == 25e6:
        assert {-1, 0, 7} <= seen[("C8", "PS")] and {8, 15, 16, 48} <= seen[("C8", "SG")]
        assert {16, 31} <= seen[("D", "B16")] and {32, 33, 48} <= seen[("D", "CH")] and {-1, 0, 15} <= seen[("D", "PS")]
        assert {-17, -1, 0, 15} <= seen[("W512", "PS")] and {16, 31, 32} <= seen[("W512", "B16")]
    else:
        for form in ("W512", "C8", "D"):
            assert {-17, -1, 0, 15} <= seen[(form, "PS")] and {16, 17, 31, 32, 48} <= seen[(form, "B8")]
