"""A catalogue of PROBES for the engine-history tests (tests/test_gpu_engine_history.py; tests/test_engine_history_cases.py
holds the CPU half): what a call returns must not depend on what the engine did before it (docs/notes/engine_state.md).

A probe is one library call on a staged engine with a function that returns ALL of its outputs (results, maps, records, end
states, and the ring where the call writes it), a check of those outputs against the oracle or the call's statement at the
tolerance its family's own tests use, and a margin: the reference's decision must be clear of a tie (the two largest values
of its map more than MARGIN apart, as tests/deep_cases.py demands), so that two correct answers cannot differ in an index.
Probes are grouped into SCENES: one ring image plus one set of staged code slots.  Probes of a scene run without re-staging,
so the cached paths are the ones exercised; switching scene re-allocates the ring and the slots.

Inputs are those of the existing case modules where they fit (deep_cases, ddm_cases, corr_cases, refine_cases, cancel_cases,
downconvert_cases, resample_cases, the golden trajectory); everything is seeded and cached."""
import functools
from collections import namedtuple

import numpy as np

import cancel_cases as cnc
import corr_cases as cc
import ddm_cases as dd
import deep_cases as dc
import downconvert_cases as dcases
import refine_cases as rc
import resample_cases as rcases
from oracle import sydr_oracle as orc
from sydr_amd.signal import downconvert as dconv
from sydr_amd.signal import packing as pk
from sydr_amd.signal import probe as pb

FMT_CI8, FMT_CF64 = 0, 3
MARGIN = dc.MARGIN          # 1e-6, relative: the two largest values of the reference's map
MAP_RTOL = 1e-9             # tests/test_gpu_pcps.py
RATIO_RTOL = 1e-9           # ... and every ratio and correlator
OPTION_DEFAULTS = {"pcps_fused": 1, "pcps_general_kernels": 0, "pcps_prn_chunk": 0, "pcps_no_shared_spectra": 0}

Scene = namedtuple("Scene", "name fmt capacity image slots max_chips max_periods")
# run(engine) -> the outputs; check(outputs) asserts them against the reference; margin() measures on the CPU how far the
# reference's decisions keep from a tie or a threshold (the CPU test demands more than MARGIN).  `decides` False, margin() None:
# the call returns sums, exact integer counts or table look-ups and decides nothing a rounding could move -- those probes are
# named, each with its reason, in DECIDES_NOTHING and nowhere else.
# writes: the call writes the ring (the runner restores the scene's image behind it)
Probe = namedtuple("Probe", "name scene run check margin decides writes")


def to_bytes(out) -> bytes:
    """Every output of a probe, in order, as bytes."""
    if out is None:
        return b"<none>"
    if isinstance(out, (bytes, bytearray)):
        return bytes(out)
    if isinstance(out, np.ndarray):
        return str((out.dtype.str, out.shape)).encode() + np.ascontiguousarray(out).tobytes()
    if isinstance(out, (list, tuple)):
        return b"[" + b"|".join(to_bytes(v) for v in out) + b"]"
    if isinstance(out, dict):
        return to_bytes([(k, out[k]) for k in sorted(out)])
    if isinstance(out, (bool, int, str)):
        return repr(out).encode()
    if isinstance(out, float):
        return np.float64(out).tobytes()
    if isinstance(out, np.generic):
        return out.tobytes()
    return bytes(out)             # a ctypes structure


def stage(engine, scene):
    """The scene's ring and codes onto the engine."""
    engine.iq_alloc(scene.capacity, scene.fmt)
    engine.iq_upload(scene.image, 0)
    engine.code_slots(len(scene.slots), scene.max_chips, scene.max_periods)
    for slot, (kind, what) in enumerate(scene.slots):
        if kind == "gps":
            engine.load_gps_code(slot, int(what))
        else:
            engine.set_code(slot, what)


def restore(engine, scene):
    engine.iq_upload(scene.image, 0)


def slot_code(scene, slot):
    kind, what = scene.slots[slot]
    return orc.gold_code(int(what)) if kind == "gps" else np.asarray(what, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def scene_rf(name):
    """The scene's ring as complex128."""
    s = SCENES[name]
    rf = np.asarray(s.image, dtype=np.complex128) if np.iscomplexobj(s.image) else orc.iq_to_complex(s.image)
    rf.setflags(write=False)
    return rf


class options:
    """Engine options for the length of one call, each put back whatever happens."""

    def __init__(self, engine, opts):
        self.engine, self.opts = engine, dict(opts)

    def __enter__(self):
        for k, v in self.opts.items():
            self.engine.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.engine.set_option(k, OPTION_DEFAULTS[k])


# ------------------------------------------------------------------------------------------------------------ scenes
def _gps(prns):
    return tuple(("gps", int(p)) for p in prns)


def _int8_image(x):
    raw = np.empty(2 * len(x), dtype=np.int8)
    raw[0::2] = np.clip(np.rint(x.real), -127, 127)
    raw[1::2] = np.clip(np.rint(x.imag), -127, 127)
    raw.setflags(write=False)
    return raw


PRNS_4 = (7, 21, 3, 9, 14, 2, 30, 11)        # deep4: slots 0, 1 are deep_cases' (7 is present)
PRNS_WIDE = (1, 6, 12, 17, 20, 24, 27, 31)   # wide: slots 0-3 are present at 25 MHz, slots 4-7 at 50 MHz
PRNS_TEN = (5, 12, 19, 26)


def _scene_deep4():
    c, image, cap, start, _ = dc.parity_input("ci8_c2_k3_g2")
    assert start == 0 and cap == 24000 and c["prns"] == PRNS_4[:2]
    return Scene("deep4", FMT_CI8, cap, image, _gps(PRNS_4), 1023, 1)


def _synth(fs, n, prns, seed, sigma, amp=5.0):
    rng = np.random.default_rng(seed)
    sats = [dict(prn=p, doppler=float(rng.uniform(-4000, 4000)), code_phase=float(rng.uniform(0, 1023)), phase=float(rng.random()),
                 amp=amp) for p in prns]
    return orc.iq_to_complex(orc.synth_iq(fs, n, sats, sigma, seed))


def _scene_wide():
    x = _synth(50e6, 50000, PRNS_WIDE[4:], 20261101, 9.0)
    x[:25000] += _synth(25e6, 25000, PRNS_WIDE[:4], 20261102, 9.0)
    return Scene("wide", FMT_CI8, 50000, _int8_image(x), _gps(PRNS_WIDE), 1023, 1)


def _scene_ten():
    x = _synth(10e6, 10000, PRNS_TEN[::2], 20261103, 12.0, amp=7.0)
    return Scene("ten", FMT_CI8, 10000, _int8_image(x), _gps(PRNS_TEN), 1023, 1)


def _case_scene(name, case):
    slots = tuple(("gps", p) if p is not None else ("chips", np.asarray(c, dtype=np.int8)) for p, c in zip(case["prns"], case["codes"]))
    if len(slots) < 2:
        slots = slots + (("gps", 30),)
    return Scene(name, case["fmt"], case["capacity"], case["ring"], slots, case.get("max_chips", 1023), case.get("max_periods", 1))


DDM_CASE = "acq_4MHz_row0_B2_S8"
CORR_CASE = "rate_4MHz_65"
CORR_LONG_CASE = "long_code_4ms_4.092MHz"
CANCEL_CASE = "short"


@functools.lru_cache(maxsize=None)
def ddm_long_case():
    """sdr_ddm over corr_cases' 4092-chip code: its ring, its first item as the prediction, one block of four segments."""
    c = dict(cc.parity_cases()[CORR_LONG_CASE])
    c.update(name="ddm_long_code_4.092MHz", items=c["items"][:1], B=1, S=4, first=-2.0, step=0.25, T=17, span=250.0, step_hz=12.5)
    return c


# sdr_ddm keeps the code beside its prefix sums in LDS: 41 360 fixed bytes + the chips (ddm.hip kFixedLds), so 24 177 chips are
# the shortest code that takes it over the 64 KiB a kernel gets unasked (sdr_code_slots stops at 32 768); 30 000 ask for more
LDS_CHIPS = (30000, 24177)
assert 41360 + (LDS_CHIPS[1] + 15) // 16 * 16 > 65536 >= 41360 + (LDS_CHIPS[1] - 1 + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def lds_case(L):
    """A +-1 code of L chips at 1.023 Mchip/s in noise at 4 MHz; one prediction on it: 32 000 samples, one block of four segments."""
    fs, dop, W, start, rk, cap = 4e6, 1630.0, 32000, 1000, 0.25, 40000
    rng = np.random.default_rng([20261106, L])
    code = rng.integers(0, 2, L) * 2.0 - 1.0
    cstep = orc.CODE_RATE * (1.0 + dop / 1575.42e6) / fs
    n = np.arange(cap, dtype=np.float64)
    x = 20.0 * code[np.floor((rk - start * cstep) % L + n * cstep).astype(np.int64) % L] * np.exp(2j * np.pi * (dop / fs * n + 0.2))
    x += 25.0 * (rng.standard_normal(cap) + 1j * rng.standard_normal(cap))
    raw = _int8_image(x)
    return dict(name=f"ddm_{L}_chips", fs=fs, fmt=FMT_CI8, ring=raw, rf=orc.iq_to_complex(raw), capacity=cap, codes=[code], prns=[None],
                max_chips=L, max_periods=1, items=[(0, W, start, dop, 0.4, rk, cstep)], B=1, S=4, first=-2.0, step=0.25, T=17, span=250.0,
                step_hz=12.5)


def _scene_refine():
    a = rc.acquired(4e6, *rc.SATELLITES[0])
    raw = a["raw"][:2 * 48000]                        # (M = 10 periods behind s0: the window ends far inside)
    assert a["s0"] + 11 * 4000 < 48000
    return Scene("refine", FMT_CI8, 48000, raw, _gps((rc.PRN, 30)), 1023, 1)


def _scene_track():
    from test_oracle_golden import trajectory_iq
    g, fs, raw = trajectory_iq()
    n = 70 * 4000
    assert fs == 4e6 and raw.size >= 2 * n
    return Scene("track", FMT_CI8, n, raw[:2 * n], _gps((30, 7)), 1023, 1)


def _scene_cancel():
    c = cnc.geometry(CANCEL_CASE)
    slots = tuple(("gps", w) if k == "gps" else ("chips", np.asarray(w, dtype=np.int8)) for k, w in c["slots"])
    if len(slots) < 2:
        slots = slots + (("gps", 30),)
    return Scene("cancel", FMT_CI8, c["capacity"], cnc.ring_image(CANCEL_CASE, FMT_CI8), slots, 1023, 1)


def _scene_ddc():
    """A cf64 ring the converters write: its image is noise the pushes overwrite in part."""
    rng = np.random.default_rng(20261104)
    image = (rng.standard_normal(DDC_CAP) + 1j * rng.standard_normal(DDC_CAP)).astype(np.complex128)
    return Scene("ddc", FMT_CF64, DDC_CAP, image, _gps((3, 30)), 1023, 1)


DDC_N_IN = 9001
DDC_CAP = 16064
_BUILDERS = {"deep4": _scene_deep4, "wide": _scene_wide, "ten": _scene_ten, "refine": _scene_refine, "track": _scene_track,
             "cancel": _scene_cancel, "ddc": _scene_ddc,
             "ddm": lambda: _case_scene("ddm", dd.parity_cases()[DDM_CASE]),
             "corr": lambda: _case_scene("corr", cc.parity_cases()[CORR_CASE]),
             "corr_long": lambda: _case_scene("corr_long", cc.parity_cases()[CORR_LONG_CASE]),
             "lds_30000": lambda: _case_scene("lds_30000", lds_case(LDS_CHIPS[0])),
             "lds_24177": lambda: _case_scene("lds_24177", lds_case(LDS_CHIPS[1]))}


class _Scenes(dict):
    def __missing__(self, name):
        self[name] = _BUILDERS[name]()
        return self[name]


SCENES = _Scenes()
SCENE_NAMES = tuple(_BUILDERS)


# ------------------------------------------------------------------------------------------------------------ PCPS
def classes(fs, nbins, step):
    """P of plan_shared_spectra (pcps_plan.h): the smallest P <= 64 with 2 P <= bins whose P steps are a whole number q of
    transform bins (and q * ((bins - 1) / P) <= 4096), or 0: every bin its own forward transform."""
    N = orc.samples_per_code(fs)
    for P in range(1, 65):
        if 2 * P > nbins:
            break
        v = P * step * N / fs
        r = np.rint(v)
        if r >= 1.0 and abs(v - r) <= 1e-9 * r and r * ((nbins - 1) // P) <= 4096.0:
            return P
    return 0


PcpsRef = namedtuple("PcpsRef", "peak ratio margin map")


@functools.lru_cache(maxsize=None)
def pcps_ref(scene, prns, start, fs, if_hz, R, S, coh, noncoh, keep_map):
    N = orc.samples_per_code(fs)
    x = scene_rf(scene)[start:start + N * coh * noncoh].reshape(1, -1)
    out = []
    for p in prns:
        m = orc.pcps_map(x, if_hz, fs, orc.code_spectrum(orc.gold_code(p), fs), R, S, N, coh, noncoh)
        peak, ratio = orc.two_peak_compare(m, N, round(fs / orc.CODE_RATE))
        if keep_map:
            m.setflags(write=False)
        out.append(PcpsRef(peak, float(ratio), float(dc.top2_margin(m)), m if keep_map else None))
    return tuple(out)


def _check_pcps(name, out, ref, want_map):
    pb_, pc_, pr_, cmap = out
    assert (cmap is not None) == want_map and len(pb_) == len(ref)
    for k, r in enumerate(ref):
        assert [int(pb_[k]), int(pc_[k])] == r.peak, (name, k)
        assert abs(pr_[k] - r.ratio) <= RATIO_RTOL * r.ratio, (name, k, pr_[k], r.ratio)
        if want_map:
            assert cmap[k].shape == r.map.shape and np.abs(cmap[k] - r.map).max() <= MAP_RTOL * r.map.max(), (name, k)


def _pcps_probe(name, scene, slots, fs, R, S, if_hz=0.0, want_map=False, bins=None, fused=None, P=None, opts=()):
    prns = tuple(_BUILDERS_PRNS[scene][s] for s in slots)
    nbins = len(orc.doppler_bins(R, S))
    N = orc.samples_per_code(fs)
    # (the grids are what the catalogue says they are: asserted where the probe is made)
    assert bins is None or nbins == bins, (name, nbins)
    if fused is not None:
        terms = {25000: 1, 50000: 2}[N]
        assert (not want_map and terms * len(slots) * nbins >= 256) == fused, name
    if P is not None:
        assert classes(fs, nbins, S) == P, (name, classes(fs, nbins, S))

    def ref():
        return pcps_ref(scene, prns, 0, fs, if_hz, R, S, 1, 1, want_map)

    def run(e):
        with options(e, dict(opts)):
            return e.pcps(list(slots), 0, fs, if_hz, R, S, 1, 1, want_map=want_map)

    return Probe(name, scene, run, lambda out: _check_pcps(name, out, ref(), want_map), lambda: min(r.margin for r in ref()), True, False)


_BUILDERS_PRNS = {"deep4": PRNS_4, "wide": PRNS_WIDE, "ten": PRNS_TEN}


def _pcps_probes():
    P = _pcps_probe
    return [
        # the map route: radix passes at 4000 and 3000, chirp-z at two lengths (two chirps), the general four-step at 10 000
        P("map_4000", "deep4", (0, 1, 2), 4e6, 2000.0, 250.0, want_map=True, bins=17),
        P("map_3000", "deep4", (0, 1), 3e6, 1000.0, 250.0, want_map=True),
        P("chirpz_4006", "deep4", (0, 3), 4.006e6, 1000.0, 250.0, want_map=True),
        P("chirpz_4079", "deep4", (0, 3), 4.079e6, 1000.0, 250.0, want_map=True),
        P("map_10000", "ten", (0, 1), 10e6, 1000.0, 250.0, want_map=True),
        P("map_50000", "wide", (4, 5), 50e6, 500.0, 250.0, want_map=True),
        # the map-free sweeps at 4 MHz: every slot, a subset, a permutation, and a rate with the same N and other bits
        P("sweeps_4mhz", "deep4", (0, 1, 2, 3), 4e6, 5000.0, 250.0, bins=41),
        P("sweeps_4mhz_subset", "deep4", (2, 0), 4e6, 5000.0, 250.0),
        P("sweeps_4mhz_permuted", "deep4", (3, 1, 0, 2), 4e6, 5000.0, 250.0),
        P("sweeps_4mhz_other_grid", "deep4", (0, 1, 2, 3), 4e6, 4000.0, 500.0, if_hz=1250.0),
        P("sweeps_4.0004mhz", "deep4", (0, 1, 2, 3), 4.0004e6, 5000.0, 250.0),
        # the fused search at 10 MHz (ten classes: P x 300 Hz = 3 transform bins)
        P("fused_10mhz", "ten", (0, 1, 2, 3), 10e6, 5000.0, 300.0, bins=34, P=10),
        P("fused_10mhz_other_classes", "ten", (0, 1, 2, 3), 10e6, 5000.0, 250.0, bins=41, P=4),
        # the fused sweep at 25 and at 50 MHz: with classes and without; 4 x 82 = 4 x 2 x 41 = 328 = one round + 72 units
        P("fused_25mhz_classes", "wide", (0, 1, 2, 3), 25e6, 5000.0, 125.0, bins=81, fused=True, P=8),
        P("fused_25mhz_classless", "wide", (0, 1, 2, 3), 25e6, 5000.0, 123.0, bins=82, fused=True, P=0),
        P("fused_25mhz_8_prns", "wide", tuple(range(8)), 25e6, 5000.0, 250.0, bins=41, fused=True, P=4),
        P("fused_50mhz_classes", "wide", (4, 5, 6, 7), 50e6, 5000.0, 250.0, bins=41, fused=True, P=4),
        P("fused_50mhz_classless", "wide", (4, 5, 6, 7), 50e6, 5000.0, 247.0, bins=41, fused=True, P=0),
        P("fused_50mhz_other_prns", "wide", (0, 1, 2, 3), 50e6, 5000.0, 250.0, bins=41, fused=True, P=4),
    ]


def _spectra_probe():
    fs, R, S, prns = 4e6, 1000.0, 250.0, (PRNS_4[0], 25)            # (25 is staged nowhere: the caller's own spectrum)

    def ref():
        return pcps_ref("deep4", prns, 0, fs, 0.0, R, S, 1, 1, True)

    def run(e):
        spec = np.array([orc.code_spectrum(orc.gold_code(p), fs) for p in prns])
        return e.pcps_spectra(spec, 0, fs, 0.0, R, S, 1, 1, want_map=True)

    return Probe("pcps_spectra", "deep4", run, lambda out: _check_pcps("pcps_spectra", out, ref(), True),
                 lambda: min(r.margin for r in ref()), True, False)


SERIAL = dict(fs=4e6, R=500.0, S=250.0, slots=(0, 1))


@functools.lru_cache(maxsize=None)
def serial_ref():
    x = scene_rf("deep4")[:4000].reshape(1, -1)
    out = []
    for s in SERIAL["slots"]:
        m = orc.serial_search(x, orc.gold_code(PRNS_4[s]), SERIAL["R"], SERIAL["S"], SERIAL["fs"], 4000)
        peak, ratio = orc.two_peak_compare_ss(m)
        m.setflags(write=False)
        out.append(PcpsRef(peak, float(ratio), float(dc.top2_margin(m)), m))
    return tuple(out)


def _serial_probe():
    def run(e):
        return e.serial_search(list(SERIAL["slots"]), 0, SERIAL["fs"], SERIAL["R"], SERIAL["S"], want_map=True)

    return Probe("serial_search", "deep4", run, lambda out: _check_pcps("serial_search", out, serial_ref(), True),
                 lambda: min(r.margin for r in serial_ref()), True, False)


def _two_peak_probes():
    """The two host-map comparisons (they upload into pcps_map): the oracle's own maps, answers exact (one fp64 division)."""
    def m_pcps():
        return pcps_ref("deep4", PRNS_4[:3], 0, 4e6, 0.0, 2000.0, 250.0, 1, 1, True)[0]

    def check(out):
        r = m_pcps()
        assert out[0] == r.peak and out[1] == orc.two_peak_compare(r.map, 4000, 4)[1]

    def check_ss(out):
        r = serial_ref()[0]
        assert out[0] == r.peak and out[1] == orc.two_peak_compare_ss(r.map)[1]

    return [Probe("two_peak_compare", "deep4", lambda e: e.two_peak_compare(m_pcps().map, 4), check, lambda: m_pcps().margin, True, False),
            Probe("two_peak_compare_ss", "deep4", lambda e: e.two_peak_compare_ss(serial_ref()[0].map), check_ss,
                  lambda: serial_ref()[0].margin, True, False)]


DETECT = dict(n_peaks=3, excl_code=4, excl_bins=1)


def _deep_probes():
    c = dict(dc.PARITY["ci8_c2_k3_g2"], **DETECT)
    assert (c["C"], c["K"], c["G"]) == (2, 3, 2)

    def maps():
        return dc.parity_statement("ci8_c2_k3_g2")

    def margin():
        return min(float(dc.top2_margin(m)) for m in maps())

    def run(e):
        return e.acq_deep([0, 1], 0, c["fs"], c["if_hz"], c["R"], c["S"], c["C"], c["K"], c["G"], c["rf"], want_map=True)

    def check(out):
        from test_gpu_deep import _hold
        _hold("history: acq_deep", out[0], out[1], maps(), c)

    def run_detect(e):
        return e.acq_deep_detect([0, 1], 0, c["fs"], c["if_hz"], c["R"], c["S"], c["C"], c["K"], c["G"], c["rf"], c["n_peaks"],
                                 c["excl_code"], c["excl_bins"], want_map=True)

    def check_detect(out):
        from test_gpu_deep import _hold
        from test_gpu_detect import _hold as hold_detect
        res, peaks, noise, cmap = out
        _hold("history: acq_deep_detect", res, cmap, maps(), c)
        hold_detect("history: acq_deep_detect", c, res, peaks, noise, cmap)

    return [Probe("acq_deep", "deep4", run, check, margin, True, False),
            Probe("acq_deep_detect", "deep4", run_detect, check_detect, margin, True, False)]


# ------------------------------------------------------------------------------------------------------------ other ring readers
REFINE = dict(M=10, S=8, span=250.0, step=5.0)


def _refine_probe():
    def acquired():
        return rc.acquired(4e6, *rc.SATELLITES[0])

    @functools.lru_cache(maxsize=None)
    def model():
        a = acquired()
        return rc.refine_model(scene_rf("refine"), a["s0"], a["code"], 4e6, a["f0"], REFINE["M"], REFINE["S"], REFINE["span"], REFINE["step"])

    def run(e):
        from sydr_amd.engine import make_refine_items
        a = acquired()
        return e.acq_refine(make_refine_items(0, a["s0"], a["f0"]), 4e6, REFINE["M"], REFINE["S"], REFINE["span"], REFINE["step"],
                            want_tables=True)

    def check(out):
        from test_gpu_refine import check_parity
        res, power, z = out
        check_parity(res[0], power[0], z[0], model(), REFINE["M"], REFINE["S"], "history: acq_refine")

    return Probe("acq_refine", "refine", run, check, lambda: float(rc.margin(model()[3])), True, False)


def _items(case):
    from sydr_amd.engine import make_items
    return make_items(*(np.array(col) for col in zip(*case["items"])))


def _ddm_probe(name, scene, case_of):
    def run(e):
        c = case_of()
        return e.ddm(_items(c), c["fs"], c["B"], c["S"], c["first"], c["step"], c["T"], c["span"], c["step_hz"], want_segments=True)

    def check(out):
        from test_gpu_ddm import check_against_model
        check_against_model(case_of(), *out)

    return Probe(name, scene, run, check, lambda: min(float(dd.margin(m["map"])) for m in dd.case_model(case_of())), True, False)


def _corr_probe(name, scene, case_name):
    def run(e):
        c = cc.parity_cases()[case_name]
        return e.corr_profile(_items(c), c["first"], c["step"], c["n_taps"], c["fs"])

    def check(out):
        c = cc.parity_cases()[case_name]
        assert (cc.worst_error(out, cc.case_model(c)) <= cc.CAP).all()

    return Probe(name, scene, run, check, lambda: None, False, False)


EPL_SPACING = (-0.5, 0.0, 0.5)


def _epl_model(scene, items, fs, spacing=EPL_SPACING):
    """orc.epl per item on the scene's ring -> [n_items][2 * taps]"""
    rf = scene_rf(scene)
    out = []
    for it in items:
        x = rf[(int(it["start_sample"]) + np.arange(int(it["n_samples"]))) % len(rf)]
        code = orc.pad_code(np.asarray(slot_code(SCENES[scene], int(it["code_slot"])), dtype=np.float64))
        out.append(orc.epl(x, code, fs, float(it["carrier_hz"]), float(it["rem_carrier"]), float(it["rem_code"]), float(it["code_step"]),
                           spacing))
    return np.array(out)


def _check_epl(got, ref):
    scale = np.repeat(np.maximum(np.hypot(ref[:, 0::2], ref[:, 1::2]), 1.0), 2, axis=1)
    assert got.shape == ref.shape and np.max(np.abs(got - ref) / scale) < RATIO_RTOL        # (smoke()'s bar)


def _epl_batch_probe():
    def run(e):
        return e.epl_batch(_items(cc.parity_cases()[CORR_CASE]), EPL_SPACING, 4e6)

    def check(out):
        _check_epl(out, _epl_model("corr", _items(cc.parity_cases()[CORR_CASE]), 4e6))

    return Probe("epl_batch", "corr", run, check, lambda: None, False, False)


def plan_items(fs, slot, starts, doppler=-2250.0):
    from sydr_amd.engine import make_items
    step = orc.CODE_RATE / fs
    return make_items(slot, orc.required_samples(0.25, step), np.array(starts), doppler, 1.0, 0.25, step)


PLAN_STARTS = {25e6: (37, 12345, 20011), 50e6: (3, 8, 11)}       # (every window inside the ring)


def _plan_probe(name, fs, slot):
    """A plan made, run, fetched and destroyed (its buffers go to the pool), then a second one: the outputs of both."""
    def run(e):
        outs = []
        for k in range(2):
            plan = e.epl_plan(plan_items(fs, slot, PLAN_STARTS[fs][k:]), EPL_SPACING, fs)
            try:
                plan.run()
                outs.append((plan.variant, plan.fetch()))
            finally:
                plan.close()
        return outs

    def check(out):
        for k, (variant, got) in enumerate(out):
            _check_epl(got, _epl_model("wide", plan_items(fs, slot, PLAN_STARTS[fs][k:]), fs))
        # (the variant word, as tests/test_gpu_epl.py reads it: 26 + KM in the low byte -- a chip-aligned straight-line kernel --
        # and 65536 on the half-chip view, which is what needs luts2)
        assert out[0][0] == out[1][0] and (out[0][0] & 255) > 26 and (out[0][0] >= 65536) == (fs == 50e6), out[0][0]

    def margin():
        # the variant word is chosen on the host from the items' code_step: samples per chip (per half chip on the half-chip
        # view) against the chip-aligned kernels' limits (epl_variant.h: 15.5 and 25.9) and against the whole numbers between
        # which the block length KM is taken
        spc = 1.0 / float(plan_items(fs, slot, PLAN_STARTS[fs])["code_step"][0]) / (2.0 if fs == 50e6 else 1.0)
        assert 15.5 < spc < 25.9
        return float(min(spc - 15.5, 25.9 - spc, spc - np.floor(spc), np.ceil(spc) - spc) / spc)

    return Probe(name, "wide", run, check, margin, True, False)


def _probe_probe(name, nfft):
    start, n = 1001, 20000

    def run(e):
        r = e.iq_probe(start, n, nfft=nfft, fs=4e6, hist=True)
        return (r.raw(), r.hist, r.psd)

    def check(out):
        want = pb.probe(np.asarray(SCENES["deep4"].image)[2 * start:2 * (start + n)], nfft=nfft, fs=4e6)
        assert out[0] == want.raw() and np.array_equal(out[1], want.hist)
        assert np.max(np.abs(out[2] - want.psd)) <= 1e-9 * want.psd.max()

    return Probe(name, "deep4", run, check, lambda: None, False, False)


TRACK_EPOCHS = 60


def _track_setup():
    from test_gpu_tracking import initial_state, loop_cfg
    from test_oracle_golden import KAPLAN_CFG, trajectory_iq
    g, fs, _ = trajectory_iq()
    acq = g["kaplan_acq"]
    return g, fs, initial_state(1, fs, acq[3], int(acq[5]), KAPLAN_CFG, slot=1), loop_cfg(1, fs, KAPLAN_CFG)


def _check_track(records, n):
    """Epoch records against the reference's golden trajectory: integers equal, loop quantities to 1e-9 (test_gpu_tracking)."""
    from test_gpu_tracking import close
    g = _track_setup()[0]
    ref = g["kaplan_epochs"][:n]
    assert len(records) == n
    assert np.array_equal(records["start_sample"], ref[:, 0].astype(np.int64)) and np.array_equal(records["n_samples"], ref[:, 1].astype(np.int32))
    assert np.array_equal(records["lock_state"], ref[:, 22].astype(np.int32)) and np.array_equal(records["track_flags"], ref[:, 23].astype(np.int32))
    assert np.array_equal(records["nav_bit"], ref[:, 24].astype(np.int32))
    for t in range(3):
        mag = np.hypot(ref[:, 6 + 2 * t], ref[:, 7 + 2 * t])
        err = np.hypot(records["corr"][:, 2 * t] - ref[:, 6 + 2 * t], records["corr"][:, 2 * t + 1] - ref[:, 7 + 2 * t])
        assert np.all(err <= RATIO_RTOL * np.maximum(mag, 1.0))
    assert close(records["carrier_hz"], ref[:, 15]) and close(records["code_hz"], ref[:, 16])
    assert close(records["dll"], ref[:, 12], scale=1.0) and close(records["pll"], ref[:, 13], scale=1.0)
    assert close(records["fll"], ref[:, 14], scale=1.0) and close(records["cn0"], ref[:, 19], scale=1.0)


@functools.lru_cache(maxsize=None)
def track_margin(epochs):
    """The oracle's Kaplan loop over the first `epochs` epochs of the track scene (the golden run's integers, asserted): the
    closest any decision of those epochs comes to its decision point -- the lock indicators to the thresholds they are compared
    with (lock_edge_cases.decision_margin), the prompt's I to zero relative to the prompt (the sign behind bit sync), a bit's
    sum of twenty to zero relative to the sum of their magnitudes, and the argument of the next epoch's ceil() to a whole
    number of samples."""
    import lock_edge_cases as lec
    from test_oracle_golden import KAPLAN_CFG
    g, fs, st, _ = _track_setup()
    rf = scene_rf("track")
    loop = orc.KaplanLoop(fs, orc.gold_code(7), KAPLAN_CFG, st.carrier_hz, int(st.current_sample))
    recs, worst = [], np.inf
    for _ in range(epochs):
        recs.append(loop.step(rf[loop.current_sample:loop.current_sample + loop.n]))
        ip, qp = recs[-1]["corr"][2], recs[-1]["corr"][3]
        arg = (loop.epoch_chips - loop.rem_code) / loop.code_step
        worst = min(worst, abs(ip) / np.hypot(ip, qp), arg - np.floor(arg), np.ceil(arg) - arg)
        if recs[-1]["nav_bit"] >= 0:
            last = np.array([r["corr"][2] for r in recs[-loop.epochs_per_bit:]])
            worst = min(worst, abs(last.sum()) / np.abs(last).sum())
    ref = g["kaplan_epochs"][:epochs]
    assert [r["start"] for r in recs] == list(ref[:, 0].astype(np.int64)) and [r["n"] for r in recs] == list(ref[:, 1].astype(np.int64))
    assert [r["lock_state"] for r in recs] == list(ref[:, 22].astype(np.int64)) and [r["flags"] for r in recs] == list(ref[:, 23].astype(np.int64))
    assert [r["nav_bit"] for r in recs] == list(ref[:, 24].astype(np.int64))
    return float(min(worst, lec.decision_margin(recs, KAPLAN_CFG)))


def _closed_loop_probe(name, parts):
    def run(e):
        _, _, st, cfg = _track_setup()
        e.track_cluster(parts)
        try:
            states, traj = e.track_closed_loop([st], cfg, TRACK_EPOCHS)
        finally:
            e.track_cluster(0)
        return (bytes(states[0]), traj)

    return Probe(name, "track", run, lambda out: _check_track(out[1][0], TRACK_EPOCHS), lambda: track_margin(TRACK_EPOCHS), True, False)


BANK_TICKS = 4


def _bank_tick_probe():
    """A few receiver ticks without a slab (the ring is staged): the cluster's one-epoch step, cut at the exchange."""
    def run(e):
        from test_gpu_bank import as_row
        from sydr_amd._lib import LOOP_CFG_DTYPE, TRACK_STATE_DTYPE
        _, _, st, cfg = _track_setup()
        bank = e.bank(2)
        try:
            bank.put(1, as_row(st, TRACK_STATE_DTYPE), as_row(cfg, LOOP_CFG_DTYPE))
            recs, states = [], None
            for _ in range(BANK_TICKS):
                rec, states, done = bank.tick(None, 0, [1])
                assert list(done) == [1]
                recs.append(rec[0].copy())
            return (np.array(recs), states.copy())
        finally:
            bank.close()

    return Probe("bank_ticks", "track", run, lambda out: _check_track(out[0], BANK_TICKS), lambda: track_margin(BANK_TICKS), True, False)


# ------------------------------------------------------------------------------------------------------------ ring writers
def _cancel_probe():
    def run(e):
        c = cnc.geometry(CANCEL_CASE)
        stats = e.iq_cancel(c["items"], cnc.amps_of(CANCEL_CASE, FMT_CI8), c["fs"], window=(c["w0"], c["W"]))
        return (stats, e.iq_download(c["capacity"], 0))

    def check(out):
        from test_gpu_cancel import _expected_ring, _hold, _inside
        c = cnc.geometry(CANCEL_CASE)
        res, image = cnc.statement(CANCEL_CASE, FMT_CI8)
        assert np.array_equal(image, SCENES["cancel"].image) and out[0] == res.stats
        _hold("history: iq_cancel", out[1], _expected_ring(image, res, c["w0"]), FMT_CI8, cnc.bound(CANCEL_CASE, FMT_CI8),
              _inside(c["capacity"], c["w0"], c["W"]))

    def margin():
        # an integer ring: the statement's values keep clear of rounding ties and of the rails by more than the bound
        tie, rail = cnc.tie_and_rail_margins(CANCEL_CASE, FMT_CI8)
        d = cnc.bound(CANCEL_CASE, FMT_CI8)
        assert tie > d and rail > d
        return float(min(tie, rail) / d - 1.0)

    return Probe("iq_cancel", "cancel", run, check, margin, True, True)


DDC_PLAIN = (dconv.IN_R8, 33, 2)                 # (input, T, D): ddc.hip
DDC_RATIONAL = (dconv.IN_CI16, 5, 4, 43)         # (input, L, M, T): resample.hip


def _ddc_configs():
    a = dcases.config(DDC_PLAIN[0], DDC_PLAIN[1], DDC_PLAIN[2], dcases.FCWS["odd"], dcases.gain_for(DDC_PLAIN[0], FMT_CF64))
    b = rcases.config(DDC_RATIONAL[0], *DDC_RATIONAL[1:], dcases.FCWS["odd"], dcases.gain_for(DDC_RATIONAL[0], FMT_CF64))
    return a, b


DDC_OFFSETS = (0, 4800)


def _ddc_probe():
    """One push through a decimating converter and one through a rational resampler (both stage their inputs in ddc_stage),
    into two windows of a cf64 ring."""
    def raws():
        return [dcases.stream(fmt, DDC_N_IN) for fmt in (DDC_PLAIN[0], DDC_RATIONAL[0])]

    def run(e):
        outs = []
        for cfg, raw, off in zip(_ddc_configs(), raws(), DDC_OFFSETS):
            ddc = e.ddc_create(cfg)
            try:
                outs.append(e.ddc_push(ddc, raw, off))
            finally:
                e.ddc_destroy(ddc)
        return (outs, e.iq_download(DDC_CAP, 0))

    def check(out):
        from test_gpu_downconvert import check_ring
        from test_gpu_resample import check_ring as check_resampled
        counts, ring = out
        expect = np.asarray(SCENES["ddc"].image).view(np.float64).copy()
        touched = np.zeros(DDC_CAP, dtype=bool)
        for cfg, raw, off, n_out in zip(_ddc_configs(), raws(), DDC_OFFSETS, counts):
            v = dconv.statement(cfg, [raw])
            assert n_out == v.size and off + n_out <= DDC_CAP and not touched[off:off + n_out].any()
            touched[off:off + n_out] = True
            # (each converter against its own family's check: tests/test_gpu_downconvert.py, tests/test_gpu_resample.py)
            (check_ring if cfg.interpolation == 1 else check_resampled)(ring[2 * off:2 * (off + n_out)], v, cfg, FMT_CF64,
                                                                        dcases.max_abs(cfg.in_fmt, raw), "history: ddc_push")
        assert np.array_equal(ring.reshape(-1, 2)[~touched], expect.reshape(-1, 2)[~touched])

    return Probe("ddc_push_two_kinds", "ddc", run, check, lambda: None, False, True)


PACKING = pk.Packing(2, [-3, -1, 1, 3], msb_first=False)
PACKED_N, PACKED_OFFSET = 8000, 1000


def _packed_probe():
    def packed():
        rng = np.random.default_rng(20261105)
        return rng.integers(0, 256, pk.packed_bytes(PACKING, PACKED_N)).astype(np.uint8)

    def run(e):
        e.iq_upload_packed(packed(), PACKED_N, PACKING, PACKED_OFFSET)
        return e.iq_download(SCENES["deep4"].capacity, 0)

    def check(out):
        want = np.array(SCENES["deep4"].image)
        want[2 * PACKED_OFFSET:2 * (PACKED_OFFSET + PACKED_N)] = pk.unpack(packed(), PACKING)
        assert np.array_equal(out, want)

    return Probe("packed_upload", "deep4", run, check, lambda: None, False, True)


# ------------------------------------------------------------------------------------------------------------ the catalogue
def _build():
    probes = _pcps_probes() + [_spectra_probe(), _serial_probe()] + _two_peak_probes() + _deep_probes()
    probes += [_refine_probe(),
               _ddm_probe("ddm", "ddm", lambda: dd.parity_cases()[DDM_CASE]),
               _ddm_probe("ddm_long_code", "corr_long", ddm_long_case),
               _ddm_probe("ddm_30000_chips", "lds_30000", lambda: lds_case(LDS_CHIPS[0])),
               _ddm_probe("ddm_24177_chips", "lds_24177", lambda: lds_case(LDS_CHIPS[1])),
               _corr_probe("corr_profile", "corr", CORR_CASE),
               _corr_probe("corr_profile_long_code", "corr_long", CORR_LONG_CASE),
               _epl_batch_probe(),
               _plan_probe("plans_25mhz_straight_line", 25e6, 0),
               _plan_probe("plans_50mhz_half_chip_view", 50e6, 4),
               _probe_probe("iq_probe_nfft_256", 256), _probe_probe("iq_probe_nfft_1024", 1024),
               _closed_loop_probe("closed_loop_one_workgroup", 1), _closed_loop_probe("closed_loop_cluster", 0),
               _bank_tick_probe(),
               _cancel_probe(), _ddc_probe(), _packed_probe()]
    out = {p.name: p for p in probes}
    assert len(out) == len(probes)
    return out


PROBES = _build()
NAMES = tuple(PROBES)
# The probes without a margin, and why none can be stated: nothing in their outputs is an index, a sign or a rounded value.
DECIDES_NOTHING = {
    "corr_profile": "correlator sums I, Q per tap; no peak is picked",
    "corr_profile_long_code": "correlator sums I, Q per tap; no peak is picked",
    "epl_batch": "correlator sums I, Q per tap",
    "iq_probe_nfft_256": "exact integer sums, extremes, rail counts and histogram of an int8 ring, and a spectrum of sums; no peak is picked",
    "iq_probe_nfft_1024": "exact integer sums, extremes, rail counts and histogram of an int8 ring, and a spectrum of sums; no peak is picked",
    "ddc_push_two_kinds": "filter sums into a complex-double ring: nothing is rounded to an integer",
    "packed_upload": "a table look-up per 2-bit field: exact",
}
assert set(DECIDES_NOTHING) == {n for n, p in PROBES.items() if not p.decides}
