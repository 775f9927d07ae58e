"""What a call returns does not depend on what the engine did before it (docs/notes/engine_state.md lists the state an engine
carries from call to call).  Every probe of tests/engine_history_cases.py is first run on a FRESH engine and held to the
oracle or its statement at its family's own tolerance; those bytes are then the expectation, with ==, for the same call
after designed histories -- one per piece of carried state --, in seeded random orders over all probes and scenes, and on two
engines that share the device and take turns.  The engines are made here (never the session's), two alive at most."""
import numpy as np
import pytest

import engine_history_cases as ehc
from sydr_amd.engine import Engine

pytestmark = pytest.mark.gpu

P = ehc.PROBES
_FRESH = {}


def fresh(name, check=False):
    """The bytes of the probe's outputs on an engine that has done nothing else (made once, kept for the session)."""
    if name not in _FRESH or check:
        probe = P[name]
        e = Engine(0)
        try:
            ehc.stage(e, ehc.SCENES[probe.scene])
            out = probe.run(e)
            if check:
                probe.check(out)
            _FRESH.setdefault(name, ehc.to_bytes(out))
            assert ehc.to_bytes(out) == _FRESH[name], f"{name}: two fresh engines disagree"
        finally:
            e.close()
    return _FRESH[name]


class Walk:
    """One engine with a history: each call's bytes against the fresh engine's."""

    def __init__(self):
        self.e = Engine(0)
        self.scene = None
        self.log = []

    def close(self):
        self.e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def stage(self, scene):
        """(Re-)stage: the ring and the code slots are allocated again."""
        ehc.stage(self.e, ehc.SCENES[scene])
        self.scene = scene
        self.log.append(f"<stage {scene}>")

    def restage_slot(self, slot, prn=None):
        """One slot staged again -- with the scene's own code (default: another stamp, the same chips) or with another PRN."""
        kind, what = ehc.SCENES[self.scene].slots[slot]
        assert kind == "gps"
        self.e.load_gps_code(slot, int(what if prn is None else prn))
        self.log.append(f"<slot {slot} = PRN {what if prn is None else prn}>")

    def run(self, name, **opts):
        probe = P[name]
        if self.scene != probe.scene:
            self.stage(probe.scene)
        try:
            with ehc.options(self.e, opts):
                out = probe.run(self.e)
        finally:
            if probe.writes:
                ehc.restore(self.e, ehc.SCENES[probe.scene])
        self.log.append(name + (f" {opts}" if opts else ""))
        return out

    def same(self, name):
        """The call now == the call on a fresh engine, bit for bit."""
        want = fresh(name)
        got = ehc.to_bytes(self.run(name))
        assert got == want, f"{name} differs from a fresh engine's after: {' -> '.join(self.log[-12:])}"

    def off_route(self, name, **opts):
        """The call with options switched (another route: other bits are allowed, a wrong answer is not)."""
        P[name].check(self.run(name, **opts))

    def walk(self, steps):
        for step in steps:
            if callable(step):
                step(self)
            else:
                self.same(step)


def restage(slot, prn=None):
    return lambda w: w.restage_slot(slot, prn)


def stage_again(scene):
    return lambda w: w.stage(scene)


def off(name, **opts):
    return lambda w: w.off_route(name, **opts)


def unchecked(name):
    """A call whose answer is not the catalogue's (a slot holds another PRN): it only leaves its traces."""
    return lambda w: w.run(name)


# ------------------------------------------------------------------------------------------------ 1. fresh results are right
@pytest.mark.parametrize("name", ehc.NAMES)
def test_fresh_engine_agrees_with_the_reference(name):
    """The probe on a fresh engine against the oracle / statement at its family's tolerance; and a second fresh engine
    returns the same bytes (otherwise nothing below could hold)."""
    fresh(name, check=True)
    fresh(name, check=True)


# ------------------------------------------------------------------------------------------------ 2. designed sequences
# name -> (the state it aims at, the steps).  A string is a probe: its bytes must equal the fresh engine's.
SEQUENCES = {
    "twiddles": ("pcps_tw_n: the twiddle table of N = 4000, replaced by 10 000's, needed again",
                 ["map_4000", "map_10000", "map_4000", "sweeps_4mhz", "fused_10mhz", "sweeps_4mhz", "map_10000", "map_50000", "map_4000"]),
    "chirpz_plan": ("pcps_blu_n and the four chirp-z buffers: two chirp lengths, a radix length in between",
                    ["chirpz_4006", "chirpz_4079", "map_3000", "chirpz_4006", "chirpz_4079", "map_4000", "chirpz_4079"]),
    "spectra_key": ("pcps_spec_key (N, fs bits, slots and their stamps), code_generation: the cached code spectra",
                    ["sweeps_4mhz", "sweeps_4mhz", "sweeps_4mhz_subset", "sweeps_4mhz_permuted", "sweeps_4mhz", restage(2), "sweeps_4mhz",
                     "pcps_spectra", "sweeps_4mhz", stage_again("deep4"), "sweeps_4mhz", "acq_deep", "sweeps_4mhz", "sweeps_4.0004mhz",
                     "sweeps_4mhz", restage(0, 25), unchecked("sweeps_4mhz"), unchecked("map_4000"), restage(0), "sweeps_4mhz", "map_4000",
                     "sweeps_4mhz_other_grid", "sweeps_4mhz_permuted"]),
    "code2_image": ("pcps_code2_ok: the parity image of the code spectra at N = 50 000",
                    ["fused_50mhz_classes", "fused_50mhz_other_prns", "fused_50mhz_classes", restage(4), "map_50000", "fused_50mhz_classes",
                     restage(5, 2), unchecked("fused_50mhz_classes"), restage(5), "fused_50mhz_classes", "fused_25mhz_classes",
                     "fused_50mhz_classes"]),
    "offset_table": ("pcps_spec_off_key: the bins' offsets into the class spectra, grids of different (P, q)",
                     ["fused_25mhz_classes", "fused_25mhz_8_prns", "fused_25mhz_classes", "fused_50mhz_classes", "fused_25mhz_classes",
                      "fused_10mhz", "fused_10mhz_other_classes", "fused_10mhz", "fused_25mhz_classless", "fused_25mhz_classes"]),
    "work_list_25_then_50": ("pcps_work_key: the fused sweep's work list, equal (n_prn, vbins, block_bins), other pieces",
                             ["fused_25mhz_classless", "fused_50mhz_classless", "fused_25mhz_classless", "fused_50mhz_classless"]),
    "work_list_50_then_25": ("pcps_work_key, the other order",
                             ["fused_50mhz_classless", "fused_25mhz_classless", "fused_50mhz_classless", "fused_25mhz_classless"]),
    "theta_and_tickets": ("pcps_theta_prn / _flip, pcps_tickets_n: the per-PRN bound arrays and tickets, 4 -> 8 -> 4 PRNs",
                          ["fused_25mhz_classes", "fused_25mhz_8_prns", "fused_25mhz_classes", "fused_25mhz_classes", "fused_50mhz_classes",
                           "fused_25mhz_8_prns", "fused_50mhz_classes", "fused_25mhz_classless"]),
    "shared_scratch": ("pcps_a / _b / _fwd / _map / _part / _res and d_slots between unrelated calls",
                       ["sweeps_4mhz", "two_peak_compare", "sweeps_4mhz", "serial_search", "sweeps_4mhz", "two_peak_compare_ss", "map_4000",
                        "acq_deep_detect", "map_4000", "acq_deep", "pcps_spectra", "two_peak_compare", "acq_deep_detect", "serial_search",
                        "chirpz_4006", "acq_deep", "sweeps_4mhz"]),
    "probe_tables": ("probe_tab_nfft: the Welch transform's twiddles and window",
                     ["iq_probe_nfft_256", "iq_probe_nfft_1024", "iq_probe_nfft_256", "iq_probe_nfft_1024"]),
    "plan_pool": ("plan_pool: a destroyed plan's buffers under the next plan, across rates and calls",
                  ["plans_25mhz_straight_line", "plans_50mhz_half_chip_view", "plans_25mhz_straight_line", "epl_batch", "corr_profile",
                   "plans_50mhz_half_chip_view", "epl_batch"]),
    "half_chip_tables": ("luts2_generation / _stamp: the doubled replicas across a re-staged slot and re-allocated slots",
                         ["plans_50mhz_half_chip_view", restage(4), "plans_50mhz_half_chip_view", restage(4, 3),
                          unchecked("plans_50mhz_half_chip_view"), restage(4), "plans_50mhz_half_chip_view", stage_again("wide"),
                          "plans_50mhz_half_chip_view", "plans_25mhz_straight_line"]),
    "options_and_back": ("pcps_no_shared_spectra, pcps_fused, pcps_general_kernels, pcps_prn_chunk switched between identical calls",
                         ["fused_25mhz_classes", off("fused_25mhz_classes", pcps_no_shared_spectra=1), "fused_25mhz_classes",
                          off("fused_25mhz_classes", pcps_fused=0), "fused_25mhz_classes",
                          off("fused_25mhz_classes", pcps_general_kernels=1), "fused_25mhz_classes",
                          off("fused_25mhz_classes", pcps_fused=0, pcps_prn_chunk=1), "fused_25mhz_classes",
                          "fused_50mhz_classes", off("fused_50mhz_classes", pcps_no_shared_spectra=1), "fused_50mhz_classes",
                          off("fused_50mhz_classes", pcps_fused=0), "fused_50mhz_classes",
                          "fused_10mhz", off("fused_10mhz", pcps_fused=0), "fused_10mhz", off("fused_10mhz", pcps_no_shared_spectra=1),
                          "fused_10mhz", "sweeps_4mhz", off("sweeps_4mhz", pcps_prn_chunk=1), "sweeps_4mhz",
                          off("sweeps_4mhz", pcps_general_kernels=1), "sweeps_4mhz", "acq_deep", off("acq_deep", pcps_prn_chunk=1), "acq_deep"]),
    "exchange_tags": ("the closed-loop scratch of a stream (traj, xchg) and the two-launch ticks' exchange tags",
                      ["closed_loop_cluster", "bank_ticks", "closed_loop_one_workgroup", "bank_ticks", "bank_ticks", "closed_loop_cluster",
                       "closed_loop_one_workgroup"]),
    "lds_attribute": ("corr_lds_allowed / ddm_lds_allowed and the per-call workspaces: a longer code, a shorter one, the longer again",
                      ["ddm_long_code", "corr_profile_long_code", "ddm", "corr_profile", "ddm_long_code", "corr_profile_long_code",
                       "acq_refine", "ddm", "ddm_30000_chips", "ddm_24177_chips", "ddm", "ddm_30000_chips"]),
    "ring_writers": ("ddc_stage (every converter's), unpack_stage, cancel_ws; the ring restored behind each writer",
                     ["ddc_push_two_kinds", "ddc_push_two_kinds", "iq_cancel", "iq_cancel", "packed_upload", "sweeps_4mhz", "packed_upload",
                      "ddc_push_two_kinds", "iq_probe_nfft_256", "iq_cancel"]),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_designed_sequence(name):
    state, steps = SEQUENCES[name]
    print(f"{name}: {state}")
    with Walk() as w:
        w.walk(steps)


def test_options_are_reset_when_a_call_fails():
    """ehc.options puts every option back in its __exit__: after a refused call inside it the next call is the default route's."""
    with Walk() as w:
        w.same("fused_25mhz_classes")
        with pytest.raises(Exception):
            with ehc.options(w.e, {"pcps_fused": 0, "pcps_prn_chunk": 1}):
                w.e.pcps([99], 0, 25e6, 0.0, 5000.0, 125.0)           # no such slot
        w.same("fused_25mhz_classes")


# ------------------------------------------------------------------------------------------------ 3. seeded random orders
@pytest.mark.parametrize("seed", [20261201, 20261202, 20261203])
def test_seeded_random_order_of_every_probe(seed):
    """Every probe of every scene, shuffled; the scene is switched wherever the shuffle says."""
    order = list(np.random.default_rng(seed).permutation(ehc.NAMES))
    switches = sum(P[a].scene != P[b].scene for a, b in zip(order, order[1:]))
    print(f"seed {seed}: {len(order)} calls, {switches} scene switches")
    assert switches >= len(ehc.SCENE_NAMES)
    for name in order:
        fresh(name)
    with Walk() as w:
        w.walk(order)


# ------------------------------------------------------------------------------------------------ 4. two engines, one device
def test_two_engines_take_turns_on_one_device():
    """Different rings and codes on two engines of one process; each engine's bytes equal its fresh bytes.  sdr_ddm and
    sdr_corr_profile with a 4092-chip code on the first engine and 1023-chip codes on the second, the longer one first and
    again last (the dynamic-LDS attribute belongs to the kernel, the caches to the engines); the fused sweeps of both rates,
    whose work lists and bound arrays are per engine."""
    turns = [("ddm_long_code", "ddm"), ("corr_profile_long_code", "corr_profile"), ("ddm_long_code", "corr_profile"),
             ("fused_25mhz_classless", "fused_10mhz"), ("fused_50mhz_classless", "sweeps_4mhz"), ("fused_25mhz_classes", "map_4000"),
             ("plans_50mhz_half_chip_view", "epl_batch"), ("closed_loop_cluster", "fused_10mhz"), ("bank_ticks", "acq_deep"),
             ("corr_profile_long_code", "ddm"), ("ddm_long_code", "corr_profile")]
    for a, b in turns:
        fresh(a), fresh(b)
    with Walk() as first, Walk() as second:
        for a, b in turns:
            first.same(a)
            second.same(b)
        first.same("ddm_long_code")
        first.same("corr_profile_long_code")


def test_two_engines_ask_for_more_than_64_kib_of_lds_in_turn():
    """sdr_ddm over 64 KiB of dynamic LDS on two engines: 30 000 chips on the first, then 24 177 -- the shortest code that
    needs the attribute raised at all -- on the second, then the first again.  The attribute belongs to the kernel, each
    engine's record of it (ddm_lds_allowed) to the engine: the second engine's smaller request must not leave the first
    one's launch without its LDS."""
    for name in ("ddm_30000_chips", "ddm_24177_chips"):
        fresh(name)
    with Walk() as first, Walk() as second:
        first.same("ddm_30000_chips")
        second.same("ddm_24177_chips")
        first.same("ddm_30000_chips")
        second.same("ddm")
        first.same("ddm_30000_chips")
