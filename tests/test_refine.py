"""Fine carrier-frequency / bit-edge refinement (sdr_acq_refine), the CPU side: the two new entry points in the ABI, the
NumPy model alone on the inputs the GPU tests use (tests/test_gpu_refine.py) -- the proof that those inputs are fair --
and the plugins' two optional [ACQUISITION] keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refine_cases as rc
from conftest import REPO
from fake_engine import OracleEngine
from sydr_amd import _lib
from test_abi import declared_symbols
from test_host_layer import BORRE_INI, channel_config, drive, rf_signal

SPAN, STEP = 250.0, 5.0        # the parity cases' grid: +-250 Hz in 5 Hz steps (K = 101)
# (fs, n_periods, n_segments, row of rc.SATELLITES) of the single-item parity cases
SINGLE_CASES = [(4e6, 10, 8, 0), (10e6, 10, 8, 1), (25e6, 10, 8, 2), (4e6, 1, 8, 3), (4e6, 20, 8, 4), (4e6, 10, 1, 1)]
MARGIN = 1e-6                  # the model's maximum must exceed every other entry of P by more than this times itself


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_refine_symbols_are_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("sdr_acq_refine", "sdr_acq_refine_bins"):
        assert name in declared_symbols() and name in _lib.exported_symbols() and hasattr(lib, name)
    assert lib.sdr_abi_version() == 5 == _lib.ABI_VERSION


def test_refine_bins_host_helper():
    lib = _lib.load()
    for span, step in ((150.0, 5.0), (250.0, 5.0), (125.0, 10.0), (100.0, 7.0), (3.0, 5.0)):
        assert lib.sdr_acq_refine_bins(span, step) == 2 * int(np.floor(span / step)) + 1
    assert lib.sdr_acq_refine_bins(100.0, 0.0) == 0 and lib.sdr_acq_refine_bins(-1.0, 5.0) == 0


def test_refine_struct_layouts(tmp_path):
    assert C.sizeof(_lib.RefineItem) == 32 == _lib.REFINE_ITEM_DTYPE.itemsize
    assert C.sizeof(_lib.RefineResult) == 32 == _lib.REFINE_RESULT_DTYPE.itemsize
    for ct, dt in ((_lib.RefineItem, _lib.REFINE_ITEM_DTYPE), (_lib.RefineResult, _lib.REFINE_RESULT_DTYPE)):
        for name, (_, off) in dt.fields.items():
            assert getattr(ct, name).offset == off
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   "sizeof(sdr_refine_item),sizeof(sdr_refine_result),offsetof(sdr_refine_item,carrier_hz),"
                   "offsetof(sdr_refine_result,fine_idx));return 0;}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)]).split()] == [32, 32, _lib.RefineItem.carrier_hz.offset,
                                                                             _lib.RefineResult.fine_idx.offset]


# ------------------------------------------------------------------------------------------------ 2. the model alone
@pytest.mark.parametrize("fs", rc.RATES)
def test_model_recovers_frequency_and_edge(fs):
    """What the GPU recovery test asks of the device, asked of the model with tighter caps: within 2 Hz of the truth (the
    device: one 5 Hz step), every edge found, the best hypothesis at least 1.5 x the second best."""
    for seed, dop, later in rc.RECOVERY:
        c = rc.acquired(fs, seed, dop, later)
        fine, h, _, P, _ = rc.refine_model(c["rf"], c["s0"], c["code"], fs, c["f0"], 10, 8, 150.0, STEP)
        print(f"fs={fs / 1e6} dop={dop} coarse={c['f0']} fine={fine} edge={h} true={c['true_edge'](10)} "
              f"ratio={rc.hypothesis_ratio(P):.2f} margin={rc.margin(P):.2e}")
        assert abs(c["f0"] - dop) <= 150.0                      # the truth lies on the fine grid (noise may pick the next bin)
        assert abs(fine - dop) <= 2.0
        assert h == c["true_edge"](10)
        assert rc.hypothesis_ratio(P) >= 1.5


@pytest.mark.parametrize("fs,M,S,row", SINGLE_CASES)
def test_model_maximum_is_distinct_on_the_parity_cases(fs, M, S, row):
    c = rc.acquired(fs, *rc.SATELLITES[row])
    _, _, _, P, _ = rc.refine_model(c["rf"], c["s0"], c["code"], fs, c["f0"], M, S, SPAN, STEP)
    print(f"fs={fs / 1e6} M={M} S={S}: margin {rc.margin(P):.2e}")
    assert rc.margin(P) > MARGIN


def test_model_maximum_is_distinct_on_the_other_parity_inputs():
    _, rf, items = rc.many_items()
    for k, s0, f0 in items:
        P = rc.refine_model(rf, s0, rc.orc.gold_code(rc.MANY_SATS[k]["prn"]), 4e6, f0, 10, 8, SPAN, STEP)[3]
        assert rc.margin(P) > MARGIN, (k, s0)
    _, rf, code, s0, f0 = rc.long_code_case()
    fine, h, _, P, _ = rc.refine_model(rf, s0, code, 4e6, f0, 5, 8, SPAN, STEP)
    assert rc.margin(P) > MARGIN and abs(fine - rc.LONG_DOPPLER) <= 2.0 and h == 0
    for dtype in (np.int16,):                                    # the ci16 ring's recording
        c = rc.acquired(4e6, *rc.SATELLITES[0], dtype=dtype)
        assert rc.margin(rc.refine_model(c["rf"], c["s0"], c["code"], 4e6, c["f0"], 10, 8, SPAN, STEP)[3]) > MARGIN


# ------------------------------------------------------------------------------------------------ 3. plugin configuration
def _manager(fine_ms=None):
    from sydr_amd.channel.l1ca_borre import ChannelL1CA
    from sydr_amd.channel.manager import ChannelManager
    cfg = channel_config(BORRE_INI)
    if fine_ms is not None:
        cfg["ACQUISITION"]["fine_frequency_ms"] = str(fine_ms)
    eng = OracleEngine()
    mgr = ChannelManager(rf_signal(4e6), engine=eng)
    mgr.addChannel(ChannelL1CA, cfg, 1)
    return mgr, eng, mgr.requestTracking(7)


def test_keys_absent_nothing_changes():
    from sydr_amd.utils.enumerations import ChannelMessage, ChannelState
    c = rc.acquired(4e6, *rc.SATELLITES[0])
    for fine_ms in (None, 0):
        mgr, eng, ch = _manager(fine_ms)
        assert ch.acq_requiredSamples == 4000 == ch.acq_waitSamples and not ch.fineFrequencySearch
        ticks = drive(mgr, c["raw"], 4000, 3)
        acq = [p for t in ticks for p in t if p["type"] is ChannelMessage.ACQUISITION_UPDATE]
        assert len(acq) == 1 and eng.calls["pcps"] == 1 and ch.channelState is ChannelState.TRACKING
        assert any(p["type"] is ChannelMessage.ACQUISITION_UPDATE for p in ticks[0])      # in the first tick, as ever
        assert set(acq[0]) == {"cid", "type", "carrierFrequency", "codeOffset", "frequency_idx", "code_idx", "correlation_map",
                               "peak_ratio"}
        assert acq[0]["carrierFrequency"] == c["f0"]            # the grid's bin


def test_fine_frequency_ms_makes_the_channel_wait_for_the_window():
    """Fails on the parent, which ignores the key and acquires in the first tick."""
    from sydr_amd.utils.enumerations import ChannelMessage, ChannelState
    c = rc.acquired(4e6, *rc.SATELLITES[0])
    mgr, eng, ch = _manager(10)
    assert ch.fineFrequencySearch and ch.acq_fineFrequencyMs == 10 and ch.acq_fineFrequencyStep == 5.0
    assert ch.acq_requiredSamples == 4000                       # the searched slab is what it was
    assert ch.acq_waitSamples == 4000 + (10 + 1) * 4000
    ticks = drive(mgr, c["raw"], 4000, 11)                      # one millisecond short of the wait
    assert not any(p["type"] is ChannelMessage.ACQUISITION_UPDATE for t in ticks for p in t)
    assert eng.calls["pcps"] == 0 and ch.channelState is ChannelState.ACQUIRING
    with pytest.raises(ValueError):
        _manager(21)                                            # more than one data bit


def test_a_ring_too_short_for_the_window_is_refused_at_configuration():
    from sydr_amd.channel.l1ca_borre import ChannelL1CA
    from sydr_amd.channel.manager import ChannelManager
    cfg = channel_config(BORRE_INI)
    cfg["ACQUISITION"]["fine_frequency_ms"] = "10"
    mgr = ChannelManager(rf_signal(4e6), engine=OracleEngine(), ring_ms=10)      # 10 ms of ring, 12 ms of wait
    with pytest.raises(ValueError, match="ring"):
        mgr.addChannel(ChannelL1CA, cfg, 1)


def test_serial_search_plugin_ignores_the_keys():
    from sydr_amd.channel.l1ca_kaplan_ss import ChannelL1CA_Kaplan_SS
    from sydr_amd.channel.manager import ChannelManager
    from test_host_layer import KAPLAN_INI
    cfg = channel_config(KAPLAN_INI)
    cfg["ACQUISITION"]["fine_frequency_ms"] = "10"
    mgr = ChannelManager(rf_signal(4e6), engine=OracleEngine())
    mgr.addChannel(ChannelL1CA_Kaplan_SS, cfg, 1)
    ch = mgr.requestTracking(7)
    assert not ch.fineFrequencySearch and ch.acq_waitSamples == ch.acq_requiredSamples
