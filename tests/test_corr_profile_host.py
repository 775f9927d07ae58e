"""The host layers of sdr_corr_profile without a GPU: the channel, the manager and the manager of several devices build the
item of a channel's LATEST epoch from the bank's `last` row and make one engine call -- against the oracle-backed engine of
tests/fake_engine.py, given the profile's NumPy statement (tests/corr_cases.py) as its `corr_profile`."""
import numpy as np
import pytest

import corr_cases as cc
from fake_engine import OracleEngine
from oracle import sydr_oracle as orc
from sydr_amd.channel.l1ca_borre import ChannelL1CA
from sydr_amd.channel.l1ca_kaplan import ChannelL1CA_Kaplan
from sydr_amd.channel.manager import ChannelManager
from sydr_amd.channel.multidevice import MultiDeviceChannelManager
from sydr_amd.utils.enumerations import ChannelState
from test_host_layer import BORRE_INI, KAPLAN_INI, channel_config, rf_signal


class ProfileEngine(OracleEngine):
    """OracleEngine + corr_profile: the model, item by item; counts its calls."""
    profile_calls = 0

    def corr_profile(self, items, first, step, n_taps, fs):
        self.profile_calls += 1
        rf = self.ring[0::2].astype(np.float64) + 1j * self.ring[1::2].astype(np.float64)
        return np.array([cc.profile_model(rf, self.codes[int(it["code_slot"])], fs,
                                          (int(it["code_slot"]), int(it["n_samples"]), int(it["start_sample"]), float(it["carrier_hz"]),
                                           float(it["rem_carrier"]), float(it["rem_code"]), float(it["code_step"])), first, step, n_taps)
                         for it in items])


FS, SPMS = 4e6, 4000
SATS = [dict(prn=p, doppler=d, code_phase=c, phase=0.1, amp=8.0) for p, d, c in ((7, 1750.0, 300.25), (12, -3000.0, 17.5))]


def _tracking_manager(plugin, ini, multi, ms=16):
    eng = ProfileEngine()
    mgr = ChannelManager(rf_signal(FS), engines=[eng]) if multi else ChannelManager(rf_signal(FS), engine=eng)
    mgr.addChannel(plugin, channel_config(ini), 3)
    chans = [mgr.requestTracking(s["prn"]) for s in SATS]
    raw = orc.synth_iq(FS, ms * SPMS, SATS, 20.0, 99)
    return eng, mgr, chans, raw


@pytest.mark.parametrize("multi", [False, True], ids=["one_device", "device_list"])
@pytest.mark.parametrize("plugin,ini", [(ChannelL1CA_Kaplan, KAPLAN_INI), (ChannelL1CA, BORRE_INI)], ids=["kaplan", "borre"])
def test_profiles_of_the_latest_epoch_in_one_call(plugin, ini, multi):
    eng, mgr, chans, raw = _tracking_manager(plugin, ini, multi)
    assert isinstance(mgr, MultiDeviceChannelManager) == multi
    with pytest.raises(ValueError, match="no tracking epoch"):
        chans[0].correlationProfile(-0.5, 0.5, 3)
    assert mgr.correlationProfiles(-0.5, 0.5, 3) == {} and eng.profile_calls == 0
    for k in range(16):
        mgr.addNewRFData(raw[2 * k * SPMS:2 * (k + 1) * SPMS])
        mgr.run()
    assert all(ch.channelState is ChannelState.TRACKING for ch in chans)
    profiles = mgr.correlationProfiles(-0.5, 0.5, 3)
    assert eng.profile_calls == 1                                   # ONE call for every tracking channel
    assert sorted(profiles) == [ch.channelID for ch in chans]       # (the idle third channel has none)
    for ch in chans:
        last = np.array(ch.correlatorsResults[:6]).reshape(3, 2)
        assert profiles[ch.channelID].shape == (3, 2)
        assert np.abs(profiles[ch.channelID] - last).max() <= cc.CAP * np.hypot(last[:, 0], last[:, 1]).max()
        assert np.array_equal(ch.correlationProfile(-0.5, 0.5, 3), profiles[ch.channelID])
        slot, n, start, f, rc, rk, cstep = ch.correlationProfileItem()
        rec = ch._bank.last[ch.channelID]
        assert (slot, n, start) == (ch.codeSlot, int(rec["n_samples"]), int(rec["start_sample"]))
        assert (f, rc, rk, cstep) == (rec["carrier_hz_in"], rec["rem_carrier_in"], rec["rem_code_in"], rec["code_step_in"])
    wide = mgr.correlationProfiles(-2.0, 1.0 / 16, 65)
    for ch in chans:
        mag = np.hypot(wide[ch.channelID][:, 0], wide[ch.channelID][:, 1])
        assert abs(int(mag.argmax()) - 32) <= 5 and wide[ch.channelID].shape == (65, 2)
    mgr.close()


def test_an_epoch_the_ring_no_longer_holds_is_refused():
    """Decided from the ring's write index and capacity: once more than capacity - n samples were written behind the
    epoch's last one, its first samples are gone."""
    eng, mgr, chans, raw = _tracking_manager(ChannelL1CA_Kaplan, KAPLAN_INI, False)
    for k in range(16):
        mgr.addNewRFData(raw[2 * k * SPMS:2 * (k + 1) * SPMS])
        mgr.run()
    ring = mgr.sharedBuffer
    ch = chans[0]
    _, n, start, *_ = ch.correlationProfileItem()
    unread = ring.getNbUnreadSamples((start + n) % ring.maxSize)
    room = ring.maxSize - n - unread                  # samples that may still be written before the epoch's first one goes
    assert room > SPMS
    ring.shiftIdxWrite(room // SPMS * SPMS)           # (bookkeeping alone: what the writes of that many samples leave)
    ch.correlationProfileItem()                       # still inside
    assert ch.channelID in mgr.correlationProfiles(-0.5, 0.5, 3)
    ring.shiftIdxWrite(SPMS)
    with pytest.raises(ValueError, match="no longer holds"):
        ch.correlationProfile(-0.5, 0.5, 3)
    assert ch.channelID not in mgr.correlationProfiles(-0.5, 0.5, 3)
    mgr.close()


def test_a_reused_or_parked_channel_is_refused():
    """A channel given a new satellite has run no epoch of it yet: its previous satellite's last record is not profiled
    with the new code.  A channel the device has parked (lost lock) is refused too: nothing guards the ring for it."""
    eng, mgr, chans, raw = _tracking_manager(ChannelL1CA_Kaplan, KAPLAN_INI, False)
    for k in range(16):
        mgr.addNewRFData(raw[2 * k * SPMS:2 * (k + 1) * SPMS])
        mgr.run()
    ch, other = chans
    assert ch.correlationProfile(-0.5, 0.5, 3).shape == (3, 2)
    ch._bank.lost[ch.channelID] = True
    with pytest.raises(ValueError, match="lost lock"):
        ch.correlationProfile(-0.5, 0.5, 3)
    assert sorted(mgr.correlationProfiles(-0.5, 0.5, 3)) == [other.channelID]
    ch._bank.lost[ch.channelID] = False
    ch.setSatellite(30)                               # the channel goes to another satellite
    with pytest.raises(ValueError, match="no tracking epoch"):
        ch.correlationProfile(-0.5, 0.5, 3)
    assert sorted(mgr.correlationProfiles(-0.5, 0.5, 3)) == [other.channelID]
    mgr.close()
