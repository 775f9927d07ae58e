"""A channel plugin whose tracking state lives on the GPU.

The reference's plugins (sydr/channel/channel_l1ca_kaplan.py, channel_l1ca_borre.py) carry the loop
state as Python attributes and update it statement by statement every millisecond.  Here a channel is
a VIEW: its state is one row of the device-resident bank that belongs to the device ring
(`ChannelBank`, one per GPU), every tracking epoch -- correlators, discriminators, loop filters, NCO,
lock-state machine, bit decisions -- is one device step for all channels, and the reference's
attribute names are properties over the mirrored row.  What stays on the host is what the reference's
plugin surface demands: the constructor signature, the INI keys, the acquisition seams
(`runSignalSearch` / `runPeakFinder` / `postAcquisitionUpdate`), `_processHandler`, the packets.

Subclasses describe a plugin declaratively: which loop (`LOOP_KIND`), which INI key feeds which
`sdr_loop_cfg` field (`CFG_KEYS`, `FILTERS`), which reference attribute name maps to which state /
record field (`STATE_VIEW`, `RECORD_VIEW`).
"""
from __future__ import annotations

import numpy as np

from ..dsp.ddm import segments_for
from ..engine import make_items, make_refine_items
from ..utils.constants import GPS_L1CA_CARRIER_FREQ, GPS_L1CA_CODE_FREQ, GPS_L1CA_CODE_MS, GPS_L1CA_CODE_SIZE_BITS, LNAV_MS_PER_BIT
from ..utils.devicering import CircularBuffer as DeviceRing
from ..utils.enumerations import ChannelMessage, ChannelState, GNSSSignalType, GNSSSystems, TrackingFlags
from .bank import tracking_packet
from .navdecoder import HOST_FLAGS, default_decoder
from .base import Channel
from .seams import GpuCorrelatorSeams


def loop_filter_taus(noise_bandwidth: float, damping: float, gain: float):
    """tau1, tau2 of a second-order loop filter from its noise bandwidth (sydr/dsp/tracking.py:39-61)."""
    wn = noise_bandwidth * 8.0 * damping / (4.0 * damping**2 + 1)
    return gain / wn**2, 2.0 * damping / wn


def _state_property(field, cast):
    def getter(self):
        return cast(self._bank.state[field][self._row])

    def setter(self, value):
        self._bank.state[field][self._row] = value
        self._bank.touch(self._row)
    return property(getter, setter)


def _record_property(field):
    return property(lambda self: float(self._bank.last[field][self._row]))


class _ViewMeta(type(Channel)):
    """Turns the STATE_VIEW / RECORD_VIEW tables of a plugin class into properties."""

    def __new__(mcls, name, bases, ns):
        for attr, (field, cast) in ns.get("STATE_VIEW", {}).items():
            ns.setdefault(attr, _state_property(field, cast))
        for attr, field in ns.get("RECORD_VIEW", {}).items():
            ns.setdefault(attr, _record_property(field))
        return super().__new__(mcls, name, bases, ns)


class DeviceTrackedChannel(GpuCorrelatorSeams, Channel, metaclass=_ViewMeta):
    LOOP_KIND = None          # bank.KIND_*
    N_TAPS = 3
    CFG_KEYS = {}             # [TRACKING] ini key -> sdr_loop_cfg field
    FILTERS = ()              # (cfg prefix, ini prefix): <ini>_noise_bandwidth/_damping_ratio/_loop_gain -> <cfg>_tau1/_tau2
    STATE_VIEW = {}           # reference attribute name -> (sdr_track_state field, cast)
    RECORD_VIEW = {}          # reference attribute name -> sdr_track_epoch field of the latest epoch

    def __init__(self, cid, sharedBuffer, resultQueue, rfSignal, configuration):
        if not isinstance(sharedBuffer, DeviceRing):
            raise TypeError("a device-tracked channel needs the device ring (sydr_amd.utils.devicering.CircularBuffer); "
                            "to accelerate the reference's own plugin over its host ring, mix GpuCorrelatorSeams into it")
        sharedBuffer.bankFor(cid)                       # (grows the ring's bank to hold this channel)
        self._ring, self._row = sharedBuffer, int(cid)
        self._bank.state[self._row] = np.zeros((), dtype=self._bank.state.dtype)
        self._bank.tracking[self._row] = self._bank.lost[self._row] = False
        self._bank.code_since_tow[self._row] = 0
        self._bank.tow[self._row], self._bank.tow_decoded[self._row], self._bank.host_flags[self._row] = 0.0, False, 0
        del self._bank.nav_bits[self._row][:]
        super().__init__(cid, sharedBuffer, resultQueue, rfSignal, configuration)
        self.setDecoding()
        self.codeOffset = 0
        self.setAcquisition(configuration['ACQUISITION'])
        self.setTracking(configuration['TRACKING'])

    @property
    def _bank(self):
        """The ring's channel bank AS IT IS NOW: the bank is re-created when it has to grow (a 33rd channel), and a
        reference kept from construction would leave this channel on the old, closed one."""
        return self._ring.channelBank

    # ------------------------------------------------------------------ configuration ([ACQUISITION] / [TRACKING])
    def setAcquisition(self, configuration):
        self.acq_dopplerRange = float(configuration['doppler_range'])
        self.acq_dopplerSteps = float(configuration['doppler_steps'])
        self.acq_coherentIntegration = int(configuration['coherent_integration'])
        self.acq_nonCoherentIntegration = int(configuration['non_coherent_integration'])
        self.acq_threshold = float(configuration['threshold'])
        ms = self.acq_nonCoherentIntegration * self.acq_coherentIntegration
        self.acq_requiredSamples = int(self.rfSignal.samplingFrequency * 1e-3 * ms)
        # optional (no counterpart in the reference): a fine frequency search over `fine_frequency_ms` code periods from the
        # sample tracking starts at, on a grid of `fine_frequency_step` Hz across +-doppler_steps (sdr_acq_refine);
        # absent or 0: off -- tracking starts on the search grid's bin, as the reference does
        self.acq_fineFrequencyMs = int(configuration.get('fine_frequency_ms', 0))
        self.acq_fineFrequencyStep = float(configuration.get('fine_frequency_step', 5.0))
        if not 0 <= self.acq_fineFrequencyMs <= LNAV_MS_PER_BIT or not self.acq_fineFrequencyStep > 0.0:
            raise ValueError(f"fine_frequency_ms must lie in 0..{LNAV_MS_PER_BIT} (one data bit) and fine_frequency_step be positive")
        if self.fineFrequencySearch and self.acq_waitSamples > self.rfBuffer.maxSize:
            raise ValueError(f"the ring holds {self.rfBuffer.maxSize} samples; the search and the fine frequency window behind it "
                             f"need {self.acq_waitSamples} (a longer ring_ms, or a shorter fine_frequency_ms)")
        self._acqFine = None
        # optional (no counterpart in the reference): the deep search (sdr_acq_deep) in place of sdr_pcps when either key
        # is present -- `bit_edge_groups` (1 or 2 interleaved sets of coherent blocks, so that with blocks of half a data
        # bit one set holds no bit edge) and `code_doppler_compensation` (0 or 1: every block's map moved back by the
        # code's drift at the bin's Doppler, scaled by the L1 carrier).  coherent_integration / non_coherent_integration
        # keep their meaning.  Both absent: sdr_pcps, as the reference searches.
        self.acq_deep = None
        if 'bit_edge_groups' in configuration or 'code_doppler_compensation' in configuration:
            groups = int(configuration.get('bit_edge_groups', 1))
            compensate = int(configuration.get('code_doppler_compensation', 0))
            if groups not in (1, 2) or compensate not in (0, 1):
                raise ValueError("bit_edge_groups must be 1 or 2 and code_doppler_compensation 0 or 1")
            if not 1 <= self.acq_coherentIntegration <= LNAV_MS_PER_BIT or self.acq_nonCoherentIntegration < groups:
                raise ValueError(f"the deep search takes coherent_integration in 1..{LNAV_MS_PER_BIT} and at least "
                                 "bit_edge_groups non-coherent blocks")
            self.acq_deep = (groups, GPS_L1CA_CARRIER_FREQ if compensate else 0.0)
        self._acqDeep = None
        # optional (no counterpart in the reference): with `detection_sigmas` the channel searches through
        # sdr_acq_deep_detect -- the deep search with the two keys above if given, else one group and no compensation -- and
        # counts as acquired iff its strongest peak stands `detection_sigmas` standard deviations or more above the mean of
        # the map's noise cells (z_0 of include/sydr_amd.h); `threshold` is still parsed and no longer decides anything.
        # `detection_peaks` (1..8) separated peaks are kept, each clear of the others by `detection_exclusion_chips` chips
        # of code and `detection_exclusion_bins` Doppler bins.  A channel that is not acquired goes back to IDLE.
        self.acq_detect = None
        if 'detection_sigmas' in configuration:
            sigmas = float(configuration['detection_sigmas'])
            n_peaks = int(configuration.get('detection_peaks', 1))
            chips = float(configuration.get('detection_exclusion_chips', 1.0))
            excl_bins = int(configuration.get('detection_exclusion_bins', 1))
            if not sigmas > 0.0 or not 1 <= n_peaks <= 8 or not chips >= 0.0 or excl_bins < 0:
                raise ValueError("detection_sigmas must be positive, detection_peaks lie in 1..8 and the exclusion windows "
                                 "not be negative")
            groups = 1 if self.acq_deep is None else self.acq_deep[0]
            if not 1 <= self.acq_coherentIntegration <= LNAV_MS_PER_BIT or self.acq_nonCoherentIntegration < groups:
                raise ValueError(f"detection statistics take coherent_integration in 1..{LNAV_MS_PER_BIT} and at least "
                                 "bit_edge_groups non-coherent blocks")
            excl_code = int(np.rint(chips * (self.rfSignal.samplingFrequency / GPS_L1CA_CODE_FREQ)))
            per_code = int(np.rint(self.rfSignal.samplingFrequency * GPS_L1CA_CODE_SIZE_BITS / GPS_L1CA_CODE_FREQ))
            if n_peaks * (2 * excl_code + 1) >= per_code:
                raise ValueError("detection_peaks x the excluded code columns leave no noise cell")
            self.acq_detect = (sigmas, n_peaks, excl_code, excl_bins)
        self._acqDetect = None
        self.acq_detection = None       # the last search's peaks and noise figures: see acquisitionDetection

    def setTracking(self, configuration):
        """Fill this channel's sdr_loop_cfg row and the state tracking starts from (kaplan:256-338, borre:206-259)."""
        cfg, st = self._bank.cfg[self._row], self._bank.state[self._row]
        cfg["loop_kind"], cfg["n_taps"], cfg["fs"] = self.LOOP_KIND, self.N_TAPS, self.rfSignal.samplingFrequency
        for key, field in self.CFG_KEYS.items():
            cfg[field] = float(configuration[key])
        for cfg_prefix, ini_prefix in self.FILTERS:
            cfg[cfg_prefix + "_tau1"], cfg[cfg_prefix + "_tau2"] = loop_filter_taus(
                float(configuration[ini_prefix + "_noise_bandwidth"]), float(configuration[ini_prefix + "_damping_ratio"]),
                float(configuration[ini_prefix + "_loop_gain"]))
        self._configure_taps(configuration, cfg)
        st["code_hz"] = GPS_L1CA_CODE_FREQ
        st["code_step"] = GPS_L1CA_CODE_FREQ / self.rfSignal.samplingFrequency
        st["n_samples"] = int(np.ceil((GPS_L1CA_CODE_SIZE_BITS - 0.0) / st["code_step"]))   # 4001 at 4 MHz
        self._initial_loop_state(st, cfg)
        self._bank.touch(self._row)

    def _configure_taps(self, configuration, cfg):
        raise NotImplementedError

    def _initial_loop_state(self, st, cfg):
        pass

    # ------------------------------------------------------------------ views that need more than a cast
    @property
    def channelState(self):
        return self._channel_state

    @channelState.setter
    def channelState(self, value):
        self._channel_state = value
        self._bank.tracking[self._row] = value is ChannelState.TRACKING
        ring = self._bank.ring                                 # (the manager caches its channel lists against this)
        ring.stateVersion = getattr(ring, "stateVersion", 0) + 1

    @property
    def currentSample(self):
        return int(self._bank.state["current_sample"][self._row]) % self.rfBuffer.maxSize

    @currentSample.setter
    def currentSample(self, value):
        self._bank.state["current_sample"][self._row] = int(value)
        self._bank.touch(self._row)

    @property
    def trackFlags(self):
        v = int(self._bank.state["track_flags"][self._row]) | int(self._bank.host_flags[self._row])
        return TrackingFlags(v) if v in TrackingFlags._value2member_map_ else v

    @trackFlags.setter
    def trackFlags(self, value):
        """The tracking loop's bits live on the device, the decoder's (HOST_FLAGS) on the host."""
        device_bits = int(value) & ~HOST_FLAGS
        self._bank.host_flags[self._row] = int(value) & HOST_FLAGS
        if device_bits != int(self._bank.state["track_flags"][self._row]):
            self._bank.state["track_flags"][self._row] = device_bits
            self._bank.touch(self._row)

    @property
    def tow(self):
        return self._bank.channel_tow(self._row)

    @tow.setter
    def tow(self, value):
        self._bank.tow[self._row], self._bank.tow_decoded[self._row] = float(value), bool(value)

    @property
    def codeSinceTOW(self):
        return int(self._bank.code_since_tow[self._row])

    @codeSinceTOW.setter
    def codeSinceTOW(self, value):
        self._bank.code_since_tow[self._row] = int(value)

    @property
    def correlatorsResults(self):
        return self._bank.last["corr"][self._row][:2 * self.N_TAPS]

    @property
    def navBits(self):
        return self._bank.nav_bits[self._row]

    @property
    def lostLock(self):
        """True once the device stopped this channel because its NCO left the staged replica / the ring."""
        return bool(self._bank.lost[self._row])

    # ------------------------------------------------------------------ satellite
    def setSatellite(self, satelliteID):
        super().setSatellite(satelliteID)
        self.systemID = GNSSSystems.GPS
        self.signalID = GNSSSignalType.GPS_L1_CA
        eng = self._ensure_code()                       # Gold code generated by the device LFSR kernel
        self._bank.state["code_slot"][self._row] = self.codeSlot
        self._bank.last["n_samples"][self._row] = 0     # (no epoch of THIS satellite yet: correlationProfileItem)
        chips = eng.read_code(self.codeSlot).astype(np.float64)
        self.code = np.r_[chips[-1], chips, chips[0]]   # padded table of kaplan:104-107, kept for API compatibility

    # ------------------------------------------------------------------ decoding seam (navdecoder.py)
    DECODER_PLUGIN = "kaplan"      # whose subframe logic the default (reference-backed) decoder drives

    def setDecoding(self, decoder="default"):
        """Choose what turns this channel's navigation bits into DECODING_UPDATE packets / `tow` / the TOW and EPH
        flags (kaplan:680-698 sets up the reference's own buffers at this point).  "default": the reference's own
        subframe logic when `sydr` is importable on this host, else None (bits only); None; or any NavDecoder."""
        if isinstance(decoder, str):
            decoder = default_decoder(self.channelID, self.DECODER_PLUGIN)
        self._bank.decoders[self._row] = decoder
        if decoder is not None:
            decoder.reset()

    @property
    def navDecoder(self):
        return self._bank.decoders[self._row]

    def runDecoding(self):
        """The seam of kaplan:702-726 / borre:455: the DECODING_UPDATE packet completed by the epoch `runTracking` just
        ran, or None.  (The bits are decided on the device and pushed through the decoder as they arrive -- bank.py
        `_new_bit`; a ChannelManager collects the packets of all channels itself.)"""
        mine = [item for item in self._bank.decoded if item[0] == self._row]
        if not mine:
            return None
        self._bank.decoded.remove(mine[0])
        return mine[0][2]

    def getTimeSinceTOW(self):
        ms = self.codeSinceTOW * GPS_L1CA_CODE_MS
        return ms + self.rfBuffer.getNbUnreadSamples(self.currentSample) / (self.rfSignal.samplingFrequency / 1e3)

    # ------------------------------------------------------------------ per-tick entry of ONE channel
    def _processHandler(self):
        """What `Channel.run()` calls when a channel is driven on its own; a ChannelManager batches instead."""
        if self.channelState == ChannelState.IDLE:
            raise Warning(f"Tracking channel {self.channelID} is in IDLE.")
        if self.channelState == ChannelState.ACQUIRING:
            packet = self.runAcquisition()
        elif self.channelState == ChannelState.TRACKING:
            return [p for p in (self.runTracking(), self.runDecoding()) if p is not None]
        else:
            raise ValueError(f"Channel state {self.channelState} is not valid.")
        return [] if packet is None else [packet]

    # ------------------------------------------------------------------ acquisition (host seams around sdr_pcps)
    FINE_FREQUENCY_SEGMENTS = 8     # segments a code period is cut into for the fine search (sdr_acq_refine's n_segments)
    _injectedFine = None            # set by a batching manager: this channel's row of its group's sdr_acq_refine results

    @property
    def fineFrequencySearch(self) -> bool:
        """The fine search belongs to the default PCPS seam: a plugin that replaces `runSignalSearch` (the SerialSearch
        plugin) ignores the two keys."""
        return self.acq_fineFrequencyMs > 0 and type(self).runSignalSearch is GpuCorrelatorSeams.runSignalSearch

    @property
    def acq_waitSamples(self) -> int:
        """Unread samples acquisition waits for: the searched slab, and with the fine search on the window behind it --
        it starts at the sample tracking starts at, which `enterTracking` puts between one code period before and one
        sample past the slab's end, so it ends inside (fine_frequency_ms + 1) more milliseconds."""
        if self._warmHint is not None or not self.fineFrequencySearch:     # (a warm search has no fine stage behind it)
            return self.acq_requiredSamples
        return self.acq_requiredSamples + (self.acq_fineFrequencyMs + 1) * int(self.rfSignal.samplingFrequency * 1e-3)

    def runAcquisition(self):
        if self.rfBuffer.getNbUnreadSamples(self.currentSample) < self.acq_waitSamples:
            return None
        if self._warmHint is not None:
            return self.runWarmAcquisition()
        correlationMap = self.runSignalSearch()
        indices, ratio = self.runPeakFinder(correlationMap)
        # (the deep search's window is long enough for the code to drift: tracking starts behind the window, so it takes
        # the code start referred to the window's end -- peak_code_end -- where the packet reports the map's own index)
        start = indices if self._acqDeep is None else [indices[0], int(self._acqDeep["peak_code_end"])]
        if self._acqDetect is not None and not self.acquisitionDetection():     # (set by the default search seam alone)
            # not acquired: no tracking state is made, the channel is free for another satellite (the packet reports
            # the search as any acquisition packet does)
            self._acqFine = self._injectedFine = None
            self.channelState = ChannelState.IDLE
            return self.prepareResultsAcquisition(correlationMap, indices, ratio)
        self._acqFine = self.runFineFrequencySearch(start) if self.fineFrequencySearch else None
        self.postAcquisitionUpdate(start)
        return self.prepareResultsAcquisition(correlationMap, indices, ratio)

    def acquisitionDetection(self) -> bool:
        """Keep the search's detection figures as `acq_detection` -- dict(peaks=[dict(group, bin, code, code_end, value, z)],
        noise=dict(n_cells, mean, variance), sigmas, acquired) -- and decide: acquired iff z_0 >= detection_sigmas."""
        peaks, noise = self._acqDetect
        self._acqDetect = None
        acquired = bool(float(peaks[0]["z"]) >= self.acq_detect[0])
        self.acq_detection = dict(
            peaks=[dict(group=int(p["group"]), bin=int(p["bin"]), code=int(p["code"]), code_end=int(p["code_end"]),
                        value=float(p["value"]), z=float(p["z"])) for p in peaks],
            noise=dict(n_cells=int(noise["n_cells"]), mean=float(noise["mean"]), variance=float(noise["variance"])),
            sigmas=self.acq_detect[0], acquired=acquired)
        return acquired

    # ------------------------------------------------------------------ warm acquisition (sdr_ddm around a hint)
    _warmHint = None                # a prediction for this channel's next acquisition: see setWarmHint
    _injectedWarm = None            # set by a batching manager: (this channel's sdr_ddm_result row, its map or None)
    WARM_SEGMENT_FRACTION = 0.25    # a segment of the warm search is this part of a code period or shorter

    def setWarmHint(self, atSample, codePhaseChips, carrierFrequency, codeStep=None, chips=4.0, chipStep=0.25, spanHz=500.0,
                    stepHz=25.0):
        """A prediction for the next acquisition of this channel: at ring sample `atSample` the code phase is
        `codePhaseChips` (the rem_code of an sdr_epl_item that starts there) and the carrier `carrierFrequency` (IF
        included), the code advances by `codeStep` chips per sample (None: the nominal rate); the truth is expected within
        +-`chips` (searched at `chipStep`) and +-`spanHz` (at `stepHz`).  While the hint stands, `runAcquisition` searches
        that neighbourhood with one sdr_ddm item over its usual slab instead of the whole code period and every bin."""
        if not (chips > 0.0 and chipStep > 0.0 and spanHz >= 0.0 and stepHz > 0.0):
            raise ValueError("the uncertainties of a warm hint must be positive")
        step = GPS_L1CA_CODE_FREQ / self.rfSignal.samplingFrequency if codeStep is None else float(codeStep)
        self._warmHint = dict(sample=int(atSample), phase=float(codePhaseChips), carrier=float(carrierFrequency), code_step=step,
                              chips=float(chips), chip_step=float(chipStep), span_hz=float(spanHz), step_hz=float(stepHz))

    def warmRequest(self):
        """This channel's warm search: the sdr_epl_item fields of its slab (the hint's phase carried forward to the slab's
        first sample) and the sdr_ddm_cfg values -- a batching manager puts a tick's warm channels into one call."""
        h = self._warmHint
        fs, W = self.rfSignal.samplingFrequency, int(self.acq_requiredSamples)
        ahead = (self.currentSample - h["sample"]) % self.rfBuffer.maxSize
        phase = (h["phase"] + ahead * h["code_step"]) % GPS_L1CA_CODE_SIZE_BITS
        B = max(1, int(self.acq_nonCoherentIntegration))
        S = segments_for(W, B, GPS_L1CA_CODE_SIZE_BITS / h["code_step"], self.WARM_SEGMENT_FRACTION)
        half = int(np.floor(h["chips"] / h["chip_step"]))
        return dict(item=(self.codeSlot, W, self.currentSample, h["carrier"], 0.0, phase, h["code_step"]), fs=fs, n_blocks=B,
                    n_segments=S, first_chips=-half * h["chip_step"], step_chips=h["chip_step"], n_taps=2 * half + 1,
                    span_hz=h["span_hz"], step_hz=h["step_hz"])

    def runWarmAcquisition(self):
        """The warm search and, from its peak, the step a PCPS result takes: `enterTracking` with a fresh loop state at
        peak_hz, at the sample where the code period begins according to rem_code + peak_chips."""
        r = self.warmRequest()
        if self._injectedWarm is not None:
            (res, cmap), self._injectedWarm = self._injectedWarm, None
        else:
            out, maps, _ = self._ensure_code().ddm(make_items(*r["item"]), r["fs"], r["n_blocks"], r["n_segments"], r["first_chips"],
                                                   r["step_chips"], r["n_taps"], r["span_hz"], r["step_hz"])
            res, cmap = out[0], maps[0]
        self._warmHint = None
        step = r["item"][6]
        phase = r["item"][5] + float(res["peak_chips"])                   # the code phase at the slab's first sample
        # rem_code = 0 at sample t means the period's first chip begins right behind t (idx = ceil(i * step)): t is where
        # the phase comes round to a whole period -- the code sample a PCPS peak reports, which _firstEpochSample turns
        # into the first epoch's sample
        per_code = int(np.round(GPS_L1CA_CODE_SIZE_BITS / step))
        code_idx = int(np.round(((-phase) % GPS_L1CA_CODE_SIZE_BITS) / step)) % per_code
        second = float(res["second_value"])
        ratio = float(res["peak_value"]) / second if second > 0.0 else float("inf")
        self._acqFine = self._acqDeep = None
        self.enterTracking(float(res["peak_hz"]), code_idx)
        packet = self.prepareResultsAcquisition(cmap, [int(res["peak_bin"]), code_idx], ratio)
        packet["warm_start"] = True
        return packet

    def reacquire(self, chips=4.0, chipStep=0.25, spanHz=500.0, stepHz=25.0):
        """From TRACKING (lost or not) back to ACQUIRING with this channel's own NCO state as the warm hint: the next
        epoch's first sample, its rem_code, the carrier and the code step.  The loop state, the flags, the bit and
        subframe synchronisation start afresh, as after a cold acquisition.  The searched slab starts at that sample: call
        while the ring still holds it.  Nothing guards the ring for a channel the device has parked (`lostLock`) -- one
        parked more than a ring's length ago would search newer samples with a stale phase -- so reacquire promptly, or
        start such a channel anew with `requestTrackingWarm` from a prediction carried forward."""
        if self.channelState is not ChannelState.TRACKING:
            raise ValueError(f"channel {self.channelID} is not tracking: there is no state to reacquire from")
        bank, row = self._bank, self._row
        st = bank.state[row]
        slot, at = int(st["code_slot"]), int(st["current_sample"])
        hint = (at, float(st["rem_code"]), float(st["carrier_hz"]), float(st["code_step"]))
        bank.state[row] = np.zeros((), dtype=bank.state.dtype)
        bank.state["code_slot"][row], bank.state["current_sample"][row] = slot, at
        bank.lost[row] = False
        bank.code_since_tow[row], bank.tow[row], bank.tow_decoded[row], bank.host_flags[row] = 0, 0.0, False, 0
        bank.last["n_samples"][row] = 0
        del bank.nav_bits[row][:]
        if bank.decoders[row] is not None:
            bank.decoders[row].reset()
        self.trackFlags = TrackingFlags.UNKNOWN
        self.setTracking(self.configuration['TRACKING'])
        self.setWarmHint(*hint, chips=chips, chipStep=chipStep, spanHz=spanHz, stepHz=stepHz)
        self.channelState = ChannelState.ACQUIRING

    def trackingStart(self, acqIndices):
        """(coarse carrier, ring index of the sample tracking starts at) for a PCPS peak [bin, code sample]: what
        `enterTracking` is about to set, and what the fine search starts from."""
        start = self._firstEpochSample(int(np.round(acqIndices[1])))
        return self.rfSignal.interFrequency - self.searchedFrequency(acqIndices[0]), start % self.rfBuffer.maxSize

    def _firstEpochSample(self, code_offset: int) -> int:
        """The sample the first tracking epoch starts at (the searched samples are skipped, the first epoch
        is taken back, + offset + 1) -- ONE expression for `enterTracking` and for the fine search's window."""
        first_epoch = int(self._bank.state["n_samples"][self._row])
        return self.currentSample + self.acq_requiredSamples - first_epoch + code_offset + 1

    def fineFrequencyRequest(self, acqIndices):
        """This channel's sdr_refine_item (a batching manager refines a search group's channels in one call)."""
        carrier, start = self.trackingStart(acqIndices)
        return dict(code_slot=self.codeSlot, start_sample=start, carrier_hz=carrier, code_hz=GPS_L1CA_CODE_FREQ)

    def runFineFrequencySearch(self, acqIndices):
        """-> the sdr_refine_result row (fine_hz, power, power_no_edge, fine_idx, bit_edge) for this acquisition."""
        if self._injectedFine is not None:
            fine, self._injectedFine = self._injectedFine, None
            return fine
        r = self.fineFrequencyRequest(acqIndices)
        items = make_refine_items(r["code_slot"], r["start_sample"], r["carrier_hz"], r["code_hz"])
        return self._ensure_code().acq_refine(items, self.rfSignal.samplingFrequency, n_periods=self.acq_fineFrequencyMs,
                                              n_segments=self.FINE_FREQUENCY_SEGMENTS, span_hz=self.acq_dopplerSteps,
                                              step_hz=self.acq_fineFrequencyStep)[0]

    def searchedFrequency(self, bin_idx):
        """Frequency of Doppler bin `bin_idx` of this channel's search grid (np.arange(-range, range + 1, step))."""
        return -self.acq_dopplerRange + self.acq_dopplerSteps * bin_idx

    def enterTracking(self, carrier_hz: float, code_offset_samples: float):
        """From an acquisition result to the first tracking epoch: NCO carrier, and the sample at which the code period
        found at `code_offset_samples` into the searched slab begins (the searched samples are skipped,
        the first epoch is taken back, + offset + 1)."""
        self.codeOffset = int(np.round(code_offset_samples))
        self.carrierFrequency = carrier_hz
        self.currentSample = self._firstEpochSample(self.codeOffset)
        self.channelState = ChannelState.TRACKING

    def postAcquisitionUpdate(self, acqIndices):
        """PCPS peak [bin, code sample] -> NCO start values (kaplan:217-235 / borre:301-316)."""
        carrier = self.rfSignal.interFrequency - self.searchedFrequency(acqIndices[0])
        if self._acqFine is not None:                    # the fine search's frequency instead of the grid's bin
            carrier = float(self._acqFine["fine_hz"])
        self.enterTracking(carrier, acqIndices[1])

    def prepareResultsAcquisition(self, correlationMap, acqIndices, acqPeakRatio):
        packet = self.prepareResults()
        packet.update(type=ChannelMessage.ACQUISITION_UPDATE, carrierFrequency=self.carrierFrequency,
                      codeOffset=self.codeOffset, frequency_idx=acqIndices[0], code_idx=acqIndices[1],
                      correlation_map=correlationMap, peak_ratio=acqPeakRatio)
        if self._acqFine is not None:
            packet.update(fine_frequency_idx=int(self._acqFine["fine_idx"]), bit_edge=int(self._acqFine["bit_edge"]))
        if self._acqDeep is not None:                    # (correlation_map is the winning group's)
            packet.update(bit_edge_group=int(self._acqDeep["peak_group"]))
            self._acqDeep = None
        return packet

    # ------------------------------------------------------------------ tracking = one device step
    def runCorrelators(self):
        """The correlator seam (kaplan:378-401), kept for function-level use: the taps of the NEXT epoch for the
        current NCO state, open loop -- the state does not advance (runTracking / the manager's tick do that)."""
        return self._correlate()

    def correlationProfileItem(self):
        """The latest epoch of this channel as sdr_epl_item fields (code_slot, n_samples, start_sample, carrier_hz,
        rem_carrier, rem_code, code_step), from its record in the bank's `last` row: what the epoch's correlators ran with.
        ValueError when the channel has run no epoch yet (since it was given its satellite), when the device has parked
        it (`lostLock`: nothing guards the ring for it any more), or when the ring no longer holds that epoch's samples --
        the samples between the epoch's first one and the write index are then more than the ring's capacity (the
        channel's unread samples, which the manager never lets pass the capacity, plus the epoch itself).
        The last test reads the ring's write index: with read-ahead on (`ChannelManager.enableReadAhead`) the manager
        uploads whole blocks AHEAD of that index and protects unread samples only, so the epoch just read may have been
        overwritten although the index says otherwise -- profile from the per-tick loop or `runBlock`, not under
        read-ahead."""
        if self.lostLock:
            raise ValueError(f"channel {self.channelID} lost lock on the device: its last epoch is not kept in the ring")
        rec = self._bank.last[self._row]
        n = int(rec["n_samples"])
        if n <= 0:
            raise ValueError(f"channel {self.channelID} has run no tracking epoch yet: there is no epoch to profile")
        ring = self.rfBuffer
        unread = ring.getNbUnreadSamples((int(rec["start_sample"]) + n) % ring.maxSize)
        if unread + n > ring.maxSize:
            raise ValueError(f"the ring no longer holds the last epoch of channel {self.channelID} "
                             f"({n} samples, {unread} written behind it, ring of {ring.maxSize})")
        return (int(self._bank.state["code_slot"][self._row]), n, int(rec["start_sample"]), float(rec["carrier_hz_in"]),
                float(rec["rem_carrier_in"]), float(rec["rem_code_in"]), float(rec["code_step_in"]))

    def correlationProfile(self, first: float, step: float, n_taps: int):
        """The correlation function of this channel's LATEST epoch on the tap grid first + step * arange(n_taps) [chips]
        (sdr_corr_profile): the shape of the peak the channel tracks.  -> float64[n_taps, 2] = I, Q per tap; the grid
        (-0.5, 0.5, 3) gives the epoch's E, P, L again.  ValueError: see `correlationProfileItem`."""
        items = make_items(*self.correlationProfileItem())
        return self._bank.engine.corr_profile(items, first, step, n_taps, self.rfSignal.samplingFrequency)[0]

    def delayDopplerItem(self, nbMilliseconds: float):
        """The last `nbMilliseconds` of this channel, ending with its latest epoch, as sdr_epl_item fields for sdr_ddm: the
        item of `correlationProfileItem` carried BACK by the extra samples -- the code phase by back * code_step (the chips
        are indexed modulo the code length, so a negative rem_code is served), the carrier phase likewise.  ValueError as
        for `correlationProfileItem`, and when the ring does not hold the whole window (any more, or yet)."""
        slot, n, start, carrier, rem_carrier, rem_code, code_step = self.correlationProfileItem()
        fs, ring = self.rfSignal.samplingFrequency, self.rfBuffer
        W = max(n, int(round(fs * 1e-3 * nbMilliseconds)))
        back = W - n
        unread = ring.getNbUnreadSamples((start + n) % ring.maxSize)
        if unread + W > ring.size:
            raise ValueError(f"the ring does not hold the last {W} samples of channel {self.channelID} "
                             f"({unread} written behind them, {ring.size} held)")
        rem_carrier = (rem_carrier + carrier * 2.0 * np.pi * back / fs) % (2.0 * np.pi)
        return (slot, W, (start - back) % ring.maxSize, carrier, float(rem_carrier), rem_code - back * code_step, code_step)

    def runTracking(self):
        if self.lostLock or self.rfBuffer.getNbUnreadSamples(self.currentSample) < self.track_requiredSamples:
            return None
        rec, done = self._bank.step([self._row], 1)
        return tracking_packet(self.channelID, self.LOOP_KIND, rec[0, 0]) if done[0] else None
