"""Beams of a multi-antenna recording through ChannelManager (sdr_ddc_beam_attach): `leader.addBeam(weights)` gives the leader's
array or space-time converter one more weight set, whose stream goes into the ring of a further engine on the same device, and
returns the manager over that ring -- a FOLLOWER.  The leader's addNewRFData stays the one push per tick; it feeds every beam.

A follower is used like any manager (addChannel, requestTracking, run, runBlock, getChannel, correlationProfiles, ...).  Its ring
is fed by the leader: its own addNewRFData raises, its write index advances by the leader's outputs with every slab of the
leader, and it has no read-ahead -- the limits a converted recording has already.  What its ring holds is what an independent
converter with the beam's weights would have written (signal/array.py `beams_statement`)."""
from __future__ import annotations

import numpy as np

from .manager import ChannelManager


class BeamSignal:
    """The leader's recording as the manager of one of its beams sees it: every attribute the leader's channels see, but no front
    end (the leader feeds the ring) and the ring's own sample type."""
    frontEnd = None
    packing = None

    def __init__(self, rfSignal, output_bits: int):
        self._leader_signal = rfSignal
        self.fileDataType = np.int8 if int(output_bits) == 8 else np.int16

    def __getattr__(self, name):
        return getattr(self._leader_signal, name)


class BeamFollower(ChannelManager):
    def __init__(self, leader: ChannelManager, engine, beam: int, output_bits: int):
        size, per_ms = leader.sharedBuffer.maxSize, leader.rfSignal.samplingFrequency * 1e-3
        ring_ms = next((r for r in (round(size / per_ms), size / per_ms) if int(per_ms * r) == size), None)
        if ring_ms is None:
            raise ValueError(f"no ring length in milliseconds gives the leader's {size} samples")
        super().__init__(BeamSignal(leader.rfSignal, output_bits), engine=engine, keepCorrelationMap=leader.keepCorrelationMap, ring_ms=ring_ms)
        self.leader, self.beam = leader, int(beam)

    def addNewRFData(self, data):
        raise ValueError("a beam's ring is fed by its leader: call the leader's addNewRFData")

    def _upload_block(self, block, n_samples: int, offset: int):
        raise ValueError("a beam's ring is fed by its leader: blocks of the recording enter through the leader")

    def enableReadAhead(self, nbMilliseconds: int = 50):
        if int(nbMilliseconds) > 0:
            raise ValueError("read-ahead over a beam is not supported: its ring is fed by the leader's converter")
        return super().enableReadAhead(nbMilliseconds)

    def _guard_fed(self, count: int):
        """What addNewRFData checks before `count` samples enter the ring, for the leader's slab."""
        ring = self.sharedBuffer
        if ring.maxSize % count:
            raise ValueError("Data shift need to be a multiple from the max buffer size.")
        if ring.full and (self._unread_max is None or self._unread_max + count > ring.maxSize):
            self._guard_unread(count)

    def _fed(self, count: int):
        """The leader has queued `count` outputs for this ring, ordered ahead of whatever this manager's engine launches next."""
        self._unread_max = None
        self._pending = True
        self.sharedBuffer.shiftIdxWrite(count)


def _fan_out(leader: ChannelManager, data):
    """The leader's addNewRFData once it has beams: the converting one, told to and answered for every follower."""
    data, n_in = leader._raw_input(data)
    D, L = leader._frontEnd.decimation, leader._frontEnd.interpolation
    count = n_in * L // D if n_in and not n_in * L % D else 0
    if count:                                   # (everything else the leader's own route refuses, before a follower moves)
        for f in leader._beams:
            f._guard_fed(count)
    leader._addNewRFData_converted(data)
    for f in leader._beams:
        f._fed(count)


def add_beam(leader: ChannelManager, weights, output_bits=None, engine=None) -> BeamFollower:
    fe = leader._frontEnd
    if fe is not None and fe.mitigation is not None:
        raise ValueError("beams beside mitigation keys are not supported: the mitigator's state is per stream")
    if fe is None or getattr(fe, "array", None) is None or leader._ddc is None:
        raise ValueError("addBeam needs a recording whose front end is an array or space-time converter")
    if isinstance(leader, BeamFollower):
        raise ValueError("a beam is added to the leader")
    if leader.sharedBuffer.size or leader.sharedBuffer.idxWrite or leader.sharedBuffer.full:
        raise ValueError("addBeam comes before the first addNewRFData")
    bits = fe.outputBits if output_bits is None else int(output_bits)
    if bits not in (8, 16):
        raise ValueError("a beam's ring holds 8- or 16-bit samples")
    own = engine is None
    if own:
        engine = type(leader.engine)(getattr(leader.engine, "device_id", 0))
    beams = getattr(leader, "_beams", None)
    try:
        follower = BeamFollower(leader, engine, (len(beams) if beams else 0) + 1, bits)
        follower.beam = leader.engine.ddc_beam_attach(leader._ddc, engine, weights)
    except Exception:
        if own:
            engine.close()
        raise
    follower._owns_engine = own
    if beams is None:
        leader._beams = []
        leader.addNewRFData = lambda data: _fan_out(leader, data)
    leader._beams.append(follower)
    return follower


def close_beams(leader: ChannelManager):
    """Behind the leader's converter (whose destruction released the attachments): the followers, then the engines made for them."""
    for f in getattr(leader, "_beams", ()):
        f.close()
        if f._owns_engine:
            f.engine.close()
    leader._beams = []
