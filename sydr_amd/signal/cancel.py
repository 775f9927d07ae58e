"""Successive interference cancellation on the ring: the statement of `sdr_iq_cancel` (include/sydr_amd.h) in NumPy.

A strongly tracked signal is rebuilt from what its tracking loop already knows -- the NCO inputs of every epoch (an
`sdr_epl_item`) and a complex amplitude per epoch -- and subtracted from the samples; a search for a weak signal then runs on
the residue, where the strong one's cross-correlation peaks (only ~24 dB under its own peak for the C/A Gold codes) are gone.

`cancel_statement` is the definition the device is held against (`Engine.iq_cancel`, tests/test_gpu_cancel.py).  Per item with
n = n_samples, L chips c staged in its slot and amplitude A = a_re + j*a_im, sample i = 0..n-1 gets the prompt tap of the
reference's EPL (sydr/dsp/tracking.py:92-116) in its operation order:

    t_i     = np.arange(0.0, n) / fs
    theta_i = -(carrier_hz * 2.0 * np.pi * t_i) + rem_carrier
    idx_i   = ceil(linspace(rem_code + 0.0, code_step*n + rem_code + 0.0, n, endpoint=False))
    chip_i  = c[(idx_i - 1) mod L]
    r_re    = chip_i * (a_re*cos(theta_i) + a_im*sin(theta_i))
    r_im    = chip_i * (a_im*cos(theta_i) - a_re*sin(theta_i))            # A * chip * conj(replica)

(cos, sin) = np.exp(1j * theta), as the reference builds its replica.  A window sample m with ring value x widened to fp64
becomes y = x; for ch = 0 .. n_ch-1 in this order: if an item of ch covers m: y_re -= r_re; y_im -= r_im -- and is stored in
the ring's format.  A sample no item covers is copied as it is.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .._lib import EPL_ITEM_DTYPE, FMT_CF32, FMT_CF64, FMT_CI16, FMT_CI8

MAX_CHANNELS = 64
_RAIL = {FMT_CI8: 127.0, FMT_CI16: 32767.0}     # the rails of sdr_ddc_push's integer rings: symmetric

# window: complex128[W], the values the ring then holds; stats: the three counters of sdr_cancel_stats; pre: complex128[W],
# the fp64 values in front of the store; covered: bool[W], samples at least one item covers
CancelResult = namedtuple("CancelResult", "window stats pre covered")


def amplitudes_from_prompts(prompt_iq, n_samples):
    """prompt / n: the least-squares amplitude of the replica over the epoch (chip^2 = |replica|^2 = 1, so the normal
    equation is A * n = sum chip * replica * x = the prompt).  It carries the data bit's sign and the carrier phase; the
    prompt of the same item on the cancelled samples is then P - A*n = 0 to rounding.  prompt_iq[..., 2] = I, Q;
    n_samples[...]; padding (n = 0) gets 0."""
    p = np.asarray(prompt_iq, dtype=np.float64)
    n = np.asarray(n_samples, dtype=np.float64)[..., None]
    return np.where(n > 0, p / np.where(n > 0, n, 1.0), 0.0)


def items_from_records(records, code_slots, n_taps=3):
    """`sdr_track_epoch` records [n_ch][n_epochs] (what `Bank.step` and `track_closed_loop*` return) -> (items
    [n_ch][n_epochs], amps [n_ch][n_epochs][2], (w0, W)): each epoch's NCO inputs as the loop had them, the centre tap of its
    `corr` over n_samples as amplitude, and the hull window of all the items.  code_slots[n_ch]: the slot of each channel."""
    rec = np.asarray(records)
    if rec.ndim == 1:
        rec = rec[None, :]
    slots = np.broadcast_to(np.asarray(code_slots, dtype=np.int32).reshape(-1, 1), rec.shape)
    items = np.zeros(rec.shape, dtype=EPL_ITEM_DTYPE)
    items["code_slot"] = slots
    for dst, src in (("n_samples", "n_samples"), ("start_sample", "start_sample"), ("carrier_hz", "carrier_hz_in"),
                     ("rem_carrier", "rem_carrier_in"), ("rem_code", "rem_code_in"), ("code_step", "code_step_in")):
        items[dst] = rec[src]
    centre = n_taps // 2
    amps = amplitudes_from_prompts(rec["corr"][..., 2 * centre:2 * centre + 2], rec["n_samples"])
    return items, amps, hull(items)


def hull(items):
    """(w0, W): the smallest window that holds every item with n_samples > 0 (start_sample taken as it stands)."""
    it = np.asarray(items).reshape(-1)
    it = it[it["n_samples"] > 0]
    if not len(it):
        raise ValueError("no item with samples")
    w0 = int(it["start_sample"].min())
    return w0, int((it["start_sample"] + it["n_samples"]).max()) - w0


def window_offsets(items, w0, capacity):
    """off = (start_sample - w0) mod capacity of every item (capacity None: the window is not a ring's)."""
    d = np.asarray(items["start_sample"], dtype=np.int64) - int(w0)
    return d if capacity is None else d % int(capacity)


def replica(item, amp, code, fs):
    """(r_re, r_im, theta) of one item, float64[n] each: the text of the module's docstring."""
    n = int(item["n_samples"])
    carrier_hz, rem_carrier = float(item["carrier_hz"]), float(item["rem_carrier"])
    rem_code, code_step = float(item["rem_code"]), float(item["code_step"])
    a_re, a_im = float(amp[0]), float(amp[1])
    code = np.asarray(code, dtype=np.float64)
    t = np.arange(0.0, n) / fs
    theta = -(carrier_hz * 2.0 * np.pi * t) + rem_carrier
    idx = np.ceil(np.linspace(rem_code + 0.0, code_step * n + rem_code + 0.0, n, endpoint=False)).astype(np.int64)
    chip = code[(idx - 1) % len(code)]
    e = np.exp(1j * theta)
    cos, sin = e.real, e.imag
    r_re = chip * (a_re * cos + a_im * sin)
    r_im = chip * (a_im * cos - a_re * sin)
    return r_re, r_im, theta


def cancel_statement(ring_window, fmt, channels, fs, w0=0, capacity=None):
    """ring_window: complex128[W], the window's samples in window order (the ring's values, widened); fmt: the ring's format;
    channels: a sequence of (items[n_epochs], amps[n_epochs][2], code[L]) -- `code` the +-1 chips staged in the items' slot;
    w0 / capacity: the window's first ring index and the ring's size (an item sits at (start_sample - w0) mod capacity).
    -> CancelResult.  ValueError for what the call refuses."""
    x = np.asarray(ring_window, dtype=np.complex128)
    W = len(x)
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"{len(channels)} channels outside 1..{MAX_CHANNELS}")
    y_re, y_im = x.real.copy(), x.imag.copy()
    covered = np.zeros(W, dtype=bool)
    for items, amps, code in channels:
        items = np.asarray(items).reshape(-1)
        amps = np.asarray(amps, dtype=np.float64).reshape(len(items), 2)
        offs = window_offsets(items, w0, capacity)
        end = 0
        for it, amp, off in zip(items, amps, offs):
            n, off = int(it["n_samples"]), int(off)
            if n == 0:
                continue
            if n < 0 or not np.all(np.isfinite(amp)) or not float(it["code_step"]) > 0.0:
                raise ValueError("bad item")
            if off + n > W:
                raise ValueError(f"an item at window offset {off} of {n} samples leaves the window of {W}")
            if off < end:
                raise ValueError("a channel's items overlap or do not ascend")
            end = off + n
            r_re, r_im, _ = replica(it, amp, code, fs)
            y_re[off:end] -= r_re
            y_im[off:end] -= r_im
            covered[off:end] = True
    pre = y_re + 1j * y_im
    out_re, out_im = x.real.copy(), x.imag.copy()
    clipped = 0
    if fmt in _RAIL:
        lim = _RAIL[fmt]
        for out, y in ((out_re, y_re), (out_im, y_im)):
            r = np.rint(y[covered])
            clipped += int(np.count_nonzero(np.abs(r) > lim))
            out[covered] = np.clip(r, -lim, lim)
    elif fmt == FMT_CF32:
        with np.errstate(over="ignore", invalid="ignore"):
            out_re[covered] = y_re[covered].astype(np.float32)
            out_im[covered] = y_im[covered].astype(np.float32)
    else:
        out_re[covered], out_im[covered] = y_re[covered], y_im[covered]
    stats = dict(samples_written=W, samples_changed=int(np.count_nonzero(covered)), clipped_components=clipped)
    return CancelResult(out_re + 1j * out_im, stats, pre, covered)


# ------------------------------------------------------------------------------------------------ the device's distance
EPS = 2.0 ** -53          # half an ulp of 1: the relative error of one fp64 rounding


def trig_error(theta_max):
    """|cos, sin of the device - of np.exp| per component at |theta| <= theta_max (docs/notes/cancel.md):
    np.exp(1j*theta) is libm's sincos, under one ulp of a value of at most 1: 2 EPS;
    sincos_reduced: the reduced phase t = theta - k*pi/2 carries two FMA roundings of a value under 1 (EPS each) and k
    times what the two-word pi/2 leaves out (< 2^-107); its degree-13 / 14 kernels stay under one ulp: 2 EPS more."""
    k = np.ceil(abs(theta_max) * 2.0 / np.pi) + 1.0
    return 2.0 * EPS + (2.0 * EPS + k * 2.0 ** -107) + 2.0 * EPS


def parity_bound(fmt, amp_sum, theta_max, y_max, n_cover):
    """How far a component the device stores may lie from the statement's, for a sample that n_cover channels with
    sum |a_re| + |a_im| = amp_sum cover and whose partial sums stay under y_max in magnitude.
    fp64 part: per channel (|a_re| + |a_im|) * trig_error for the two trigonometric inputs, 3 EPS of the same for the two
    products and the sum that then round differently, EPS * y_max for the subtraction.  A cf32 ring adds one float ulp of
    y_max (two doubles that close may round to neighbouring floats); an integer ring adds nothing here: its tests demand
    that the statement's value keeps more than the fp64 part from a tie and then equality."""
    d = amp_sum * (trig_error(theta_max) + 3.0 * EPS) + n_cover * EPS * y_max
    if fmt == FMT_CF32:
        d += 2.0 ** -23 * y_max
    return d


__all__ = ["MAX_CHANNELS", "CancelResult", "amplitudes_from_prompts", "items_from_records", "hull", "window_offsets",
           "replica", "cancel_statement", "trig_error", "parity_bound", "FMT_CI8", "FMT_CI16", "FMT_CF32", "FMT_CF64"]
