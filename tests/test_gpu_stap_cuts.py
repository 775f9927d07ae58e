"""The space-time converter's two histories (sydr_amd/csrc/ddc.hip's history kernel with DdcStapLoad) against pushes of 0, 1,
Tp - 2, Tp - 1 and Tp frames: an element of the new history comes out of the block, or, of a push shorter than Tp - 1, further
up the old history; the raw tail the same way with its own length T_s - 1.

test_gpu_stap.py's cut test keeps to 8 taps per element and pushes none of Tp - 2 .. Tp; here the taps are 3 (T_s - 1 = 2:
shorter than most of the pushes) and 8 (longer than all of them), the shapes the smallest with Tp - 2 > 0 -- (T, D) = (5, 2):
Tp = 5; (L, M, T) = (3, 2, 7): Tp = 3 -- and the frames whole bytes (the K3_int8_complex geometry), so no length is rounded.
Without a mixer (fcw = 0) the converter's operations are the NumPy statement's own: the ring of the pieces, the ring of one push
and the statement are equal byte for byte, in a ci16 and in a cf64 ring."""
import numpy as np
import pytest

import array_cases as acases
import ddc_layout_cases as lcases
import downconvert_cases as dcases
import stap_cases as scases

from sydr_amd.engine import FMT_CF64, FMT_CI16
from sydr_amd.signal import stap

pytestmark = pytest.mark.gpu

N = 600
LAYOUT, LANES = acases.GEOMETRIES["K3_int8_complex"]
K = len(LANES)


def lengths(Tp: int) -> list:
    """Into a zero history, then -- behind 100 frames -- into a full one; then the rest."""
    short = [0, 1, Tp - 2, Tp - 1, Tp]
    return short + [100] + short


def assert_same_bytes(got, want, what):
    bad = np.flatnonzero(got.view(np.uint8) != want.view(np.uint8))
    assert bad.size == 0, (what, bad.size, bad[:5])
    assert np.any(want != 0), what


@pytest.mark.parametrize("shape", [(5, 2), (3, 2, 7)], ids=lcases.shape_id)
@pytest.mark.parametrize("T_s", [3, 8], ids=lambda t: f"taps{t}")
def test_pushes_of_0_1_and_around_the_history_length_give_the_ring_of_one_push_and_the_statement(engine, T_s, shape):
    Tp = lcases.phase_taps(shape)
    assert Tp - 2 > 0 and any(n > T_s - 1 for n in lengths(Tp)[:5]) == (T_s == 3)
    raw = acases.stream(LAYOUT, N)
    total = lcases.out_total(shape, N)
    for ring_fmt in (FMT_CI16, FMT_CF64):
        cfg = acases.config(shape, 0, acases.gain_for(LAYOUT, ring_fmt, K), LAYOUT, scases.geometry(LANES, T_s, scases.general_weights(T_s, K)))
        engine.iq_alloc(lcases.ring_capacity(total), ring_fmt)
        whole = lcases.push_all(engine, cfg, raw, total)
        engine.iq_upload(np.zeros(2 * engine.iq_capacity, dtype=whole.dtype), 0)
        ddc = engine.ddc_create(cfg)
        try:
            at = first = 0
            for n in lengths(Tp) + [None]:
                n = N - first if n is None else n
                at += engine.ddc_push(ddc, acases.piece(raw, LAYOUT, first, n), at)
                first += n
            assert at == total and first == N
            pieces = engine.iq_download(total, 0)
        finally:
            engine.ddc_destroy(ddc)
        what = (T_s, shape, dcases.RING_NAMES[ring_fmt])
        assert_same_bytes(pieces, whole, what + ("pieces against one push",))
        assert_same_bytes(whole, stap.statement(cfg, [raw], ring_fmt), what + ("one push against the statement",))
