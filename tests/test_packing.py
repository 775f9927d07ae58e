"""Packed 1-, 2- and 4-bit I,Q recordings, everything that needs no GPU: the format module against a per-field loop, the
host helper of the C-ABI, RFSignal over packed files, the manager's packed route over the oracle-backed engine (packets
equal to those of the same levels stored as int8), the unpack kernels' lane arithmetic run on the host, the packing tool."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from oracle import sydr_oracle as orc
from fake_engine import OracleEngine
import packed_cases as cases
import host_check

from sydr_amd import _lib
from sydr_amd.signal import packing as pk
from sydr_amd.signal.iqsource import RFSignal
from sydr_amd.utils.enumerations import ChannelMessage

ALL = [(bits, msb) for bits in (1, 2, 4) for msb in (False, True)]


def random_table(rng, bits):
    """A one-to-one table drawn from all of int8, -128 and 127 among its levels."""
    levels = rng.choice(np.arange(-127, 127), (1 << bits) - 2, replace=False).tolist() + [-128, 127]
    return [int(v) for v in rng.permutation(levels)]


# ---------------------------------------------------------------------------------------------- 1. the format module
@pytest.mark.parametrize("bits,msb", ALL)
def test_pack_and_unpack_are_inverse_and_agree_with_the_per_field_loop(bits, msb):
    rng = np.random.default_rng(100 * bits + msb)
    for _ in range(5):
        levels = random_table(rng, bits)
        p = pk.Packing(bits, levels, msb_first=msb)
        v = np.array(levels, dtype=np.int8)[rng.integers(0, 1 << bits, 2 * 8 * 300)]
        packed = pk.pack(v, p)
        assert packed.dtype == np.uint8 and packed.size == pk.packed_bytes(p, v.size // 2) == v.size * bits // 8
        assert np.array_equal(pk.unpack(packed, p), v)
        assert np.array_equal(pk.unpack(packed, p, 8), v[:16])               # (the first samples of a longer slab)
        blob = rng.integers(0, 256, 37).astype(np.uint8)                     # any bytes are a valid slab
        assert np.array_equal(pk.unpack(blob, p), cases.per_field_unpack(blob, bits, levels, msb))
        assert np.array_equal(pk.pack(pk.unpack(blob, p), p), blob)
    # one byte by hand: 2 bits, the default sign / magnitude table (1, 3, -1, -3)
    assert pk.unpack(np.array([0b11100100], np.uint8), pk.Packing(2)).tolist() == [1, 3, -1, -3]
    assert pk.unpack(np.array([0b11100100], np.uint8), pk.Packing(2, msb_first=True)).tolist() == [-3, -1, 3, 1]
    assert pk.unpack(np.array([0b00000110], np.uint8), pk.Packing(1)).tolist() == [1, -1, -1, 1, 1, 1, 1, 1]
    assert pk.unpack(np.array([0x8F], np.uint8), pk.Packing(4)).tolist() == [-1, -8]


def test_tables_defaults_and_refusals():
    assert pk.DEFAULT_LEVELS == {1: (1, -1), 2: (1, 3, -1, -3), 4: tuple(range(8)) + tuple(range(-8, 0))}
    for bits in (1, 2, 4):
        assert pk.Packing(bits).levels.tolist() == list(pk.DEFAULT_LEVELS[bits])
        assert pk.packed_bytes(pk.Packing(bits), 64) == 64 * 2 * bits // 8
    for bad in (0, 3, 8, 12):
        with pytest.raises(ValueError):
            pk.Packing(bad)
    with pytest.raises(ValueError):
        pk.Packing(2, (1, 3, -1))                                            # three levels for four codes
    with pytest.raises(ValueError):
        pk.Packing(1, (1, 200))                                              # not int8
    with pytest.raises(ValueError):
        pk.packed_bytes(pk.Packing(1), 6)                                    # four samples to a byte
    with pytest.raises(ValueError):
        pk.packed_bytes(pk.Packing(2), 3)
    # repeated levels: every code still has a value, but a value has no one code
    rep = pk.Packing(2, (5, 5, -5, -5))
    assert pk.unpack(np.array([0b11100100], np.uint8), rep).tolist() == [5, 5, -5, -5]
    with pytest.raises(ValueError, match="repeated"):
        pk.pack(np.array([5, -5, 5, -5], np.int8), rep)
    with pytest.raises(ValueError, match="none of"):
        pk.pack(np.array([1, 2, 1, 1], np.int8), pk.Packing(2))


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_quantise_produces_only_table_values(bits):
    rng = np.random.default_rng(bits)
    raw = np.clip(rng.normal(0, 20, 20000), -128, 127).astype(np.int8)
    few = pk.quantise(raw, bits, 5.0 if bits == 4 else 20.0)
    assert few.dtype == np.int8 and set(few.tolist()) <= set(pk.DEFAULT_LEVELS[bits])
    assert len(set(few.tolist())) == 1 << bits                               # ... and all of them at this threshold
    assert np.array_equal(np.sign(few[raw != 0]), np.sign(raw[raw != 0])) or bits == 4   # (4 bits: 0 is a level)
    if bits == 2:
        assert np.array_equal(np.abs(few) == 3, (raw >= 20) | (raw < -20))
    table = random_table(rng, bits)
    assert set(pk.quantise(raw, bits, 11.0, pk.Packing(bits, table)).tolist()) <= set(table)
    assert np.array_equal(pk.unpack(pk.pack(few, pk.Packing(bits)), pk.Packing(bits)), few)


# ---------------------------------------------------------------------------------------------- 2. the C-ABI's host helper
def test_packed_bytes_helper_of_the_library_and_struct_size(tmp_path):
    lib = _lib.load()
    assert C.sizeof(_lib.IqPacking) == 24
    for bits in (1, 2, 4):
        for flags in (0, _lib.PACK_MSB_FIRST):
            p = _lib.IqPacking(bits, flags)
            for n in (0, 4, 8, 25000, 1 << 30):
                assert lib.sdr_iq_packed_bytes(C.byref(p), n) == n * 2 * bits // 8
            assert lib.sdr_iq_packed_bytes(C.byref(p), -4) < 0
    assert lib.sdr_iq_packed_bytes(C.byref(_lib.IqPacking(1, 0)), 6) < 0       # not a multiple of four samples
    assert lib.sdr_iq_packed_bytes(C.byref(_lib.IqPacking(2, 0)), 7) < 0
    assert lib.sdr_iq_packed_bytes(C.byref(_lib.IqPacking(4, 0)), 7) == 7
    for bits in (0, 3, 8, 16, -1):
        assert lib.sdr_iq_packed_bytes(C.byref(_lib.IqPacking(bits, 0)), 8) == -1
        assert b"bits" in lib.sdr_last_error()
    assert lib.sdr_iq_packed_bytes(C.byref(_lib.IqPacking(2, 2)), 8) == -1     # an unknown flag
    assert lib.sdr_iq_packed_bytes(None, 8) == -1
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %d\\n",'
                   "sizeof(sdr_iq_packing),offsetof(sdr_iq_packing,levels),SDR_PACK_MSB_FIRST);return 0;}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "size")])
    assert subprocess.check_output([str(tmp_path / "size")]).split() == [b"24", b"8", b"1"]
    assert _lib.IqPacking.levels.offset == 8


# ---------------------------------------------------------------------------------------------- 3. RFSignal
@pytest.mark.parametrize("bits,msb", ALL)
def test_rfsignal_serves_a_packed_recording(tmp_path, bits, msb):
    rng = np.random.default_rng(7 * bits + msb)
    levels = random_table(rng, bits)
    p = pk.Packing(bits, levels, msb_first=msb)
    n_ms, spms = 130, 4000
    packed = rng.integers(0, 256, pk.packed_bytes(p, n_ms * spms)).astype(np.uint8)
    values = pk.unpack(packed, p)
    cplx = values[0::2].astype(np.float64) + 1j * values[1::2].astype(np.float64)
    path = tmp_path / "iq.bin"
    packed.tofile(path)
    sig = cases.signal(path, 4e6, bits, p)
    assert sig.packing == p and sig.fileDataType is np.uint8 and sig.dtype == np.complex128
    assert sig.samplesPerMs == spms and sig.totalSamples == n_ms * spms
    per_ms = spms * 2 * bits // 8
    first = sig.getMilliseconds(1)
    assert first.dtype == np.uint8 and np.array_equal(first, packed[:per_ms]) and np.shares_memory(first, sig._recording())
    assert np.array_equal(sig.getMilliseconds(1, raw=False), cplx[spms:2 * spms])
    assert np.array_equal(sig.getMilliseconds(7), packed[2 * per_ms:9 * per_ms]) and sig.position == 9 * spms
    view = sig.samples(3 * spms, 2 * spms)
    assert np.array_equal(view, packed[3 * per_ms:5 * per_ms]) and np.shares_memory(view, sig._recording())
    assert np.shares_memory(sig.slab(spms), sig._recording())
    sig.seek(120 * spms)
    assert np.array_equal(sig.getMilliseconds(10), packed[120 * per_ms:])
    with pytest.raises(EOFError):
        sig.getMilliseconds(1)
    # the reference's cursor calls
    rd = cases.signal(path, 4e6, bits, p)
    with pytest.raises(Warning):
        rd.getCurrentSampleIndex()
    a = rd.readFile(timeLength=2, keep_open=True)
    assert a.dtype == np.complex128 and np.array_equal(a, cplx[:2 * spms]) and rd.getCurrentSampleIndex() == 2 * spms
    b = rd.readFileBySamples(100, skip=50, keep_open=True)              # (the numbers of tests/test_host_layer.py: any sample, any count)
    assert np.array_equal(b, cplx[2 * spms + 50:2 * spms + 150]) and rd.getCurrentSampleIndex() == 2 * spms + 150
    rd.closeFile()
    with pytest.raises(Warning):
        rd.closeFile()
    assert np.array_equal(rd.readFileBySamples(10, skip=3), cplx[3:13])    # complex samples need no whole bytes
    c = rd.readFileBySamples(12, skip=4, raw=True)
    assert c.dtype == np.uint8 and np.array_equal(pk.unpack(c, p), values[8:32]) and np.shares_memory(c, rd._recording())
    assert rd.readFile(timeLength=1, skip=n_ms * spms - 10).size == 10     # a short read at the end of the file
    assert rd.readFile(timeLength=1, skip=n_ms * spms).size == 0
    sig.seek(4001)                                                       # a cursor inside a byte (1 and 2 bits)
    assert np.array_equal(sig.getMilliseconds(1, raw=False), cplx[4001:4001 + spms]) and sig.position == 4001 + spms
    assert np.array_equal(sig.slab(7, raw=False), cplx[4001 + spms:4008 + spms])
    if bits < 4:                                                         # ... where no VIEW of packed bytes can begin
        with pytest.raises(ValueError, match="whole bytes"):
            rd.samples(1, 4)
        with pytest.raises(ValueError, match="whole bytes"):
            rd.readFileBySamples(10, skip=3, raw=True)
        sig.seek(4001)
        with pytest.raises(ValueError, match="whole bytes"):
            sig.getMilliseconds(1)
    # a packing does not change under the engine that keeps its C image
    with pytest.raises(ValueError):
        p.levels[0] = 5


def test_rfsignal_packed_configuration_refusals(tmp_path):
    conf = dict(filepath="x", sampling_frequency=4e6, is_complex="true", intermediate_frequency=0)
    assert RFSignal(dict(conf, data_size=2)).packing == pk.Packing(2)        # the default table, least significant first
    assert RFSignal(dict(conf, data_size=2, bit_order="MSB")).packing == pk.Packing(2, msb_first=True)
    assert RFSignal(dict(conf, data_size=2, sample_levels="-3, -1, 1, 3")).packing == pk.Packing(2, (-3, -1, 1, 3))
    assert RFSignal(dict(conf, data_size=8)).packing is None and RFSignal(dict(conf, data_size=16)).packing is None
    with pytest.raises(ValueError):
        RFSignal(dict(conf, data_size=12))
    with pytest.raises(ValueError):
        RFSignal(dict(conf, data_size=3))
    with pytest.raises(ValueError):
        RFSignal(dict(conf, data_size=2, sample_levels="1,3,-1"))            # three levels for four codes
    with pytest.raises(ValueError):
        RFSignal(dict(conf, data_size=2, bit_order="middle"))
    with pytest.raises(ValueError, match="whole number of bytes"):
        RFSignal(dict(conf, data_size=1, sampling_frequency=4.002e6))        # 4002 samples per millisecond, four to a byte
    with pytest.raises(ValueError, match="whole number of bytes"):
        RFSignal(dict(conf, data_size=2, sampling_frequency=4.001e6))
    assert RFSignal(dict(conf, data_size=4, sampling_frequency=4.001e6)).samplesPerMs == 4001
    with pytest.raises(ValueError):
        RFSignal(dict(conf, data_size=2, is_complex=""))                     # packed recordings are I,Q too


# ---------------------------------------------------------------------------------------------- 4. the manager
class PackedOracleEngine(OracleEngine):
    """The oracle-backed engine with the packed entry points: unpack on the host, then the unpacked namesake -- the statement
    the device's kernels are held to (tests/test_gpu_packed.py).  `_begin` / `sync` make the manager defer slabs as it does
    on the device."""

    def __init__(self):
        super().__init__()
        self.packed_calls = dict(sync=0, begin=0)

    def iq_upload_packed(self, packed, n_samples, packing, ring_offset=0):
        assert packed.dtype == np.uint8 and packed.size == pk.packed_bytes(packing, n_samples)
        self.packed_calls["sync"] += 1
        self.iq_upload(pk.unpack(packed, packing), ring_offset)

    def iq_upload_packed_begin(self, packed, n_samples, packing, ring_offset=0):
        assert packed.dtype == np.uint8 and packed.size == pk.packed_bytes(packing, n_samples)
        self.packed_calls["begin"] += 1
        self.iq_upload(pk.unpack(packed, packing), ring_offset)

    iq_upload_packed_queue = iq_upload_packed

    def iq_upload_begin(self, raw, ring_offset=0):
        self.iq_upload(raw, ring_offset)

    def sync(self):
        pass


@pytest.fixture(scope="module")
def two_satellites():
    fs, ms = 4e6, 300
    sats = [dict(prn=7, doppler=1750.0, code_phase=300.25, phase=0.1, amp=30.0),
            dict(prn=19, doppler=-2250.0, code_phase=811.5, phase=0.6, amp=25.0)]
    raw = orc.synth_iq(fs, ms * int(fs * 1e-3), sats, 10.0, 20261041)
    return fs, ms, raw


@pytest.mark.parametrize("mode", ["ticks", "readahead", "block"])
def test_manager_over_a_packed_file_equals_the_same_levels_as_int8(tmp_path, two_satellites, mode):
    """One few-level stream written twice -- 2 bits packed (`data_size = 2`) and int8 of the same levels (`data_size = 8`):
    equal packets, key by key, bit for bit, through plain ticks, read-ahead blocks and runBlock, a channel joining late."""
    fs, ms, raw = two_satellites
    threshold = float(raw.astype(np.float64).std())
    packed_path, plain_path, packing, few = cases.write_both(tmp_path, raw, 2, threshold)
    assert os.path.getsize(packed_path) * 4 == os.path.getsize(plain_path) == few.size
    cfg = cases.kaplan_config(noncoh=3)
    kw = dict(prns=[7], cfg=cfg, ms=ms, mode=mode, late=(70, [19]), ring_ms=400 if mode == "block" else 100, keep_map=(mode == "ticks"))
    eng = PackedOracleEngine()
    got, mgr = cases.receive(cases.signal(packed_path, fs, 2), eng, **kw)
    want, want_mgr = cases.receive(cases.signal(plain_path, fs, 8), PackedOracleEngine(), **kw)
    assert mgr.sharedBuffer.fmt == 0 and mgr.sharedBuffer.rawDtype == np.int8       # a ci8 ring
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, k
    assert cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 2                  # both satellites found ...
    assert cases.count(got) > (400 if mode != "block" else 300)                      # ... and tracked
    assert eng.packed_calls["begin"] + eng.packed_calls["sync"] > 0
    assert np.array_equal(eng.ring, want_mgr.engine.ring)
    if mode == "ticks":
        assert eng.packed_calls["begin"] == ms                                       # every slab deferred, as int8 slabs are
    if mode == "readahead":
        assert eng.bank_calls["step"] > 5 and eng.packed_calls["sync"] > 5          # blocks of packed bytes went up
    # an int8 or complex array handed to the manager of a packed recording keeps working as before
    mgr2 = cases.ChannelManager(cases.signal(packed_path, fs, 2), engine=PackedOracleEngine())
    spms = int(fs * 1e-3)
    mgr2.addNewRFData(few[:2 * spms])
    mgr2.addNewRFData(few[2 * spms:4 * spms:2].astype(np.float64) + 1j * few[2 * spms + 1:4 * spms:2])
    mgr2._flush_pending()
    assert np.array_equal(mgr2.engine.iq_download(2 * spms, 0), few[:4 * spms])


# ---------------------------------------------------------------------------------------------- 5. the lane arithmetic
@host_check.requires_hipcc
def test_unpack_lane_arithmetic_on_the_host():
    """sydr_amd/csrc/unpack_lanes.h, the code the unpack kernels' lanes run, compiled for the host alone: every byte value
    x position x order x width with hostile tables equals the per-field statement."""
    exe = host_check.build("unpack_lanes_check")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) == 6 * 2 * 256 * (2 + 4 + 8)


# ---------------------------------------------------------------------------------------------- 6. the tool
def test_pack_recording_tool_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    raw = np.clip(rng.normal(0, 25, 2 * 40000), -128, 127).astype(np.int8)
    raw.tofile(tmp_path / "in.bin")
    tool = os.path.join(REPO, "tools", "pack_recording.py")
    run = lambda *a: subprocess.run([sys.executable, tool, *map(str, a)], capture_output=True, text=True, check=True).stdout
    out = run(tmp_path / "in.bin", tmp_path / "p2.bin", "--bits", 2, "--threshold", 25)
    assert "40000 samples" in out
    packed = np.fromfile(tmp_path / "p2.bin", dtype=np.uint8)
    few = pk.quantise(raw, 2, 25.0)
    assert np.array_equal(packed, pk.pack(few, pk.Packing(2)))
    run(tmp_path / "p2.bin", tmp_path / "back.bin", "--bits", 2, "--unpack")
    assert np.array_equal(np.fromfile(tmp_path / "back.bin", dtype=np.int8), few)
    # packing what is few-level already, another table and order: the same file again
    run(tmp_path / "back.bin", tmp_path / "p2m.bin", "--bits", 2, "--exact", "--msb", "--levels=-3,-1,1,3")
    p = pk.Packing(2, (-3, -1, 1, 3), msb_first=True)
    assert np.array_equal(pk.unpack(np.fromfile(tmp_path / "p2m.bin", dtype=np.uint8), p), few)
    # int16 in, 4 bits, streamed in chunks smaller than the file
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import pack_recording
    raw16 = (raw.astype(np.int16) * 40)
    raw16.tofile(tmp_path / "in16.bin")
    n, thr = pack_recording.convert(tmp_path / "in16.bin", tmp_path / "p4.bin", pk.Packing(4), 400.0, int16=True, chunk=4096)
    assert n == 40000 and thr == 400.0
    assert np.array_equal(pk.unpack(np.fromfile(tmp_path / "p4.bin", dtype=np.uint8), pk.Packing(4)), pk.quantise(raw16, 4, 400.0))
