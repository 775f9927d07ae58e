"""Input layouts of the down-converter (packed, float32 and interleaved recordings), everything that needs no GPU: `decode`
against `packing.unpack` and plain NumPy views; the statement with a layout against the statement with the old format on the
decoded integers, bit for bit; `bytes_for`; the [RFSIGNAL] keys and their refusals; the manager's route over a packed real
recording (oracle-backed engine); the C struct and sdr_ddc_layout_bytes; the shared field arithmetic run on the host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
import downconvert_cases as dcases
import host_check
import ddc_layout_cases as cases
import packed_cases
from test_downconvert import ConvertingOracleEngine

from sydr_amd import _lib
from sydr_amd.channel.manager import ChannelManager
from sydr_amd.engine import layout_struct
from sydr_amd.signal import downconvert as dc
from sydr_amd.signal import packing as pk
from sydr_amd.signal.iqsource import RFSignal
from sydr_amd.utils.enumerations import ChannelMessage

INVALID = -1


# ---------------------------------------------------------------------------------------------- 1. decode
@pytest.mark.parametrize("bits", [1, 2, 4])
@pytest.mark.parametrize("msb_first", [False, True], ids=["lsb", "msb"])
def test_decode_of_packed_fields_equals_unpack(bits, msb_first):
    levels = cases.ODD_TABLE if bits == 2 and msb_first else None
    rng = np.random.default_rng(cases.SEED + bits)
    raw = rng.integers(0, 256, 72 * 35).astype(np.uint8)              # (whole frames of every stride below: 72 * 35 * 8 bits)
    f = pk.unpack(raw, pk.Packing(bits, levels, msb_first))
    assert np.array_equal(f[:64 * (8 // bits)], packed_cases.per_field_unpack(raw[:64], bits, pk.Packing(bits, levels, msb_first).levels, msb_first))
    for stride in (1, 2, 3, 4, 5, 7, 9):
        for lane in range(stride):
            lay = dc.InputLayout(dc.FIELD_PACKED, bits, stride, lane, False, False, msb_first, levels)
            xr, xi = dc.decode(raw, lay)
            n = raw.size * 8 // (stride * bits)
            assert xr.dtype == xi.dtype == np.float64 and xr.size == xi.size == n
            assert np.array_equal(xr, f[lane::stride][:n]) and not xi.any()
            if lane + 2 <= stride:
                for swap in (False, True):
                    lay = dc.InputLayout(dc.FIELD_PACKED, bits, stride, lane, True, swap, msb_first, levels)
                    a, b = f[lane::stride][:n].astype(np.float64), f[lane + 1::stride][:n].astype(np.float64)
                    xr, xi = dc.decode(raw, lay)
                    assert np.array_equal(xr, b if swap else a) and np.array_equal(xi, a if swap else b)


def test_decode_of_frames_that_are_not_whole_bytes():
    # 1-bit stride 3 lane 1 real: input j is bit 3 j + 1 of the stream
    raw = np.array([0b10110100, 0b01001011, 0b11100001], dtype=np.uint8)
    bits = np.unpackbits(raw, bitorder="little")
    xr, xi = dc.decode(raw, cases.packed_layout(1, stride=3, lane=1))
    assert xr.tolist() == [1.0 - 2.0 * int(bits[3 * j + 1]) for j in range(8)] and not xi.any()
    # 4-bit stride 3 lane 1 complex: frame 0 is nibbles 0..2, I = nibble 1 (the HIGH nibble of byte 0), Q = nibble 2 (the LOW
    # nibble of byte 1); frame 1 is nibbles 3..5: I = low nibble of byte 2, Q = high nibble of byte 2
    raw = np.array([0x7A, 0x3F, 0x81], dtype=np.uint8)
    xr, xi = dc.decode(raw, cases.packed_layout(4, complex=True, stride=3, lane=1))
    assert xr.tolist() == [7.0, 1.0] and xi.tolist() == [-1.0, -8.0]
    xr, xi = dc.decode(raw, cases.packed_layout(4, complex=True, stride=3, lane=1, swap_iq=True))
    assert xr.tolist() == [-1.0, -8.0] and xi.tolist() == [7.0, 1.0]
    with pytest.raises(ValueError):
        dc.decode(raw[:2], cases.packed_layout(4, complex=True, stride=3, lane=1))     # 16 bits: one frame and a nibble


@pytest.mark.parametrize("field,dtype", [(dc.FIELD_INT8, np.int8), (dc.FIELD_INT16, np.int16), (dc.FIELD_FLOAT32, np.float32)])
def test_decode_of_unpacked_fields_equals_numpy_views(field, dtype):
    rng = np.random.default_rng(cases.SEED + 5)
    for stride in (1, 2, 3, 4):
        raw = (rng.uniform(-100.0, 100.0, 50 * stride).astype(dtype) if field == dc.FIELD_FLOAT32 else rng.integers(-120, 121, 50 * stride).astype(dtype))
        for lane in range(stride):
            xr, xi = dc.decode(raw, dc.InputLayout(field, 0, stride, lane))
            assert np.array_equal(xr, raw[lane::stride].astype(np.float64)) and not xi.any() and xr.dtype == np.float64
            xr2, _ = dc.decode(raw.view(np.uint8), dc.InputLayout(field, 0, stride, lane))      # (bytes or the field's type: the same)
            assert np.array_equal(xr, xr2)
            if lane + 2 <= stride:
                xr, xi = dc.decode(raw, dc.InputLayout(field, 0, stride, lane, True))
                assert np.array_equal(xr, raw[lane::stride].astype(np.float64)) and np.array_equal(xi, raw[lane + 1::stride].astype(np.float64))
                sr, si = dc.decode(raw, dc.InputLayout(field, 0, stride, lane, True, True))
                assert np.array_equal(sr, xi) and np.array_equal(si, xr)


# ---------------------------------------------------------------------------------------------- 2. the layout's checks
def test_layout_limits_and_bytes_for():
    L = dc.InputLayout
    for bad in (lambda: L(4), lambda: L(-1), lambda: L(dc.FIELD_PACKED), lambda: L(dc.FIELD_PACKED, 3), lambda: L(dc.FIELD_PACKED, 8),
                lambda: L(dc.FIELD_INT8, 1), lambda: L(dc.FIELD_FLOAT32, 4), lambda: L(dc.FIELD_INT8, 0, 0), lambda: L(dc.FIELD_INT8, 0, 65),
                lambda: L(dc.FIELD_INT8, 0, 1, -1), lambda: L(dc.FIELD_INT8, 0, 1, 1), lambda: L(dc.FIELD_INT8, 0, 2, 1, True),
                lambda: L(dc.FIELD_INT8, 0, 1, 0, True), lambda: L(dc.FIELD_INT8, 0, 2, 0, False, True),
                lambda: L(dc.FIELD_INT16, 0, 2, 0, True, False, True), lambda: L(dc.FIELD_PACKED, 2, 1, 0, False, False, False, (1, 2, 3)),
                lambda: L(dc.FIELD_PACKED, 1, 1, 0, False, False, False, (1, 300)), lambda: L(dc.FIELD_INT8, 0, 1, 0, False, False, False, (1, -1))):
        with pytest.raises(ValueError):
            bad()
    assert L(dc.FIELD_INT8).stride == 1 and L(dc.FIELD_INT16, complex=True).stride == 2
    assert L(dc.FIELD_PACKED, 4, 64, 62, True, True, True).flags == 7 and L(dc.FIELD_FLOAT32, 0, 64, 63).flags == 0
    assert L(dc.FIELD_PACKED, 2).levels.tolist() == list(pk.DEFAULT_LEVELS[2])
    assert [L(dc.FIELD_INT8).dtype, L(dc.FIELD_INT16).dtype, L(dc.FIELD_FLOAT32).dtype, L(dc.FIELD_PACKED, 1).dtype] == [np.int8, np.int16, np.float32, np.uint8]
    # bytes: n_in * stride * bytes per field; packed n_in * stride * bits / 8, which must be whole
    assert L(dc.FIELD_INT8, 0, 3).bytes_for(10) == 30 and L(dc.FIELD_INT16, 0, 4, 2, True).bytes_for(10) == 80
    assert L(dc.FIELD_FLOAT32, 0, 2, 0, True).bytes_for(7) == 56 and L(dc.FIELD_FLOAT32).bytes_for(0) == 0
    one3 = cases.packed_layout(1, stride=3, lane=1)
    assert one3.bytes_for(8) == 3 and one3.bytes_for(16) == 6 and one3.frame_group == 8
    assert cases.packed_layout(2).bytes_for(4) == 1 and cases.packed_layout(2).frame_group == 4
    assert cases.packed_layout(2, stride=4).bytes_for(5) == 5 and cases.packed_layout(2, stride=4).frame_group == 1
    assert cases.packed_layout(4, complex=True, stride=3, lane=1).bytes_for(2) == 3 and cases.packed_layout(4, complex=True).frame_group == 1
    for lay, n in ((one3, 7), (one3, 1), (cases.packed_layout(2), 3), (cases.packed_layout(4, complex=True, stride=3), 1), (one3, -8), (L(dc.FIELD_INT8), -1)):
        with pytest.raises(ValueError):
            lay.bytes_for(n)
    assert one3.frames_in(3) == 8 and L(dc.FIELD_INT16, 0, 4, 2, True).frames_in(80) == 10
    with pytest.raises(ValueError):
        one3.frames_in(2)
    with pytest.raises(ValueError):
        L(dc.FIELD_INT16, 0, 4).frames_in(6)
    # what a push takes
    assert one3.input_array(np.zeros(3, dtype=np.uint8)).size == 3
    for bad in (np.zeros(3, dtype=np.int8), np.zeros(2, dtype=np.uint8), np.zeros((3, 1), dtype=np.uint8), np.zeros(6, dtype=np.uint8)[::2], [0, 0, 0]):
        with pytest.raises(ValueError):
            one3.input_array(bad)
    # a configuration with a layout does not consult in_fmt; without one nothing has changed
    assert dc.DownConverterConfig(99, layout=one3).layout is one3
    with pytest.raises(ValueError):
        dc.DownConverterConfig(99)
    with pytest.raises(ValueError):
        dc.DownConverterConfig(0, layout="packed")
    assert dc.DownConverterConfig(dc.IN_R8).layout is None


# ---------------------------------------------------------------------------------------------- 3. the statement
LAYOUTS = [cases.packed_layout(1), cases.packed_layout(2, msb_first=True, levels=cases.ODD_TABLE), cases.packed_layout(4, complex=True),
           cases.packed_layout(1, stride=3, lane=1), cases.packed_layout(4, complex=True, stride=3, lane=1),
           dc.InputLayout(dc.FIELD_INT16, 0, 4, 2, True, True), dc.InputLayout(dc.FIELD_FLOAT32, 0, 2, 0, True), dc.InputLayout(dc.FIELD_FLOAT32),
           dc.InputLayout(dc.FIELD_INT8), dc.InputLayout(dc.FIELD_INT16), dc.InputLayout(dc.FIELD_INT8, complex=True), dc.InputLayout(dc.FIELD_INT16, complex=True)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=repr)
@pytest.mark.parametrize("shape", [(33, 2), (3, 2, 7)], ids=cases.shape_id)
def test_statement_with_a_layout_equals_the_old_format_on_the_decoded_integers(layout, shape):
    n = 4000
    raw = cases.stream(layout, n)
    old_fmt = cases.old_format(layout)
    plain = cases.decoded(raw, layout)
    fcw, gain = cases.FCWS["odd"], dcases.GOLD
    new_cfg, old_cfg = cases.config(shape, fcw, gain, layout=layout), cases.config(shape, fcw, gain, old_fmt)
    whole = dc.statement(old_cfg, [plain])
    assert whole.size == cases.out_total(shape, n)
    assert dc.statement(new_cfg, [raw]).tobytes() == whole.tobytes()
    # ... however the bytes are cut (whole bytes each), pushes shorter than the history included; out_count agrees before each
    lengths = cases.rounded_lengths(cases.phase_taps(shape), layout.frame_group)
    st, parts = dc.Statement(new_cfg), []
    for piece in cases.cut_bytes(raw, layout, lengths):
        want = st.out_count(layout.frames_in(piece.nbytes))
        parts.append(st.push(piece))
        assert parts[-1].size == want
    assert np.concatenate(parts).tobytes() == whole.tobytes() and st.n_seen == n
    # the four plain layouts ARE the four old formats: the same array goes into both
    if layout.stride == (2 if layout.complex else 1) and layout.field in (dc.FIELD_INT8, dc.FIELD_INT16):
        assert plain.dtype == raw.dtype and np.array_equal(plain, raw)


def test_statement_keeps_a_nan_inside_its_windows():
    shape, n, at = (33, 2), 2000, 1001
    lay = dc.InputLayout(dc.FIELD_FLOAT32)
    raw = cases.fractional(False, n).copy()
    raw[at] = 0.0
    cfg = cases.config(shape, cases.FCWS["odd"], 1000.0, layout=lay)
    clean = dc.statement(cfg, [raw])
    raw[at] = np.nan
    with np.errstate(invalid="ignore"):
        dirty = dc.statement(cfg, [raw])
    m = np.arange(clean.size)
    inside = (m * 2 >= at) & (m * 2 - 32 <= at)                           # output m reads inputs 2 m - 32 .. 2 m
    assert np.all(np.isnan(dirty.real[inside])) and inside.sum() == 16
    assert np.array_equal(dirty[~inside].view(np.uint64), clean[~inside].view(np.uint64))


# ---------------------------------------------------------------------------------------------- 4. RFSignal
def _packed_file(tmp_path, ms=3):
    packed, few = cases.packed_real_recording(ms)
    path = tmp_path / "real_if_2bit.bin"
    packed.tofile(path)
    return path, packed, few


def test_rfsignal_layout_keys(tmp_path):
    path, packed, few = _packed_file(tmp_path)
    sig = RFSignal(cases.packed_real_conf(path))
    lay, fe = sig.layout, sig.frontEnd
    assert lay == cases.packed_layout(2) and fe.config.layout is lay and sig.packing is None and sig.fileDataType == np.uint8
    assert not sig.isComplex and fe.outputBits == 8 and fe.config.gain == 16.0 and fe.config.n_taps == 33 and fe.config.fcw == 1 << 62
    assert (sig.samplingFrequency, sig.samplesPerMs, sig.interFrequency, sig.inputSamplesPerMs) == (4.092e6, 4092, 0.0, 8184)
    # frames are counted, whole-byte views handed out
    assert sig.totalSamples == few.size == 3 * 8184
    ms = sig.getMilliseconds(1)
    assert ms.dtype == np.uint8 and ms.size == 2046 and np.array_equal(ms, packed[:2046]) and np.shares_memory(ms, sig._recording()) and sig.position == 8184
    assert np.array_equal(sig.samples(100, 40), packed[25:35])
    with pytest.raises(ValueError, match="whole bytes"):
        sig.samples(101, 40)
    with pytest.raises(ValueError, match="whole bytes"):
        sig.samples(100, 41)
    assert np.array_equal(sig.getMilliseconds(1, raw=False), few[8184:2 * 8184].astype(np.float64) + 0j)
    assert np.array_equal(sig.readFileBySamples(37, skip=1001), few[1001:1038].astype(np.float64) + 0j)      # raw=False: from any frame
    assert np.array_equal(sig.readFile(timeLength=1, raw=True), packed[:2046])
    assert np.array_equal(sig.readFileBySamples(50, skip=3 * 8184 - 20), few[-20:].astype(np.float64) + 0j)  # a short read at the end
    # levels and bit order as for packed recordings; a resampler
    odd = RFSignal(cases.packed_real_conf(path, sample_levels="-7,2,5,-128", bit_order="msb", output_bits=16))
    assert odd.layout == cases.packed_layout(2, msb_first=True, levels=cases.ODD_TABLE) and odd.frontEnd.outputBits == 16
    max2769 = RFSignal(dict(filepath="x", sampling_frequency=16.368e6, is_complex="", intermediate_frequency=4.092e6, data_size=2,
                            sample_format="packed", decimation=341, interpolation=250))
    assert max2769.samplingFrequency == 12e6 and max2769.layout == cases.packed_layout(2) and max2769.frontEnd.interpolation == 250
    one = RFSignal(dict(filepath="x", sampling_frequency=16.368e6, is_complex="", intermediate_frequency=4.092e6, data_size=1,
                        sample_format="packed", decimation=4, frame_fields=3, frame_lane=1))
    assert one.layout == cases.packed_layout(1, stride=3, lane=1)
    # float32 and interleaved integer files
    flt = RFSignal(dict(filepath="x", sampling_frequency=25e6, is_complex="true", intermediate_frequency=0.0, data_size=32, sample_format="float",
                        decimation=1, filter_taps=1, output_gain=1000.0))
    assert flt.layout == dc.InputLayout(dc.FIELD_FLOAT32, complex=True) and flt.fileDataType == np.float32 and flt.frontEnd.outputBits == 16
    two = RFSignal(dict(filepath="x", sampling_frequency=8.184e6, is_complex="true", intermediate_frequency=0.0, data_size=16, sample_format="int",
                        decimation=2, frame_fields=4, frame_lane=2, swap_iq=1))
    assert two.layout == dc.InputLayout(dc.FIELD_INT16, 0, 4, 2, True, True) and two.frontEnd.outputBits == 16
    # an int16 file of two complex streams: frames, views and complex samples
    rng = np.random.default_rng(cases.SEED + 8)
    both = rng.integers(-3000, 3001, 4 * 2 * 8184).astype(np.int16)
    both.tofile(tmp_path / "two.bin")
    two = RFSignal(dict(filepath=str(tmp_path / "two.bin"), sampling_frequency=8.184e6, is_complex="true", intermediate_frequency=0.0, data_size=16,
                        sample_format="int", decimation=2, frame_fields=4, frame_lane=2, swap_iq=1))
    assert two.totalSamples == 2 * 8184
    ms = two.getMilliseconds(1)
    assert ms.dtype == np.int16 and np.array_equal(ms, both[:4 * 8184])
    assert np.array_equal(two.getMilliseconds(1, raw=False), both[4 * 8184 + 3::4].astype(np.float64) + 1j * both[4 * 8184 + 2::4].astype(np.float64))


def test_rfsignal_layout_refusals():
    conf = cases.packed_real_conf("x")
    for bad in (dict(sample_format="nibbles"), dict(data_size=8), dict(data_size=32), dict(sample_format="float", data_size=16),
                dict(sample_format="float", data_size=2), dict(sample_format="int", data_size=2), dict(sample_format="int", data_size=32),
                dict(frame_fields=0), dict(frame_fields=65), dict(frame_lane=1), dict(frame_lane=-1), dict(swap_iq=1),             # (real: no swap)
                dict(swap_iq=2, is_complex="true"), dict(frame_fields=1, is_complex="true"), dict(bit_order="middle"), dict(sample_levels="1,2,3"),
                dict(data_size=1, frame_fields=3, sampling_frequency=8.185e6, decimation=1),           # 8185 * 3 bits: no whole bytes
                dict(output_bits=32)):
        with pytest.raises(ValueError):
            RFSignal(dict(conf, **bad))
    # bit_order and msb only mean something for packed fields
    with pytest.raises(ValueError):
        RFSignal(dict(conf, sample_format="weird", data_size=64))
    # the frame keys need sample_format beside them; every new key needs a front end
    plain = dcases.real_signal_conf("x")
    for key, value in (("frame_fields", 2), ("frame_lane", 0), ("swap_iq", 0)):
        with pytest.raises(ValueError, match="sample_format"):
            RFSignal(dict(plain, **{key: value}))
    ordinary = dict(filepath="x", sampling_frequency=8.184e6, is_complex="true", intermediate_frequency=0.0, data_size=8)
    for key, value in (("sample_format", "int"), ("frame_fields", 2), ("frame_lane", 0), ("swap_iq", 0)):
        with pytest.raises(ValueError, match="needs a front end"):
            RFSignal(dict(ordinary, **{key: value}))
    with pytest.raises(ValueError, match="needs a front end"):
        RFSignal(dict(ordinary, data_size=2, sample_format="packed"))


def test_configurations_without_sample_format_are_what_they_were():
    real = dcases.real_signal_conf("x")
    sig = RFSignal(real)
    assert sig.layout is None and sig.frontEnd.config.layout is None and sig.frontEnd.config.in_fmt == dc.IN_R8 and sig.fileDataType == np.int8
    wide = RFSignal(dict(filepath="x", sampling_frequency=50e6, is_complex="true", intermediate_frequency=1e6, data_size=16, decimation=5))
    assert wide.layout is None and wide.frontEnd.config.in_fmt == dc.IN_CI16 and wide.frontEnd.config.layout is None and wide.frontEnd.outputBits == 16
    packed = RFSignal(dict(filepath="x", sampling_frequency=4e6, is_complex="true", intermediate_frequency=0.0, data_size=2))
    assert packed.layout is None and packed.frontEnd is None and packed.packing == pk.Packing(2)
    with pytest.raises(ValueError, match="packed recordings cannot be down-converted: `decimation` needs data_size 8 or 16"):
        RFSignal(dict(real, data_size=2))
    with pytest.raises(ValueError, match="packed recordings cannot be down-converted"):
        RFSignal(dict(real, data_size=4, is_complex="true"))
    with pytest.raises(ValueError, match="real-valued recordings are not supported"):
        RFSignal({k: v for k, v in real.items() if k != "decimation"})
    with pytest.raises(ValueError, match="real-valued recordings are not supported"):
        RFSignal(dict(filepath="x", sampling_frequency=4e6, is_complex="", intermediate_frequency=0.0, data_size=2))
    for bits in (3, 12, 32, 64):
        with pytest.raises(ValueError, match=f"Data type of {bits} bit"):
            RFSignal(dict(real, data_size=bits))


# ---------------------------------------------------------------------------------------------- 5. the manager
def test_manager_over_a_packed_real_recording_equals_the_converted_recording(tmp_path):
    """The 2-bit real recording through the converter (statement-backed engine) against the statement's ci8 output fed as an
    ordinary complex int8 recording: the packets are equal, and the manager hands the converter the file's packed bytes."""
    ms = 30
    sig, conv_sig, converted = cases.write_packed_and_converted(tmp_path, ms)
    assert converted.size == 2 * ms * 4092 and int(np.max(np.abs(converted))) < 127
    cfg = packed_cases.kaplan_config()
    eng = ConvertingOracleEngine()
    got, mgr = packed_cases.receive(sig, eng, prns=[dcases.SATELLITE["prn"]], cfg=cfg, ms=ms, mode="ticks")
    want, want_mgr = packed_cases.receive(conv_sig, ConvertingOracleEngine(), prns=[dcases.SATELLITE["prn"]], cfg=cfg, ms=ms, mode="ticks")
    assert mgr.sharedBuffer.fmt == 0 and mgr.sharedBuffer.maxSize == 100 * 4092
    assert len(got) == len(want) == ms
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, k
    assert packed_cases.count(got, ChannelMessage.ACQUISITION_UPDATE) == 1 and packed_cases.count(got) > 15
    assert eng.ddc_calls == dict(create=1, push=0, queue=ms, destroy=0)
    # what the manager accepts: the layout's arrays, whole frames
    data, n_in = mgr._raw_input(sig.samples(0, 8184))
    assert data.dtype == np.uint8 and data.size == 2046 and n_in == 8184
    with pytest.raises(ValueError):
        mgr._raw_input(np.zeros(2046, dtype=np.int8))
    with pytest.raises(ValueError, match="multiple from the max buffer size"):
        mgr.addNewRFData(np.zeros(2045, dtype=np.uint8))                                  # 8180 frames: whole bytes, no millisecond
    mgr.close()
    want_mgr.close()


# ---------------------------------------------------------------------------------------------- 6. the C struct and the byte count
def test_ddc_layout_struct_agrees_with_the_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sydr_amd.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n",'
                   "sizeof(sdr_ddc_layout),offsetof(sdr_ddc_layout,field),offsetof(sdr_ddc_layout,bits),offsetof(sdr_ddc_layout,stride),"
                   "offsetof(sdr_ddc_layout,lane),offsetof(sdr_ddc_layout,flags),offsetof(sdr_ddc_layout,reserved),offsetof(sdr_ddc_layout,levels),"
                   "SDR_DDC_FIELD_INT8,SDR_DDC_FIELD_INT16,SDR_DDC_FIELD_FLOAT32,SDR_DDC_FIELD_PACKED,SDR_DDC_LAYOUT_COMPLEX,SDR_DDC_LAYOUT_SWAP_IQ,"
                   "SDR_DDC_LAYOUT_MSB_FIRST);return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    # the header's declarations are exactly these prototypes (a mismatch is an error), and the bindings say the same
    proto = tmp_path / "proto.c"
    proto.write_text('#include "sydr_amd.h"\n'
                     "int (*const create)(sdr_engine*, const sdr_ddc_cfg*, int, const sdr_ddc_layout*, sdr_ddc**) = sdr_ddc_create_layout;\n"
                     "int64_t (*const bytes)(const sdr_ddc_layout*, int64_t) = sdr_ddc_layout_bytes;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(REPO, "include"), "-c", str(proto),
                           "-o", str(tmp_path / "proto.o")])
    lib = _lib.load()
    assert lib.sdr_ddc_create_layout.restype is C.c_int and lib.sdr_ddc_layout_bytes.restype is C.c_int64
    assert list(lib.sdr_ddc_create_layout.argtypes) == [C.c_void_p, C.POINTER(_lib.DdcCfg), C.c_int, C.POINTER(_lib.DdcLayout), C.POINTER(C.c_void_p)]
    assert list(lib.sdr_ddc_layout_bytes.argtypes) == [C.POINTER(_lib.DdcLayout), C.c_int64]
    assert lib.sdr_ddc_create_layout(None, None, 1, None, None) != 0                      # (host checks come before any device call)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = _lib.DdcLayout
    assert got[:8] == [C.sizeof(D), D.field.offset, D.bits.offset, D.stride.offset, D.lane.offset, D.flags.offset, D.reserved.offset, D.levels.offset]
    assert got[:8] == [40, 0, 4, 8, 12, 16, 20, 24]
    assert got[8:] == [dc.FIELD_INT8, dc.FIELD_INT16, dc.FIELD_FLOAT32, dc.FIELD_PACKED, dc.LAYOUT_COMPLEX, dc.LAYOUT_SWAP_IQ, dc.LAYOUT_MSB_FIRST]
    assert got[8:] == [_lib.DDC_FIELD_INT8, _lib.DDC_FIELD_INT16, _lib.DDC_FIELD_FLOAT32, _lib.DDC_FIELD_PACKED, _lib.DDC_LAYOUT_COMPLEX,
                       _lib.DDC_LAYOUT_SWAP_IQ, _lib.DDC_LAYOUT_MSB_FIRST]
    assert got[8:] == [0, 1, 2, 3, 1, 2, 4]
    # the two functions are the only new dynamic symbols, and the ABI's number has not moved
    names = _lib.exported_symbols()
    assert {n for n in names if "layout" in n} == {"sdr_ddc_create_layout", "sdr_ddc_layout_bytes"}
    assert _lib.load().sdr_abi_version() == 5


def test_sdr_ddc_layout_bytes_through_ctypes():
    lib = _lib.load()

    def count(layout, n_in):
        return lib.sdr_ddc_layout_bytes(C.byref(layout_struct(layout)), n_in)

    for layout in LAYOUTS:
        for n_in in (0, 1, 2, 3, 4, 7, 8, 16, 24, 1000, 20000, 1 << 40):
            try:
                want = layout.bytes_for(n_in)
            except ValueError:
                want = INVALID
            assert count(layout, n_in) == want, (layout, n_in)
        assert count(layout, -1) == INVALID
    assert lib.sdr_ddc_layout_bytes(None, 8) == INVALID

    def raw(field=0, bits=0, stride=1, lane=0, flags=0, reserved=0):
        return lib.sdr_ddc_layout_bytes(C.byref(_lib.DdcLayout(field, bits, stride, lane, flags, reserved)), 8)

    assert raw() == 8 and raw(1, 0, 2, 0, 1) == 32 and raw(3, 4, 64, 62, 7) == 256 and raw(2, 0, 64, 63) == 2048
    for kw in (dict(field=4), dict(field=-1), dict(field=3), dict(field=3, bits=3), dict(field=3, bits=8), dict(bits=1), dict(field=2, bits=4),
               dict(stride=0), dict(stride=65), dict(lane=-1), dict(lane=1), dict(stride=2, lane=1, flags=1), dict(flags=1), dict(stride=2, flags=2),
               dict(stride=2, flags=4), dict(field=1, stride=2, flags=5), dict(stride=2, flags=8), dict(stride=2, flags=-1), dict(reserved=1)):
        assert raw(**kw) == INVALID, kw


# ---------------------------------------------------------------------------------------------- 7. the field arithmetic
@host_check.requires_hipcc
def test_field_arithmetic_on_the_host():
    """sydr_amd/csrc/ddc_layout.h, the decode the converter's kernels and its host side share, compiled for the host alone and
    checked exhaustively over bits, both bit orders, stride <= 9, every lane, real and complex, swap, j < 64 against a
    bit-by-bit reading (tests/csrc/ddc_layout_check.hip)."""
    exe = host_check.build("ddc_layout_check")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    assert int(out.stdout.split()[1]) > 50000
