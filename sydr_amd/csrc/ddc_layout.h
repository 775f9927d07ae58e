// Field arithmetic of an input layout (sdr_ddc_layout, include/sydr_amd.h): how a recording's bytes hold the converter's inputs.
// Shared by the host that checks a layout and counts a push's bytes, the kernels of ddc.hip / resample.hip that decode their
// inputs where they load them, and the host check tests/csrc/ddc_layout_check.hip.
//
// A recording is a sequence of FIELDS f = 0, 1, ..., one component each: int8, int16, float32, or a packed code of `bits` bits
// (1, 2 or 4).  With F = 8 / bits, packed field f lies in byte f div F at position p = f mod F: its code is the `bits` bits from
// bit bits * p up (least significant field first) or from bit bits * (F - 1 - p) up (MSB_FIRST); the component is levels[code].
// A FRAME is `stride` consecutive fields; input j of the stream is frame j: real x_j = field(j * stride + lane); complex
// a = field(j * stride + lane), b = the next field, x_j = a + ib, or b + ia with SWAP_IQ.  Every component widens to fp64 exactly.
// The HISTORY of such a converter holds the last Tp - 1 inputs decoded: this stream's components alone, after the swap, as int8
// (INT8 and PACKED), int16 or float32, one (real) or two (complex) per input -- itself a layout, ddc_layout_history.
#pragma once

#include <cstdint>
#include <cstring>

#include "ddc_tiles.h"

namespace sdr {

constexpr int kDdcFieldInt8 = 0, kDdcFieldInt16 = 1, kDdcFieldFloat32 = 2, kDdcFieldPacked = 3;     // sdr_ddc_field
constexpr int kDdcLayoutComplex = 1, kDdcLayoutSwapIq = 2, kDdcLayoutMsbFirst = 4;                // SDR_DDC_LAYOUT_*
constexpr int kDdcMaxStride = 64;
constexpr int64_t kDdcLayoutMaxFrames = (int64_t)1 << 48;     // of one push: its bytes and fields stay far inside 64 bits

// A layout as the kernels take it, by value: the 16 level bytes as two words, level c the byte c % 8 of lv[c / 8].
struct DdcLayout {
    int kind, bits, stride, lane, flags;
    uint64_t lv[2];
};

SDR_DDC_HD inline bool ddc_layout_valid(int kind, int bits, int stride, int lane, int flags, int reserved) {
    if (kind < kDdcFieldInt8 || kind > kDdcFieldPacked) return false;
    if (kind == kDdcFieldPacked ? !(bits == 1 || bits == 2 || bits == 4) : bits != 0) return false;
    if (flags & ~(kDdcLayoutComplex | kDdcLayoutSwapIq | kDdcLayoutMsbFirst) || reserved) return false;
    if ((flags & kDdcLayoutSwapIq) && !(flags & kDdcLayoutComplex)) return false;
    if ((flags & kDdcLayoutMsbFirst) && kind != kDdcFieldPacked) return false;
    if (stride < 1 || stride > kDdcMaxStride || lane < 0) return false;
    return lane + ((flags & kDdcLayoutComplex) ? 2 : 1) <= stride;
}

inline DdcLayout ddc_layout_make(int kind, int bits, int stride, int lane, int flags, const int8_t* levels) {
    DdcLayout l;
    l.kind = kind, l.bits = bits, l.stride = stride, l.lane = lane, l.flags = flags;
    uint8_t table[16] = {0};
    if (kind == kDdcFieldPacked) memcpy(table, levels, (size_t)1 << bits);      // (the first 1 << bits are read)
    memcpy(l.lv, table, 16);
    return l;
}

// Bytes of an unpacked field; 0 for a packed one.
SDR_DDC_HD inline int ddc_field_bytes(int kind) { return kind == kDdcFieldInt8 ? 1 : kind == kDdcFieldInt16 ? 2 : kind == kDdcFieldFloat32 ? 4 : 0; }

// Bytes a push of n_in frames reads, or -1: a packed push that is not whole bytes (n_in >= 0, a valid layout).
SDR_DDC_HD inline int64_t ddc_layout_push_bytes(const DdcLayout& l, int64_t n_in) {
    const int64_t fields = n_in * l.stride;
    if (l.kind != kDdcFieldPacked) return fields * ddc_field_bytes(l.kind);
    const int64_t bits = fields * l.bits;
    return bits % 8 ? -1 : bits / 8;
}

// The first field of frame j's input (the second, of a complex layout, follows it).
SDR_DDC_HD inline int64_t ddc_frame_field(const DdcLayout& l, int64_t j) { return j * l.stride + l.lane; }

// Packed field f: its byte, and the bit its code begins at.
SDR_DDC_HD inline int ddc_fields_log2(int bits) { return bits == 1 ? 3 : bits == 2 ? 2 : 1; }     // log2(8 / bits)
SDR_DDC_HD inline int64_t ddc_field_byte(int64_t f, int bits) { return f >> ddc_fields_log2(bits); }
SDR_DDC_HD inline int ddc_field_shift(int64_t f, int bits, bool msb_first) {
    const int F = 8 / bits, p = (int)(f & (F - 1));
    return bits * (msb_first ? F - 1 - p : p);
}
SDR_DDC_HD inline int ddc_level(const DdcLayout& l, int code) { return (int)(int8_t)(l.lv[code >> 3] >> (8 * (code & 7))); }

// Field f of the bytes at `p`, widened.  (An int16 or float32 field is read as itself: a pair at an odd field index is two loads.)
SDR_DDC_HD inline double ddc_field(const void* __restrict__ p, int64_t f, const DdcLayout& l) {
    switch (l.kind) {
        case kDdcFieldInt8: return (double)((const int8_t*)p)[f];
        case kDdcFieldInt16: return (double)((const int16_t*)p)[f];
        case kDdcFieldFloat32: return (double)((const float*)p)[f];
        default: {
            const unsigned byte = ((const uint8_t*)p)[ddc_field_byte(f, l.bits)];
            const int code = (int)(byte >> ddc_field_shift(f, l.bits, (l.flags & kDdcLayoutMsbFirst) != 0)) & ((1 << l.bits) - 1);
            return (double)ddc_level(l, code);
        }
    }
}

// Input j (frame j of the bytes at `p`) as x = re + i im.
SDR_DDC_HD inline void ddc_layout_load(const void* __restrict__ p, int64_t j, const DdcLayout& l, double* re, double* im) {
    const int64_t f = ddc_frame_field(l, j);
    const double a = ddc_field(p, f, l);
    if (!(l.flags & kDdcLayoutComplex)) {
        *re = a, *im = 0.0;
        return;
    }
    const double b = ddc_field(p, f + 1, l);
    const bool swap = (l.flags & kDdcLayoutSwapIq) != 0;
    *re = swap ? b : a, *im = swap ? a : b;
}

// The layout of the history: the decoded components of this stream alone.
SDR_DDC_HD inline DdcLayout ddc_layout_history(const DdcLayout& l) {
    DdcLayout h;
    h.kind = l.kind == kDdcFieldPacked ? kDdcFieldInt8 : l.kind, h.bits = 0, h.lane = 0;
    h.flags = l.flags & kDdcLayoutComplex, h.stride = h.flags ? 2 : 1;
    h.lv[0] = h.lv[1] = 0;
    return h;
}

// Bytes one input takes in the history.
SDR_DDC_HD inline int ddc_layout_history_unit(const DdcLayout& l) {
    const DdcLayout h = ddc_layout_history(l);
    return h.stride * ddc_field_bytes(h.kind);
}

// Input x = re + i im (components this layout's kind holds exactly) into element i of the history at `p`.
SDR_DDC_HD inline void ddc_layout_history_store(void* p, int i, const DdcLayout& hist, double re, double im) {
    const int n = hist.stride;
    for (int c = 0; c < n; ++c) {
        const double v = c ? im : re;
        const int at = i * n + c;
        if (hist.kind == kDdcFieldInt8) ((int8_t*)p)[at] = (int8_t)v;
        else if (hist.kind == kDdcFieldInt16) ((int16_t*)p)[at] = (int16_t)v;
        else ((float*)p)[at] = (float)v;
    }
}

}  // namespace sdr
