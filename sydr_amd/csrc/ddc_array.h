// An ARRAY of a converter (sdr_ddc_array, include/sydr_amd.h): K antenna elements of a multi-element recording combined into the
// one stream the converter mixes, filters and decimates.  Shared by the host that checks an array, the kernels of ddc.hip /
// resample.hip that combine their inputs where they load them, the covariance pass of ddc_array.hip and the host check
// tests/csrc/ddc_array_check.hip.  The NumPy form is sydr_amd/signal/array.py.
//
// An array is a layout (ddc_layout.h) plus K elements, K in 2..8, element a at lane lanes[a] of the frame: distinct lanes, each
// with lanes[a] + (COMPLEX ? 2 : 1) <= stride, in any order; the layout's own lane is not read.  Element a of frame j is decoded
// exactly as the layout decodes a stream at that lane: s_a = sr_a + i si_a (si = 0 of a real layout, SWAP_IQ honoured).  With
// weights w_a = wr_a + i wi_a the converter's input j is x_j = sum_a conj(w_a) s_a, in fp64, in this order and no other -- every
// product rounded, every sum rounded, nothing contracted:
//     re = 0; im = 0
//     for a = 0 .. K-1:   re = re + wr_a sr_a;  re = re + wi_a si_a;  im = im + wr_a si_a;  im = im - wi_a sr_a
// The HISTORY of such a converter holds the last Tp - 1 COMBINED inputs, cf64 (re, im), 16 bytes each: a weight change never
// reaches an input that has been combined.
// A packed frame whose bits lie within 8 consecutive bytes (a K-element complex 2-bit frame is 4 K bits) is loaded once per input
// into a 64-bit window, the elements' codes shifted out of it; wider frames are read field by field.
#pragma once

#include <cmath>

#include "ddc_layout.h"

namespace sdr {

constexpr int kDdcArrayMin = 2, kDdcArrayMax = 8;
constexpr int kDdcArrayMeasure = 1;                     // SDR_DDC_ARRAY_MEASURE
constexpr int kDdcArrayHistoryUnit = 16;                // bytes of a combined input in the history

// An array as the kernels take it, by value: lanes and weights are kernel arguments, read by wave-uniform (scalar) loads.
struct DdcArray {
    int K, flags;
    int lanes[kDdcArrayMax];
    double w[kDdcArrayMax][2];
};

// `lay` a valid layout (its lane aside: ddc_layout_valid with lane 0).
SDR_DDC_HD inline bool ddc_array_lanes_valid(const DdcLayout& lay, int K, int flags, const int* lanes) {
    if (K < kDdcArrayMin || K > kDdcArrayMax || (flags & ~kDdcArrayMeasure)) return false;
    const int width = (lay.flags & kDdcLayoutComplex) ? 2 : 1;
    for (int a = 0; a < K; ++a) {
        if (lanes[a] < 0 || lanes[a] + width > lay.stride) return false;
        for (int b = 0; b < a; ++b)
            if (lanes[b] == lanes[a]) return false;
    }
    return true;
}

inline bool ddc_array_weights_valid(int K, const double* w /*[K][2]*/) {
    for (int a = 0; a < 2 * K; ++a)
        if (!std::isfinite(w[a])) return false;
    return true;
}

// The bytes of frame j that hold packed fields, once: bits [0, 64) of `bits` are the bytes from `byte0` up, least significant
// first, as many as the frame touches; `whole` is false (and nothing loaded) when the layout is not packed or the frame touches
// more than 8 bytes.
struct DdcFrame {
    uint64_t bits;
    int64_t byte0;
    bool whole;
};

SDR_DDC_HD inline DdcFrame ddc_array_frame(const void* __restrict__ p, int64_t j, const DdcLayout& l) {
    DdcFrame fr;
    fr.bits = 0, fr.byte0 = 0, fr.whole = false;
    if (l.kind != kDdcFieldPacked) return fr;
    const int frame_bits = l.stride * l.bits;
    const int64_t bit0 = j * frame_bits;
    fr.byte0 = bit0 >> 3;
    const int touched = (int)(((bit0 + frame_bits + 7) >> 3) - fr.byte0);      // bytes the frame's bits lie in, all inside the push
    if (touched > 8) return fr;
    const uint8_t* b = (const uint8_t*)p + fr.byte0;
    for (int k = 0; k < touched; ++k) fr.bits |= (uint64_t)b[k] << (8 * k);
    fr.whole = true;
    return fr;
}

// levels[code] by a select between the table's two words (ddc_level's value without its run-time index into the layout).
SDR_DDC_HD inline int ddc_array_level(const DdcLayout& l, int code) {
    const uint64_t word = (code & 8) ? l.lv[1] : l.lv[0];
    return (int)(int8_t)(word >> (8 * (code & 7)));
}

// Field f of frame j as an integer (INT8, INT16, PACKED) ...
SDR_DDC_HD inline int ddc_array_field_int(const void* __restrict__ p, int64_t f, const DdcLayout& l, const DdcFrame& fr) {
    if (l.kind == kDdcFieldInt8) return (int)((const int8_t*)p)[f];
    if (l.kind == kDdcFieldInt16) return (int)((const int16_t*)p)[f];
    const bool msb = (l.flags & kDdcLayoutMsbFirst) != 0;
    const int mask = (1 << l.bits) - 1;
    if (fr.whole) {
        const int at = 8 * (int)(ddc_field_byte(f, l.bits) - fr.byte0) + ddc_field_shift(f, l.bits, msb);
        return ddc_array_level(l, (int)(fr.bits >> at) & mask);
    }
    const unsigned byte = ((const uint8_t*)p)[ddc_field_byte(f, l.bits)];
    return ddc_array_level(l, (int)(byte >> ddc_field_shift(f, l.bits, msb)) & mask);
}
// ... and widened, of any kind.
SDR_DDC_HD inline double ddc_array_field(const void* __restrict__ p, int64_t f, const DdcLayout& l, const DdcFrame& fr) {
    return l.kind == kDdcFieldFloat32 ? (double)((const float*)p)[f] : (double)ddc_array_field_int(p, f, l, fr);
}

// Element at `lane` of frame j (`fr` = ddc_array_frame of it) as s = re + i im: what ddc_layout_load gives the layout with that lane.
SDR_DDC_HD inline void ddc_array_element(const void* __restrict__ p, int64_t j, const DdcLayout& l, const DdcFrame& fr, int lane, double* re,
                                         double* im) {
    const int64_t f = j * l.stride + lane;
    const double a = ddc_array_field(p, f, l, fr);
    if (!(l.flags & kDdcLayoutComplex)) {
        *re = a, *im = 0.0;
        return;
    }
    const double b = ddc_array_field(p, f + 1, l, fr);
    const bool swap = (l.flags & kDdcLayoutSwapIq) != 0;
    *re = swap ? b : a, *im = swap ? a : b;
}
SDR_DDC_HD inline void ddc_array_element_int(const void* __restrict__ p, int64_t j, const DdcLayout& l, const DdcFrame& fr, int lane, int* re,
                                             int* im) {
    const int64_t f = j * l.stride + lane;
    const int a = ddc_array_field_int(p, f, l, fr);
    if (!(l.flags & kDdcLayoutComplex)) {
        *re = a, *im = 0;
        return;
    }
    const int b = ddc_array_field_int(p, f + 1, l, fr);
    const bool swap = (l.flags & kDdcLayoutSwapIq) != 0;
    *re = swap ? b : a, *im = swap ? a : b;
}

// One step of the combine: element a's four products into (re, im), in the statement's order.  Contraction is off for this
// function whatever the translation unit is compiled with: a fused multiply-add would round once where the statement rounds twice.
SDR_DDC_HD inline void ddc_array_accumulate(double wr, double wi, double sr, double si, double* re, double* im) {
#pragma clang fp contract(off)
    double r = *re, i = *im;
    const double p0 = wr * sr, p1 = wi * si, p2 = wr * si, p3 = wi * sr;
    r = r + p0;
    r = r + p1;
    i = i + p2;
    i = i - p3;
    *re = r, *im = i;
}

// Where a combine takes its weights from: the array's own, a kernel argument by value (the converter's own stream) ...
struct DdcArrayOwnWeights {
    const DdcArray& arr;
    SDR_DDC_HD double re(int a) const { return arr.w[a][0]; }
    SDR_DDC_HD double im(int a) const { return arr.w[a][1]; }
};
// ... or a row [kDdcArrayMax][2] of a table in device memory (an attached beam's: ddc_handle.h), read by wave-uniform loads.
struct DdcArrayTableWeights {
    const double* __restrict__ w;
    SDR_DDC_HD double re(int a) const { return w[2 * a]; }
    SDR_DDC_HD double im(int a) const { return w[2 * a + 1]; }
};

// Input j of the converter: x_j = sum_a conj(w_a) s_a over the frame's K elements, the weights from `w`.
template <class Weights>
SDR_DDC_HD inline void ddc_array_combine(const void* __restrict__ p, int64_t j, const DdcLayout& l, const DdcArray& arr, const Weights& w, double* re,
                                         double* im) {
    const DdcFrame fr = ddc_array_frame(p, j, l);
    double r = 0.0, i = 0.0;
    // (unrolled with constant element indices: on the device lanes and weights then stay kernel arguments in scalar registers;
    // a run-time index would copy the array to scratch memory)
#pragma unroll
    for (int a = 0; a < kDdcArrayMax; ++a) {
        if (a >= arr.K) break;
        double sr, si;
        ddc_array_element(p, j, l, fr, arr.lanes[a], &sr, &si);
        ddc_array_accumulate(w.re(a), w.im(a), sr, si, &r, &i);
    }
    *re = r, *im = i;
}
SDR_DDC_HD inline void ddc_array_load(const void* __restrict__ p, int64_t j, const DdcLayout& l, const DdcArray& arr, double* re, double* im) {
    ddc_array_combine(p, j, l, arr, DdcArrayOwnWeights{arr}, re, im);
}

// The history: combined inputs as (re, im) doubles.
SDR_DDC_HD inline void ddc_array_history_load(const void* __restrict__ p, int64_t i, double* re, double* im) {
    const double* h = (const double*)p + 2 * i;
    *re = h[0], *im = h[1];
}
SDR_DDC_HD inline void ddc_array_history_store(void* p, int i, double re, double im) {
    double* h = (double*)p + 2 * i;
    h[0] = re, h[1] = im;
}

// The covariance's 64 slots: entry (a, b) with a <= b has its real part at a * 8 + b and (a < b) its imaginary part at b * 8 + a
// -- the upper triangle of the Hermitian R, mirrored where it is read.
SDR_DDC_HD inline int ddc_array_cov_re(int a, int b) { return a * kDdcArrayMax + b; }
SDR_DDC_HD inline int ddc_array_cov_im(int a, int b) { return b * kDdcArrayMax + a; }
constexpr int kDdcArrayCovSlots = kDdcArrayMax * kDdcArrayMax;

}  // namespace sdr
