// SPACE-TIME weights of an array converter (sdr_ddc_create_stap, include/sydr_amd.h): a short FIR per antenna element in front of
// the mixer, x_j = sum_t sum_a conj(w[t][a]) s_a[j - t].  Shared by the host that checks the weights, the kernels of ddc.hip /
// resample.hip that combine their inputs where they load them (DdcStapLoad, ddc_handle.h), the lag-covariance pass of
// ddc_stap.hip and the host check tests/csrc/ddc_stap_check.hip.  The NumPy form is sydr_amd/signal/stap.py.
//
// A space-time array is an array (ddc_array.h: layout, K lanes) plus T taps, T in 1..8, weights w[t][a] = wr + i wi laid out
// [T][K][2].  Element a of frame i, s_a[i], is decoded exactly as the array converter decodes it and is 0 before the first
// input since creation or reset.  Input j is formed in fp64 in this order and no other -- one running pair that starts at +0.0,
// t ascending, inside each t a ascending, the array converter's four operations per (t, a), every product rounded, every sum
// rounded, nothing contracted (ddc_array_accumulate):
//     re = 0; im = 0
//     for t = 0 .. T-1:  for a = 0 .. K-1:   (sr, si) = s_a[j - t]
//         re = re + wr sr;  re = re + wi si;  im = im + wr si;  im = im - wi sr
// The converter keeps two histories.  The HISTORY is the array converter's: the last Tp - 1 COMBINED inputs, cf64 -- a weight
// change never reaches an input that has been combined.  The RAW TAIL is the last T - 1 frames of K DECODED elements, oldest
// first, [T - 1][K] pairs (re, im) of doubles (every field kind is exact in a double): slot i after n inputs holds frame
// n - (T - 1) + i, zero where that is negative.  A push's frame f, counted from the push's first, is read from the staged bytes
// for f >= 0 and from slot T - 1 + f of the tail for -(T - 1) <= f < 0; after a push of n_in frames the new slot i is frame
// n_in - (T - 1) + i of that same numbering -- of a push shorter than T - 1 frames the old slot i + n_in: the tail is SHIFTED.
#pragma once

#include "ddc_array.h"

namespace sdr {

constexpr int kDdcStapMinTaps = 1, kDdcStapMaxTaps = 8;
constexpr int kDdcStapTailUnit = 16;                    // bytes of one decoded element in the raw tail

// The weights as the kernels take them, by value: kernel arguments, read by wave-uniform (scalar) loads.
struct DdcStap {
    int T, reserved;
    double w[kDdcStapMaxTaps][kDdcArrayMax][2];
};

inline bool ddc_stap_taps_valid(int T) { return T >= kDdcStapMinTaps && T <= kDdcStapMaxTaps; }

inline bool ddc_stap_weights_valid(int T, int K, const double* w /*[T][K][2]*/) {
    for (int i = 0; i < 2 * T * K; ++i)
        if (!std::isfinite(w[i])) return false;
    return true;
}

inline void ddc_stap_set(DdcStap* s, int T, int K, const double* w /*[T][K][2]*/) {
    s->T = T, s->reserved = 0;
    for (int t = 0; t < kDdcStapMaxTaps; ++t)
        for (int a = 0; a < kDdcArrayMax; ++a) {
            const bool in = t < T && a < K;
            s->w[t][a][0] = in ? w[2 * (t * K + a)] : 0.0, s->w[t][a][1] = in ? w[2 * (t * K + a) + 1] : 0.0;
        }
}

// Bytes of the raw tail (at least one unit, so that there is always a buffer).
inline size_t ddc_stap_tail_bytes(int T, int K) { return (size_t)(T > 1 ? (T - 1) * K : 1) * kDdcStapTailUnit; }

// Element a of tail slot `slot` (0 the oldest of T - 1).
SDR_DDC_HD inline void ddc_stap_tail_load(const double* __restrict__ tail, int slot, int K, int a, double* re, double* im) {
    const double* h = tail + 2 * (slot * K + a);
    *re = h[0], *im = h[1];
}
SDR_DDC_HD inline void ddc_stap_tail_store(double* tail, int slot, int K, int a, double re, double im) {
    double* h = tail + 2 * (slot * K + a);
    h[0] = re, h[1] = im;
}

// The frame, in the push's numbering, that slot i of the tail holds AFTER a push of n_in frames: >= 0 a frame of the staged
// bytes, < 0 the old tail's slot T - 1 + f = i + n_in.
SDR_DDC_HD inline int64_t ddc_stap_tail_source(int64_t n_in, int T, int i) { return n_in - (T - 1) + i; }

// Input j of the converter (0 <= j < n_in, the push's numbering): x_j = sum_t sum_a conj(w[t][a]) s_a[j - t].
SDR_DDC_HD inline void ddc_stap_load(const void* __restrict__ p, const double* __restrict__ tail, int64_t j, const DdcLayout& l, const DdcArray& arr,
                                     const DdcStap& st, double* re, double* im) {
    double r = 0.0, i = 0.0;
    // (unrolled with constant tap and element indices, as ddc_array_load: weights and lanes stay kernel arguments)
#pragma unroll
    for (int t = 0; t < kDdcStapMaxTaps; ++t) {
        if (t >= st.T) break;
        const int64_t f = j - t;
        if (f >= 0) {
            const DdcFrame fr = ddc_array_frame(p, f, l);
#pragma unroll
            for (int a = 0; a < kDdcArrayMax; ++a) {
                if (a >= arr.K) break;
                double sr, si;
                ddc_array_element(p, f, l, fr, arr.lanes[a], &sr, &si);
                ddc_array_accumulate(st.w[t][a][0], st.w[t][a][1], sr, si, &r, &i);
            }
        } else {
            const int slot = st.T - 1 + (int)f;
#pragma unroll
            for (int a = 0; a < kDdcArrayMax; ++a) {
                if (a >= arr.K) break;
                double sr, si;
                ddc_stap_tail_load(tail, slot, arr.K, a, &sr, &si);
                ddc_array_accumulate(st.w[t][a][0], st.w[t][a][1], sr, si, &r, &i);
            }
        }
    }
    *re = r, *im = i;
}

// The same input with the T taps' weights out of a row [kDdcStapMaxTaps][kDdcArrayMax][2] of a table in device memory (an attached
// beam's: ddc_handle.h), DdcStap::w's own layout, read by wave-uniform loads: ddc_stap_load's statements on the same operands in
// the same order.  Kept apart from it: routed through one template the by-value form compiles to other code than it always had
// (17 063 instructions against 15 434 in the converter's kernel).
SDR_DDC_HD inline void ddc_stap_load_table(const void* __restrict__ p, const double* __restrict__ tail, int64_t j, const DdcLayout& l,
                                           const DdcArray& arr, int T, const double* __restrict__ w, double* re, double* im) {
    double r = 0.0, i = 0.0;
#pragma unroll
    for (int t = 0; t < kDdcStapMaxTaps; ++t) {
        if (t >= T) break;
        const int64_t f = j - t;
        const double* wt = w + 2 * (t * kDdcArrayMax);
        if (f >= 0) {
            const DdcFrame fr = ddc_array_frame(p, f, l);
#pragma unroll
            for (int a = 0; a < kDdcArrayMax; ++a) {
                if (a >= arr.K) break;
                double sr, si;
                ddc_array_element(p, f, l, fr, arr.lanes[a], &sr, &si);
                ddc_array_accumulate(wt[2 * a], wt[2 * a + 1], sr, si, &r, &i);
            }
        } else {
            const int slot = T - 1 + (int)f;
#pragma unroll
            for (int a = 0; a < kDdcArrayMax; ++a) {
                if (a >= arr.K) break;
                double sr, si;
                ddc_stap_tail_load(tail, slot, arr.K, a, &sr, &si);
                ddc_array_accumulate(wt[2 * a], wt[2 * a + 1], sr, si, &r, &i);
            }
        }
    }
    *re = r, *im = i;
}

// lanes[a] by selects (a run-time index into the by-value array would copy it to scratch memory).
SDR_DDC_HD inline int ddc_stap_lane(const DdcArray& arr, int a) {
    int lane = arr.lanes[0];
#pragma unroll
    for (int b = 1; b < kDdcArrayMax; ++b) lane = a == b ? arr.lanes[b] : lane;
    return lane;
}

// Element a of slot i of the tail AFTER a push of n_in frames whose bytes are `p`, `tail` being the old one.
SDR_DDC_HD inline void ddc_stap_tail_next(const void* __restrict__ p, const double* __restrict__ tail, int64_t n_in, const DdcLayout& l,
                                          const DdcArray& arr, int T, int i, int a, double* re, double* im) {
    const int64_t f = ddc_stap_tail_source(n_in, T, i);
    if (f >= 0) {
        const DdcFrame fr = ddc_array_frame(p, f, l);
        ddc_array_element(p, f, l, fr, ddc_stap_lane(arr, a), re, im);
    } else {
        ddc_stap_tail_load(tail, T - 1 + (int)f, arr.K, a, re, im);
    }
}

// The lag covariance's slots: lag tau has kDdcStapCovSlots of them, entry (a, b) its real part at 2 (8 a + b), its imaginary
// part behind it -- C[tau][a][b] = sum_j s_a[j] conj(s_b[j - tau]), every entry kept (no symmetry for tau > 0).
constexpr int kDdcStapCovSlots = 2 * kDdcArrayMax * kDdcArrayMax;
SDR_DDC_HD inline int ddc_stap_cov_slot(int a, int b) { return 2 * (a * kDdcArrayMax + b); }

}  // namespace sdr
