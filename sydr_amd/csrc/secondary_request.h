// What a request to sdr_acq_refine's stage 1 and to sdr_acq_secondary means and whether the engine can serve it (the contracts
// in include/sydr_amd.h).  Host code only, no engine in sight, beside acq_request.h: the checks take what they need of the
// engine as plain values, answer a status of include/sydr_amd.h and leave their text for sdr_fail -- shared with the
// stand-alone check tests/csrc/secondary_request_check.hip (`make check-sanitize`, tests/test_secondary.py).
//   refine_admit_item         one item of either call: slot staged, rates finite, window inside the ring, the code period
//                             inside the staged row and the LDS -> what the kernels need of it (RefineItemDev)
//   secondary_chips_check     the rows of secondary codes hold +1 and -1 alone (shared with coherent_request.h)
//   secondary_request_check   the whole of a sdr_acq_secondary call, items included
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/sydr_amd.h"

namespace sdr {

constexpr int kRefineMaxPeriods = 20;    // sdr_acq_refine: one data bit, at most one edge inside the window
constexpr int kRefineMaxSegments = 64;
constexpr int kRefineMaxBins = 4096;
constexpr int kRefineMaxLutWords = 16 * 1024 - 64;   // the replica of ONE period in the default 64 KB of dynamic LDS
constexpr int kRefineLutPad = 4;                     // == SDR_LUT_PAD (engine_internal.h; refine_segments.h asserts it)

constexpr int kSecMaxPeriods = 128;      // sdr_acq_secondary
constexpr int kSecMaxLen = 128;          // chips of a secondary code
constexpr int kSecMaxProducts = 2048;    // n_periods * n_segments

struct RefineItemDev {   // what the kernels need of one sdr_refine_item / sdr_sec_item
    int32_t slot, N;     // N = samples per code period
    int64_t base;        // start_sample modulo the ring's capacity
    double f0, code_step;
    int32_t lut_words;   // words of the slot's LDS image one period needs: checked against the row and the LDS here
    int32_t sec_row;     // sdr_acq_secondary: the item's row of sec_codes (sdr_acq_refine: 0)
};

struct RefineRing {      // of the engine
    int64_t capacity = 0;               // samples of the IQ ring
    int n_slots = 0;
    const int32_t* code_len = nullptr;  // [n_slots] chips staged per slot, <= 0: none
    int lut_stride = 0;                 // words of a slot's staged replica
};

// Item i of a call with M periods of S segments each.  SDR_OK: *out is filled; else `text` says what is wrong.
inline int refine_admit_item(const RefineRing& g, int i, int32_t code_slot, int64_t start_sample, double carrier_hz, double code_hz,
                             double fs, int M, int S, RefineItemDev* out, char* text, size_t text_len) {
    if (code_slot < 0 || code_slot >= g.n_slots || g.code_len[code_slot] <= 0) {
        snprintf(text, text_len, "item %d: code slot %d is not staged", i, code_slot);
        return SDR_ERR_INVALID;
    }
    if (!(code_hz > 0.0) || !std::isfinite(code_hz) || !std::isfinite(carrier_hz)) {
        snprintf(text, text_len, "item %d: non-finite carrier or non-positive code frequency", i);
        return SDR_ERR_INVALID;
    }
    if (start_sample < 0) {
        snprintf(text, text_len, "item %d: negative start_sample", i);
        return SDR_ERR_RANGE;
    }
    const int L = g.code_len[code_slot];
    const double n_exact = std::nearbyint(fs * (double)L / code_hz);   // samples per code period
    if (!(n_exact >= 1.0) || n_exact * M > (double)g.capacity) {
        snprintf(text, text_len, "item %d: a window of %d code periods of %.0f samples, ring holds %lld", i, M, n_exact,
                 (long long)g.capacity);
        return SDR_ERR_RANGE;
    }
    if (n_exact > (double)(1 << 30)) {
        snprintf(text, text_len, "item %d: a code period of %.0f samples (at most 2^30)", i, n_exact);
        return SDR_ERR_UNSUPPORTED;
    }
    const int N = (int)n_exact;
    if (S > N) {
        snprintf(text, text_len, "item %d: %d segments in a code period of %d samples", i, S, N);
        return SDR_ERR_UNSUPPORTED;
    }
    const double code_step = code_hz / fs;
    // the chip indices a period reaches (ceil(N * code_step) + 1 at most) must lie inside the staged row and fit the LDS
    const double words_exact = std::ceil((double)N * code_step) + kRefineLutPad + 4;
    if (!(words_exact <= (double)g.lut_stride) || !(words_exact <= (double)kRefineMaxLutWords)) {
        snprintf(text, text_len, "item %d: a code period of %d chips (at most %d)", i, L,
                 std::min(g.lut_stride, kRefineMaxLutWords) - kRefineLutPad - 4);
        return SDR_ERR_UNSUPPORTED;
    }
    *out = RefineItemDev{code_slot, N, start_sample % g.capacity, carrier_hz, code_step, (int32_t)words_exact, 0};
    return SDR_OK;
}

// Every chip of the secondary rows [n_sec][sec_len] is +1 or -1 (sdr_acq_secondary, sdr_pcps_coherent).
inline int secondary_chips_check(const int8_t* sec_codes, int n_sec, int sec_len, char* text, size_t text_len) {
    for (int64_t q = 0; q < (int64_t)n_sec * sec_len; ++q)
        if (sec_codes[q] != 1 && sec_codes[q] != -1) {
            snprintf(text, text_len, "secondary code %d, chip %d: %d is neither +1 nor -1", (int)(q / sec_len), (int)(q % sec_len),
                     (int)sec_codes[q]);
            return SDR_ERR_INVALID;
        }
    return SDR_OK;
}

struct SecRequest {
    // of the engine
    bool ring = false, slots_allocated = false;
    RefineRing g;
    // of the call
    const sdr_sec_item* items = nullptr;
    int n_items = 0;
    const int8_t* sec_codes = nullptr;  // [n_sec][sec_len]
    int n_sec = 0, sec_len = 0;
    double fs = 0.0;
    int n_periods = 0, n_segments = 0;
    double span_hz = 0.0, step_hz = 0.0;
    int K = 0;                          // sdr_acq_refine_bins(span_hz, step_hz): the one helper the grid's length comes from
    int mode = 0;
    bool results = false;               // the results pointer is not NULL
};

struct SecShape {
    int max_words = 0;                  // the longest replica of one period among the items, in words
    char text[200] = {0};               // what is wrong, for sdr_last_error
};

// dev (nullable): [n_items] records filled for the items admitted so far.
inline int secondary_request_check(const SecRequest& r, SecShape* s, RefineItemDev* dev) {
    auto fail = [&](int status, const char* what) {
        snprintf(s->text, sizeof s->text, "%s", what);
        return status;
    };
    *s = SecShape{};
    if (!r.ring) return fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!r.slots_allocated) return fail(SDR_ERR_STATE, "code slots not allocated");
    if (!r.items || r.n_items <= 0 || r.n_items > 65535) return fail(SDR_ERR_INVALID, "no item to search");
    if (!r.results) return fail(SDR_ERR_INVALID, "results is NULL");
    if (!r.sec_codes) return fail(SDR_ERR_INVALID, "sec_codes is NULL");
    if (!(r.fs > 0.0) || !std::isfinite(r.fs)) return fail(SDR_ERR_INVALID, "bad sampling frequency");
    const int M = r.n_periods, S = r.n_segments;
    if (M < 2 || M > kSecMaxPeriods) {
        snprintf(s->text, sizeof s->text, "n_periods %d outside 2..%d", M, kSecMaxPeriods);
        return SDR_ERR_INVALID;
    }
    if (S < 1 || S > kRefineMaxSegments) {
        snprintf(s->text, sizeof s->text, "n_segments %d outside 1..%d", S, kRefineMaxSegments);
        return SDR_ERR_INVALID;
    }
    if (r.sec_len < 2 || r.sec_len > kSecMaxLen) {
        snprintf(s->text, sizeof s->text, "sec_len %d outside 2..%d", r.sec_len, kSecMaxLen);
        return SDR_ERR_INVALID;
    }
    if (r.n_sec < 1 || r.n_sec > r.n_items) {
        snprintf(s->text, sizeof s->text, "n_sec %d outside 1..n_items = %d", r.n_sec, r.n_items);
        return SDR_ERR_INVALID;
    }
    if (r.mode != SDR_SEC_PILOT && r.mode != SDR_SEC_DATA) return fail(SDR_ERR_INVALID, "mode is neither SDR_SEC_PILOT nor SDR_SEC_DATA");
    if (r.K <= 0 || !std::isfinite(r.span_hz) || !std::isfinite(r.step_hz)) return fail(SDR_ERR_INVALID, "bad fine frequency grid");
    if (int rc = secondary_chips_check(r.sec_codes, r.n_sec, r.sec_len, s->text, sizeof s->text)) return rc;
    if (M * S > kSecMaxProducts) {
        snprintf(s->text, sizeof s->text, "%d periods of %d segments (at most %d segments in all)", M, S, kSecMaxProducts);
        return SDR_ERR_UNSUPPORTED;
    }
    if (r.K > kRefineMaxBins) {
        snprintf(s->text, sizeof s->text, "fine grid of %d frequencies (at most %d)", r.K, kRefineMaxBins);
        return SDR_ERR_UNSUPPORTED;
    }
    for (int i = 0; i < r.n_items; ++i) {
        const sdr_sec_item& it = r.items[i];
        if (it.sec_row < 0 || it.sec_row >= r.n_sec) {
            snprintf(s->text, sizeof s->text, "item %d: sec_row %d outside the %d rows of sec_codes", i, it.sec_row, r.n_sec);
            return SDR_ERR_INVALID;
        }
        RefineItemDev d;
        if (int rc = refine_admit_item(r.g, i, it.code_slot, it.start_sample, it.carrier_hz, it.code_hz, r.fs, M, S, &d, s->text,
                                       sizeof s->text))
            return rc;
        d.sec_row = it.sec_row;
        s->max_words = std::max(s->max_words, (int)d.lut_words);
        if (dev) dev[i] = d;
    }
    return SDR_OK;
}

}  // namespace sdr
