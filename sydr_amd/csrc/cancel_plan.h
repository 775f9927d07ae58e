// What sdr_iq_cancel (cancel.hip) checks of its item lists before anything is launched, and what it makes of them -- host code
// only, shared with the stand-alone check tests/csrc/cancel_plan_check.hip (`make check-sanitize`), which feeds it hostile
// lists under the address and undefined-behaviour sanitizers.
//
// A window of W samples starts at ring index w0; an item of n samples sits at window offset
//     off = (start_sample - w0) mod capacity
// and must lie wholly inside the window (off + n <= W).  Within a channel the offsets ascend and do not overlap; gaps are
// allowed; items with n_samples == 0 are padding and are dropped here.  What is left goes to the device as one dense list
// per channel (CancelItemDev, count[ch] of them at [ch * n_epochs]), in which the kernel finds the first epoch that reaches
// into a tile by binary search over `off + n`.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/sydr_amd.h"
#include "corr_bounds.h"

namespace sdr {

struct CancelItemDev {     // what the kernel needs of one item
    int64_t off;           // window offset of its first sample
    int32_t n, L;          // samples; chips staged in its slot
    int32_t slot, reserved;
    double w;              // (carrier_hz * 2.0) * pi: the statement's own first two products
    double rem_carrier;
    double shift, step;    // the chip line of the prompt tap: idx_i = ceil(i * step + shift) (corr_bounds.h corr_tap, spacing 0.0)
    double a_re, a_im;
};

enum CancelPlanError { CANCEL_OK = 0, CANCEL_INVALID, CANCEL_RANGE, CANCEL_UNSUPPORTED };

struct CancelPlan {
    std::vector<CancelItemDev> items;   // [n_ch][n_epochs], the first count[ch] of a row in use
    std::vector<int32_t> count;         // [n_ch]
    char text[160];                     // what is wrong, for sdr_last_error
};

// (a - b) mod m for 0 <= a, b and m > 0, without leaving int64
inline int64_t cancel_mod_diff(int64_t a, int64_t b, int64_t m) {
    const int64_t d = a % m - b % m;
    return d < 0 ? d + m : d;
}

// Two windows of W samples (1 <= W <= capacity) at ring indices a and b of one ring: do they share a sample?
inline bool cancel_windows_overlap(int64_t a, int64_t b, int64_t W, int64_t capacity) {
    const int64_t d = cancel_mod_diff(b, a, capacity);
    return d < W || capacity - d < W;
}

inline int cancel_plan(const sdr_epl_item* items, const double* amps, int n_ch, int n_epochs, int64_t w0, int64_t W,
                       int64_t capacity, int n_slots, const int32_t* code_len, CancelPlan* plan) {
    auto fail = [&](int code, const char* what, int ch, int k) {
        snprintf(plan->text, sizeof plan->text, "channel %d, item %d: %s", ch, k, what);
        return code;
    };
    auto finite = [](double x) { return x - x == 0.0; };
    plan->text[0] = 0;
    plan->items.assign((size_t)n_ch * (size_t)n_epochs, CancelItemDev{});
    plan->count.assign((size_t)n_ch, 0);
    for (int ch = 0; ch < n_ch; ++ch) {
        int64_t end = 0;   // window offset behind the channel's last item so far
        for (int k = 0; k < n_epochs; ++k) {
            const size_t at = (size_t)ch * (size_t)n_epochs + (size_t)k;
            const sdr_epl_item& it = items[at];
            if (it.n_samples == 0) continue;
            if (it.n_samples < 0) return fail(CANCEL_INVALID, "negative n_samples", ch, k);
            if (it.code_slot < 0 || it.code_slot >= n_slots || code_len[it.code_slot] <= 0)
                return fail(CANCEL_INVALID, "its code slot is not staged", ch, k);
            const double a_re = amps[2 * at], a_im = amps[2 * at + 1];
            if (!finite(a_re) || !finite(a_im)) return fail(CANCEL_INVALID, "non-finite amplitude", ch, k);
            if (!(it.code_step > 0.0) || !finite(it.code_step) || !finite(it.rem_code) || !finite(it.rem_carrier) ||
                !finite(it.carrier_hz))
                return fail(CANCEL_INVALID, "non-finite NCO parameters or non-positive code_step", ch, k);
            if (it.start_sample < 0) return fail(CANCEL_RANGE, "negative start_sample", ch, k);
            const int64_t off = cancel_mod_diff(it.start_sample, w0, capacity);
            if (off >= W || (int64_t)it.n_samples > W - off) return fail(CANCEL_RANGE, "not wholly inside the window", ch, k);
            if (off < end) return fail(CANCEL_INVALID, "overlaps the item in front of it or does not ascend", ch, k);
            end = off + it.n_samples;
            // every padded chip index inside +-2^30 (sdr_corr_profile's rule; false for NaN / Inf as well)
            const double lo = std::ceil(it.rem_code + 0.0);
            const double hi = std::ceil(it.code_step * (double)it.n_samples + it.rem_code + 0.0);
            if (!(lo >= -1073741824.0) || !(hi <= 1073741824.0)) return fail(CANCEL_UNSUPPORTED, "chip indices leave +-2^30", ch, k);
            CancelItemDev& d = plan->items[(size_t)ch * (size_t)n_epochs + (size_t)plan->count[(size_t)ch]++];
            d.off = off, d.n = it.n_samples, d.L = code_len[it.code_slot], d.slot = it.code_slot, d.reserved = 0;
            d.w = (it.carrier_hz * 2.0) * M_PI;
            if (!finite(d.w)) return fail(CANCEL_INVALID, "carrier_hz * 2 * pi overflows", ch, k);
            const CorrTap tap = corr_tap(it.n_samples, it.rem_code, it.code_step, 0.0);
            d.rem_carrier = it.rem_carrier, d.shift = tap.shift, d.step = tap.step;
            d.a_re = a_re, d.a_im = a_im;
        }
    }
    return CANCEL_OK;
}

}  // namespace sdr
