// Every decision of an E/P/L plan's creation (epl_plan.hip) as a function of plain values: the rules a list's items are
// checked by, the fold of their statistics into a variant word, the half-chip view, the period of the code slots, the
// several-chips-per-lane shape, the route -- which side checks the list, where its setups are made, how its spacings travel,
// whether the creation waits -- and the layout of the page-locked scratch.  Host arithmetic only, no engine and no call of the
// runtime: tests/csrc/epl_plan_check.hip compiles it alone (tests/test_epl_plan.py, `make check-sanitize`).
#pragma once

#include <cmath>
#include <cstring>

#include "epl_items.h"
#include "epl_variant.h"

// What the decisions read of the engine: its ring format and the diagnostics switches "epl_no_chip", "epl_no_double",
// "epl_no_chip2", "epl_no_split".
struct PlanSwitches {
    int iq_fmt;
    bool no_chip, no_double, no_chip2, no_split;
};

// n_slots, lut_stride, iq_capacity: the engine's staged slots, the row length of its replica tables, its ring.
inline ItemRules item_rules(int n_slots, int lut_stride, int64_t iq_capacity, const double* spacing, int n_taps, double scale) {
    ItemRules r = {};
    r.n_slots = n_slots;
    r.lut_stride = lut_stride;
    r.n_taps = n_taps;
    r.iq_capacity = iq_capacity;
    r.scale = scale;
    r.smin = r.smax = spacing[0];
    for (int t = 1; t < n_taps; ++t) {
        r.smin = spacing[t] < r.smin ? spacing[t] : r.smin;
        r.smax = spacing[t] > r.smax ? spacing[t] : r.smax;
    }
    r.s_anchor = scale * spacing[n_taps < 5 ? n_taps / 2 : 2];   // centre tap of the first chunk of taps the kernels serve together
    r.sp0 = spacing[0];
    r.sp2 = n_taps >= 3 ? spacing[2] : 0.0;
    r.want_s12 = n_taps == 3;   // both outer taps switch chips 12.x samples into the anchor's block (KS = 12 kernel)
    return r;
}

// ---- the statistics of a list, folded item by item (the host's walk) or merged from parts (what validate_items_kernel's
// atomics leave of its threads' shares: the same operations, on the initial value the host wrote)
constexpr int kNoBadItem = 0x7fffffff;
inline ItemStats item_stats_initial(bool want_s12) { return ItemStats{kNoBadItem, 0, 0, 0ull, ~0ull, kNoBadItem, 0, want_s12 ? 1 : 0}; }

inline void item_stats_merge(ItemStats& s, const ItemStats& o) {
    if (o.first_bad < s.first_bad) s.first_bad = o.first_bad, s.bad_code = o.bad_code;
    s.maxlen = o.maxlen > s.maxlen ? o.maxlen : s.maxlen;
    s.max_step_bits = o.max_step_bits > s.max_step_bits ? o.max_step_bits : s.max_step_bits;
    s.min_step_bits = o.min_step_bits < s.min_step_bits ? o.min_step_bits : s.min_step_bits;
    s.m_lo = o.m_lo < s.m_lo ? o.m_lo : s.m_lo;
    s.m_hi = o.m_hi > s.m_hi ? o.m_hi : s.m_hi;
    s.all_split &= o.all_split;
}

// One result of check_item: `bad` (ITEM_OK: maxlen, step, m_chip and split are the item's share; else they mean nothing).
inline void item_stats_add(ItemStats& s, int index, int bad, int maxlen, double step, int m_chip, bool split) {
    unsigned long long sb;
    std::memcpy(&sb, &step, sizeof(sb));
    item_stats_merge(s, bad ? ItemStats{index, bad, 0, 0ull, ~0ull, kNoBadItem, 0, 1} : ItemStats{kNoBadItem, 0, maxlen, sb, sb, m_chip, m_chip, split ? 1 : 0});
}

// What a list of these statistics gets: its lowest bad item (kNoBadItem: none; else the rest means nothing), the words of a
// replica its kernels stage, its variant word (epl_variant.h: choose_variant).
struct ListVerdict { int first_bad, lut_words, word; };
inline ListVerdict list_verdict(const ItemStats& s, const ItemRules& r, const double* spacing, const PlanSwitches& sw) {
    if (s.first_bad != kNoBadItem) return {s.first_bad, 0, 0};
    VariantInputs v = {};
    v.n_taps = r.n_taps, v.scale = r.scale, v.s_anchor = r.s_anchor, v.spacing = spacing;
    std::memcpy(&v.max_step, &s.max_step_bits, sizeof(double));
    std::memcpy(&v.min_step, &s.min_step_bits, sizeof(double));
    v.m_lo = s.m_lo, v.m_hi = s.m_hi, v.all_split = s.all_split != 0;
    v.iq_fmt = sw.iq_fmt, v.lut_stride = r.lut_stride, v.no_chip = sw.no_chip, v.no_split = sw.no_split;
    return {kNoBadItem, s.maxlen + SDR_LUT_PAD + 2, choose_variant(v)};
}

// ---- the half-chip view: a list that misses the chip-aligned correlator only because a chip holds too many samples (32-52:
// GPS L1 C/A at 50 MHz) runs on the view of its replicas with every chip twice.  ok2 / wide2: the rules of scale 2 were met,
// and their word; lut2_stride: the row length of the doubled tables (known once they exist: read only where the view is taken).
inline bool half_chip_view_allowed(int word, const PlanSwitches& sw) {
    return !variant_chip_aligned(word) && sw.iq_fmt == SDR_FMT_CI8 && !sw.no_chip && !sw.no_double;
}
struct HalfChipView { bool taken; int word, lut_words; };
inline HalfChipView half_chip_view(int word, bool ok2, int wide2, const PlanSwitches& sw, int lut_words, int lut2_stride) {
    if (!(half_chip_view_allowed(word, sw) && ok2 && variant_chip_aligned(wide2))) return {false, word, lut_words};
    return {true, wide2, 2 * lut_words < lut2_stride ? 2 * lut_words : lut2_stride};
}

// ---- the period C of the code-slot pattern: code_slot[i] == code_slot[i + C] for every i (what lets four epochs of a channel
// share a staged table), 0: the list has none.  stride_bytes: from one item's code_slot to the next one's.
inline int group_stride(const int32_t* code_slot, size_t stride_bytes, int n_items) {
    auto slot = [&](int i) { return *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(code_slot) + (size_t)i * stride_bytes); };
    int c = 1;
    while (c < n_items && slot(c) != slot(0)) ++c;
    bool periodic = c < n_items || n_items == 1;
    for (int i = 0; periodic && i + c < n_items; ++i) periodic = slot(i) == slot(i + c);
    return periodic ? c : 0;
}

// ---- several chips per lane (correlator_chip2.h; SDR_EPL_CHIPN_SHAPES): three taps half a chip apart and chips of 9.5 .. 10 or
// 11.5 .. 12 samples (the reference's shipped 10 MHz; 12 MHz): two chips per lane, if (nearly) every item fits the scheme.  (At
// 24 .. 24.5 samples per chip -- boundaries <12, 24, 36, 48> -- the same kernel was measured against the one-chip form: 5 % fewer
// instructions per sample, 60 % more per epoch, at the register cap: 0.335 instead of 0.316 ms per 32 000 epochs; three chips per
// lane at 10 MHz -- <4, 9, 14, 19, 24, 29> -- spill 27 registers at three waves per SIMD: 0.44 instead of 0.57 of the roof.
// Neither is instantiated.)  ... and chips of 3.75 .. 4 samples (the reference's 4 MHz, BASELINE configs[0]): FOUR chips per
// lane, where the list would otherwise go per sample (round 6).
// form: decode() of the list's word.  (Long multi-period replicas keep the four-epochs-per-workgroup kernels.)
inline bool shape_possible(const EplForm& form, int n_taps, const PlanSwitches& sw, bool doubled, int lut_words) {
    return sw.iq_fmt == SDR_FMT_CI8 && n_taps == 3 && !doubled && !sw.no_chip2 && (form.w == 8 || form.w == 0) && lut_words < kLongLutWords;
}
// The shape (1 .. 3; 0: none) a list asks for.  code_step: its first item's (any positive step got here).
inline int list_shape(const EplForm& form, double code_step, const double* spacing, int n_taps, const PlanSwitches& sw, bool doubled,
                      int lut_words) {
    if (!shape_possible(form, n_taps, sw, doubled, lut_words)) return 0;
    const double two_chips = std::floor(2.0 / code_step), four_chips = std::floor(4.0 / code_step);   // samples in two, in four chips
    const bool half_apart = spacing[0] == -0.5 && spacing[1] == 0.0 && spacing[2] == 0.5;
    return form.w == 8 ? (two_chips == 19.0 ? 1 : (two_chips == 23.0 ? 2 : 0)) : (four_chips == 15.0 && half_apart ? 3 : 0);
}
// missed: the items the scheme does not cover (the kernel redoes them per sample).  Too many strays: the boundary variant
// serves the list.
inline bool shape_kept(int n_items, int missed) { return missed <= n_items / 64; }

// ---- the route of a creation
constexpr int kLongList = 4096;
// A short list is checked by the host before anything is allocated (one call per EPL(): latency); a long one, or one that is
// in device memory, by one thread per item behind its upload.
inline bool list_is_long(int n_items, bool in_device_memory) { return in_device_memory || n_items >= kLongList; }

enum SetupsOn { kSetupsOnHost, kSetupsOnEngineStream, kSetupsOnPlanStream };
struct PlanRoute {
    bool check_on_device;        // (else: by the host's walk)
    SetupsOn setups;             // where the per-item setups are made, if the list has any
    bool spacings_with_check;    // the spacings that travel with a long list's check are the plan's (else: sent afterwards)
    bool spacings_via_scratch;   // ... afterwards, out of the page-locked scratch (else: out of the caller's memory)
    bool ahead;                  // the creation ends with `ready` recorded behind the setups (else: with a wait of the engine's stream)
};
// use_workspaces: sdr_epl_batch's shared buffers; doubled: the half-chip view; row_setups: the word names a straight-line
// kernel with a ChipSetup per item; shape: list_shape().  Only a long list's row setups leave the engine's stream: a short
// list's are made by the host, the half-chip view's read items and spacings that are queued on the engine's stream, the shared
// workspaces serve the next call, and a shape's count of strays is waited for.
inline PlanRoute plan_route(int n_items, bool in_device_memory, bool use_workspaces, bool doubled, bool row_setups, int shape) {
    PlanRoute r = {};
    r.check_on_device = list_is_long(n_items, in_device_memory);
    r.setups = !r.check_on_device ? kSetupsOnHost
               : row_setups && shape == 0 && !doubled && !use_workspaces ? kSetupsOnPlanStream : kSetupsOnEngineStream;
    r.spacings_with_check = r.check_on_device && !doubled;
    r.spacings_via_scratch = r.check_on_device && doubled;
    r.ahead = r.setups == kSetupsOnPlanStream;
    return r;
}

// ---- the page-locked scratch of a long list's creation (StreamCtx::pinned of the engine's stream): the statistics of the
// two rule sets, then the tap spacings.
constexpr size_t kPlanPinnedBytes = 2 * sizeof(ItemStats) + SDR_MAX_TAPS * sizeof(double);
inline ItemStats* plan_pinned_stats(void* pinned) { return static_cast<ItemStats*>(pinned); }
inline double* plan_pinned_spacing(void* pinned) { return reinterpret_cast<double*>(static_cast<char*>(pinned) + 2 * sizeof(ItemStats)); }
