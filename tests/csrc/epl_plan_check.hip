// Host-side proof of the decisions of an E/P/L plan's creation (sydr_amd/csrc/epl_plan.h), built with `hipcc --cuda-host-only`
// (tests/test_epl_plan.py; under the address and undefined-behaviour sanitizers by `make check-sanitize`).  The expected values
// are written out here, from what plan_create_impl did while these decisions were spelled inside it:
//  - the route: which side checks a list, where its setups are made, how its spacings travel, whether the creation waits;
//  - the several-chips-per-lane shape a list asks for, and the rule that keeps it;
//  - group_stride, the half-chip view, item_rules, the layout of the page-locked scratch;
//  - the fold of a list's statistics: item by item and merged from seven scrambled parts it gives what the host's walk of old
//    (restated below) gave, and the lowest of the bad items planted in the list.
//   usage: epl_plan_check   -> "ok <checks>" and exit status 0, or the first failed check and 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sydr_amd/csrc/epl_plan.h"

static long checks = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        ++checks;                                                           \
        if (!(cond)) return printf("line %d: %s\n", __LINE__, #cond), 1;    \
    } while (0)

static bool same(const ItemStats& a, const ItemStats& b) {
    return a.first_bad == b.first_bad && a.maxlen == b.maxlen && a.max_step_bits == b.max_step_bits && a.min_step_bits == b.min_step_bits &&
           a.m_lo == b.m_lo && a.m_hi == b.m_hi && a.all_split == b.all_split;
}

// The host's walk as sdr_epl_plan_create had it before the fold existed: six locals, the first bad item ends it.
static int walk_of_old(const std::vector<sdr_epl_item>& items, const ItemRules& r, const int32_t* code_len, const double* spacing,
                       const PlanSwitches& sw, int* lut_words, int* word) {
    int maxlen = 0, m_lo = 0x7fffffff, m_hi = 0;
    double max_step = 0.0, min_step = 1e300;
    bool all_split = r.want_s12;
    for (size_t i = 0; i < items.size(); ++i) {
        int ml = 0, m_chip = 0;
        double step = 0.0, lo = 0.0, hi = 0.0;
        bool split = true;
        if (check_item(items[i], r, code_len, ml, step, m_chip, split, lo, hi)) return (int)i;
        m_lo = m_chip < m_lo ? m_chip : m_lo;
        m_hi = m_chip > m_hi ? m_chip : m_hi;
        all_split = all_split && split;
        if (step > max_step) max_step = step;
        if (step < min_step) min_step = step;
        if (ml > maxlen) maxlen = ml;
    }
    *lut_words = maxlen + SDR_LUT_PAD + 2;
    VariantInputs v = {};
    v.n_taps = r.n_taps, v.scale = r.scale, v.s_anchor = r.s_anchor, v.spacing = spacing;
    v.max_step = max_step, v.min_step = min_step, v.m_lo = m_lo, v.m_hi = m_hi, v.all_split = all_split;
    v.iq_fmt = sw.iq_fmt, v.lut_stride = r.lut_stride, v.no_chip = sw.no_chip, v.no_split = sw.no_split;
    *word = choose_variant(v);
    return -1;
}

static ItemStats fold(const std::vector<sdr_epl_item>& items, size_t begin, size_t end, const ItemRules& r, const int32_t* code_len) {
    ItemStats s = item_stats_initial(r.want_s12);
    for (size_t i = begin; i < end; ++i) {
        int ml = 0, m_chip = 0;
        double step = 0.0, lo = 0.0, hi = 0.0;
        bool split = true;
        const int bad = check_item(items[i], r, code_len, ml, step, m_chip, split, lo, hi);
        item_stats_add(s, (int)i, bad, ml, step, m_chip, split);
    }
    return s;
}

int main() {
    const PlanSwitches plain = {SDR_FMT_CI8, false, false, false, false};
    // ---- the route: plan_route(n_items, in device memory, use_workspaces, doubled, row setups, shape)
    {
        PlanRoute r = plan_route(4095, false, false, false, true, 0);      // a short list: all on the host, one wait at the end
        CHECK(!r.check_on_device && r.setups == kSetupsOnHost && !r.ahead && !r.spacings_with_check && !r.spacings_via_scratch);
        r = plan_route(4095, false, false, true, true, 0);                 // ... on the half-chip view: its spacings out of the creation's array
        CHECK(!r.check_on_device && r.setups == kSetupsOnHost && !r.ahead && !r.spacings_with_check && !r.spacings_via_scratch);
        r = plan_route(4096, false, false, false, true, 0);                // a long list, buffers of its own, row setups: ahead
        CHECK(r.check_on_device && r.setups == kSetupsOnPlanStream && r.ahead && r.spacings_with_check && !r.spacings_via_scratch);
        r = plan_route(4096, false, false, false, false, 0);               // ... whose word has no setups: nothing to be ahead of
        CHECK(r.check_on_device && !r.ahead && r.spacings_with_check && !r.spacings_via_scratch);
        r = plan_route(1, true, false, false, true, 0);                    // a list in device memory is long at any length
        CHECK(r.check_on_device && r.setups != kSetupsOnHost && r.setups == kSetupsOnPlanStream && r.ahead && r.spacings_with_check);
        r = plan_route(4096, false, true, false, true, 0);                 // sdr_epl_batch's workspaces keep the engine's stream
        CHECK(r.check_on_device && r.setups == kSetupsOnEngineStream && !r.ahead && r.spacings_with_check && !r.spacings_via_scratch);
        r = plan_route(4096, false, false, true, true, 0);                 // the half-chip view, pool buffers
        CHECK(r.check_on_device && r.setups == kSetupsOnEngineStream && !r.ahead && !r.spacings_with_check && r.spacings_via_scratch);
        r = plan_route(4096, false, false, false, false, 1);               // a shape: its count of strays is waited for
        CHECK(r.check_on_device && r.setups == kSetupsOnEngineStream && !r.ahead && r.spacings_with_check && !r.spacings_via_scratch);
        CHECK(kLongList == 4096 && !list_is_long(4095, false) && list_is_long(4096, false) && list_is_long(1, true));
    }
    // ---- the shape a list asks for
    {
        const double half[4] = {-0.5, 0.0, 0.5, 1.0}, quarter[3] = {-0.25, 0.0, 0.25};
        const EplForm w8 = decode(8, SDR_FMT_CI8, 3, 1, true), w0 = decode(0, SDR_FMT_CI8, 3, 1, true);
        CHECK(w8.w == 8 && w0.w == 0 && !w8.setups && !w0.setups);
        const double s19 = 2.0 / 19.5, s23 = 2.0 / 23.5, s20 = 2.0 / 20.5, s15 = 4.0 / 15.5;   // floor(2 / step): 19, 23, 20; floor(4 / step): 15
        CHECK(list_shape(w8, s19, half, 3, plain, false, 1033) == 1);
        CHECK(list_shape(w8, s23, half, 3, plain, false, 1033) == 2);
        CHECK(list_shape(w8, s20, half, 3, plain, false, 1033) == 0);
        CHECK(list_shape(w8, s19, quarter, 3, plain, false, 1033) == 1);      // (two chips per lane: at any spacing)
        CHECK(list_shape(w0, s15, half, 3, plain, false, 1033) == 3);
        CHECK(list_shape(w0, s15, quarter, 3, plain, false, 1033) == 0);
        CHECK(list_shape(decode(16, SDR_FMT_CI8, 3, 1, true), s19, half, 3, plain, false, 1033) == 0);
        // each of these alone: none
        PlanSwitches no_chip2 = plain, ci16 = plain;
        no_chip2.no_chip2 = true, ci16.iq_fmt = SDR_FMT_CI16;
        CHECK(list_shape(w8, s19, half, 3, plain, true, 1033) == 0);
        CHECK(list_shape(w8, s19, half, 3, no_chip2, false, 1033) == 0);
        CHECK(list_shape(w8, s19, half, 4, plain, false, 1033) == 0);
        CHECK(list_shape(decode(8, SDR_FMT_CI16, 3, 1, true), s19, half, 3, ci16, false, 1033) == 0);
        CHECK(kLongLutWords == 4096 && list_shape(w8, s19, half, 3, plain, false, 4095) == 1 && list_shape(w8, s19, half, 3, plain, false, 4096) == 0);
        CHECK(list_shape(w0, s15, half, 3, plain, true, 1033) == 0 && list_shape(w0, s15, half, 3, no_chip2, false, 1033) == 0 &&
              list_shape(w0, s15, half, 4, plain, false, 1033) == 0 && list_shape(w0, s15, half, 3, plain, false, 4096) == 0);
        // strays
        CHECK(shape_kept(64, 1) && !shape_kept(63, 1) && shape_kept(63, 0) && !shape_kept(127, 2) && shape_kept(128, 2));
    }
    // ---- group_stride
    {
        const int32_t a[7] = {0, 1, 2, 0, 1, 2, 0}, b[4] = {0, 1, 0, 2}, same5[5] = {3, 3, 3, 3, 3}, distinct[4] = {0, 1, 2, 3}, c[5] = {0, 1, 0, 1, 1};
        CHECK(group_stride(a, sizeof(int32_t), 7) == 3);
        CHECK(group_stride(b, sizeof(int32_t), 4) == 0);
        CHECK(group_stride(a, sizeof(int32_t), 1) == 1);
        CHECK(group_stride(same5, sizeof(int32_t), 5) == 1);
        CHECK(group_stride(distinct, sizeof(int32_t), 4) == 0 && group_stride(distinct, sizeof(int32_t), 2) == 0);
        CHECK(group_stride(c, sizeof(int32_t), 5) == 0 && group_stride(c, sizeof(int32_t), 4) == 2);
        sdr_epl_item items[8] = {};      // (as creation reads them: the slots of a list of items; 8 items over 2 slots)
        for (int i = 0; i < 8; ++i) items[i].code_slot = i % 2, items[i].n_samples = 7 - i;
        CHECK(group_stride(&items[0].code_slot, sizeof(sdr_epl_item), 8) == 2);
    }
    // ---- the half-chip view
    {
        const int aligned = kVariantChip + 24 + 256 * 12, boundary = 16;
        CHECK(variant_chip_aligned(aligned) && !variant_chip_aligned(boundary) && !variant_chip_aligned(0));
        HalfChipView v = half_chip_view(boundary, true, aligned, plain, 1033, 2076);
        CHECK(v.taken && v.word == aligned && v.lut_words == 2066);          // (2 * lut_words, under the doubled tables' row)
        v = half_chip_view(0, true, aligned, plain, 1040, 2076);
        CHECK(v.taken && v.word == aligned && v.lut_words == 2076);          // (... capped by it)
        v = half_chip_view(boundary, true, aligned, plain, 1038, 2076);
        CHECK(v.taken && v.lut_words == 2076);
        PlanSwitches ci16 = plain, no_chip = plain, no_double = plain;
        ci16.iq_fmt = SDR_FMT_CI16, no_chip.no_chip = true, no_double.no_double = true;
        CHECK(half_chip_view_allowed(boundary, plain) && !half_chip_view_allowed(aligned, plain) && !half_chip_view_allowed(boundary, ci16) &&
              !half_chip_view_allowed(boundary, no_chip) && !half_chip_view_allowed(boundary, no_double));
        const HalfChipView not_taken[] = {half_chip_view(kVariantChip, true, aligned, plain, 1033, 2076), half_chip_view(boundary, true, aligned, ci16, 1033, 2076),
                                          half_chip_view(boundary, true, aligned, no_chip, 1033, 2076), half_chip_view(boundary, true, aligned, no_double, 1033, 2076),
                                          half_chip_view(boundary, false, aligned, plain, 1033, 2076), half_chip_view(boundary, true, 8, plain, 1033, 2076)};
        for (const HalfChipView& n : not_taken) CHECK(!n.taken && n.lut_words == 1033 && (n.word == boundary || n.word == kVariantChip));
    }
    // ---- item_rules, the scratch
    {
        const double sp[5] = {-1.0, -0.5, 0.25, 0.5, 1.5};
        ItemRules r = item_rules(4, 1041, 1 << 20, sp, 5, 2.0);
        CHECK(r.n_slots == 4 && r.lut_stride == 1041 && r.n_taps == 5 && r.iq_capacity == 1 << 20 && r.scale == 2.0 && r.smin == -1.0 &&
              r.smax == 1.5 && r.s_anchor == 0.5 && r.sp0 == -1.0 && r.sp2 == 0.25 && !r.want_s12);
        r = item_rules(4, 1041, 1 << 20, sp, 3, 1.0);
        CHECK(r.smin == -1.0 && r.smax == 0.25 && r.s_anchor == -0.5 && r.sp2 == 0.25 && r.want_s12);
        r = item_rules(4, 1041, 1 << 20, sp, 2, 1.0);
        CHECK(r.smax == -0.5 && r.s_anchor == -0.5 && r.sp2 == 0.0 && !r.want_s12);
        r = item_rules(4, 1041, 1 << 20, sp, 1, 1.0);
        CHECK(r.smin == -1.0 && r.smax == -1.0 && r.s_anchor == -1.0);
        alignas(16) char scratch[kPlanPinnedBytes];
        CHECK(kPlanPinnedBytes == 2 * sizeof(ItemStats) + SDR_MAX_TAPS * sizeof(double));
        CHECK((char*)plan_pinned_stats(scratch) == scratch && (char*)plan_pinned_spacing(scratch) == scratch + 2 * sizeof(ItemStats));
    }
    // ---- the fold: 5000 honest items of tests/csrc/fuzz_items.hip's generator
    {
        uint64_t state = 20260021ull * 6364136223846793005ull + 1442695040888963407ull;
        auto rnd = [&]() {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            return state >> 11;
        };
        auto uni = [&]() { return (double)rnd() / 9007199254740992.0; };
        const int32_t code_len[4] = {1023, 1023, 0, 4092};
        const double spacing[3] = {-0.5, 0.0, 0.5};
        const double rates[7] = {4e6, 10e6, 12e6, 16.368e6, 20e6, 25e6, 50e6};
        for (int one_rate = 0; one_rate < 2; ++one_rate) {      // (every rate in one list; then 25 MHz alone: a chip-aligned word)
            std::vector<sdr_epl_item> items(5000);
            for (sdr_epl_item& it : items) {
                const double fs = one_rate ? 25e6 : rates[rnd() % 7];
                const double step = 1.023e6 * (1.0 + (uni() - 0.5) * 1e-5) / fs;
                it.code_slot = (int)(rnd() % 2);
                it.code_step = step;
                it.rem_code = uni() * step;
                it.n_samples = (int)std::ceil((1023.0 - it.rem_code) / step) + (int)(rnd() % 3) - 1;
                it.start_sample = (int64_t)(rnd() % ((1 << 20) - 60000));
                it.carrier_hz = (uni() - 0.5) * 1e4;
                it.rem_carrier = uni() * 6.28;
            }
            for (double scale = 1.0; scale <= 2.0; scale += 1.0) {
                const ItemRules r = item_rules(4, 1023 + 2 * SDR_LUT_PAD + 8, 1 << 20, spacing, 3, scale);
                int lut_words = 0, word = 0;
                CHECK(walk_of_old(items, r, code_len, spacing, plain, &lut_words, &word) == -1);
                const ItemStats whole = fold(items, 0, items.size(), r, code_len);
                // seven parts, merged in a scrambled order
                const size_t cut[8] = {0, 17, 700, 701, 2500, 3999, 4001, 5000};
                const int order[7] = {4, 0, 6, 2, 5, 1, 3};
                ItemStats merged = item_stats_initial(r.want_s12);
                for (int k : order) item_stats_merge(merged, fold(items, cut[k], cut[k + 1], r, code_len));
                CHECK(same(whole, merged) && whole.first_bad == kNoBadItem);
                const ListVerdict a = list_verdict(whole, r, spacing, plain), b = list_verdict(merged, r, spacing, plain);
                CHECK(a.first_bad == kNoBadItem && a.lut_words == lut_words && a.word == word);
                CHECK(b.first_bad == kNoBadItem && b.lut_words == lut_words && b.word == word);
                if (one_rate && scale == 1.0) CHECK(variant_chip_aligned(word) && lut_words > 1023);
                // two bad items planted: the lowest is the list's
                std::vector<sdr_epl_item> spoilt = items;
                spoilt[4000].code_slot = -1, spoilt[17].n_samples = 0;
                CHECK(walk_of_old(spoilt, r, code_len, spacing, plain, &lut_words, &word) == 17);
                const ItemStats bad_whole = fold(spoilt, 0, spoilt.size(), r, code_len);
                ItemStats bad_merged = item_stats_initial(r.want_s12);
                for (int k : order) item_stats_merge(bad_merged, fold(spoilt, cut[k], cut[k + 1], r, code_len));
                CHECK(bad_whole.first_bad == 17 && bad_whole.bad_code == ITEM_SAMPLES && bad_merged.first_bad == 17 && bad_merged.bad_code == ITEM_SAMPLES);
                CHECK(list_verdict(bad_whole, r, spacing, plain).first_bad == 17 && list_verdict(bad_merged, r, spacing, plain).first_bad == 17);
            }
        }
        // the neutral element merges to itself
        for (int want = 0; want < 2; ++want) {
            ItemStats s = item_stats_initial(want != 0);
            item_stats_merge(s, item_stats_initial(want != 0));
            CHECK(same(s, item_stats_initial(want != 0)) && s.first_bad == 0x7fffffff && s.maxlen == 0 && s.max_step_bits == 0ull &&
                  s.min_step_bits == ~0ull && s.m_lo == 0x7fffffff && s.m_hi == 0 && s.all_split == want);
        }
    }
    printf("ok %ld\n", checks);
    return 0;
}
