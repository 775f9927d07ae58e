// The variant word of an E/P/L plan (sdr_epl_plan_variant) -- how a list's statistics become one (choose_variant), what a
// word means (decode: the ONLY reader of its bits), and the lists of the compiled forms a word can name: the straight-line
// kernels of epl.hip and epl_straight.hip, the several-chips-per-lane shapes.  Host arithmetic only, no kernel in sight:
// tests/csrc/epl_variant_dump.hip compiles it alone (tests/test_epl_variant.py, `make check-sanitize`).  The other decisions of
// a plan's creation (epl_plan.hip) -- the fold of a list's statistics that feeds choose_variant among them -- are epl_plan.h's.
#pragma once

#include "../../include/sydr_amd.h"

// word = low byte + 256 * KS + kVariantKI + kVariantC2 * shape:
//   low byte  samples a lane owns: 0 (per sample), 8 / 16 (boundary variants), kVariantChip (chip-aligned: a lane owns a
//             chip) + the block length KM compiled in, or + kVariantKM1516
//   KS        three taps, the outer ones switching KS.x samples into the anchor's block (12 at 24 / 25 samples per chip, 9 at 19 / 20)
constexpr int kVariantChip = 26;         // = sdr::kChipMax (epl_kernel.h asserts it)
constexpr int kVariantKSMask = 256 * 15;
constexpr int kVariantKM1516 = 16;       // (added to kVariantChip) 15.x or 16.x samples per chip by the epoch: both block lengths compiled in
constexpr int kVariantKI = 4096;         // taps whole (half-)chips apart: no switch inside a block
constexpr int kVariantC2 = 8192;         // x shape (1 .. 3): several chips per lane (correlator_chip2.h), SDR_EPL_CHIPN_SHAPES below
// the limits of the correlator cores (correlator.h, correlator_chip.h: epl_kernel.h asserts that they are theirs)
constexpr double kVariantFastMaxStep = 0.06, kVariantFastMaxStep8 = 0.125, kVariantFastMinStep = 1e-4;
constexpr int kVariantFastMaxLutWords = 1 << 18;
constexpr double kVariantChipMinStep = 1.0 / 25.9, kVariantChipMaxStep = 1.0 / 15.5;
constexpr int kLongLutWords = 4096;  // replicas of 16 KB and more (multi-period / BOC half-chip codes): four epochs share a staged copy (decode's wpw = 4)

// ---- the compiled forms.  X(NT, KM, KS, KI): epl_kernel<ci8, NT, kChipMax, KM, 1, KS, KI>, one wave per workgroup, and --
// where KS or KI is set -- chip_setup<NT, KM, KS, KI> for the plan's ChipSetup<NT> per item.  Each unit instantiates its own
// list (the split is for compile time); a word that decodes to a tuple in neither has no kernel.
// epl.hip: the headline geometries
#define SDR_EPL_ROWS_HEADLINE(X) X(3, 24, 12, 0) X(3, 19, 9, 0) X(3, 24, 0, 1) X(5, 24, 0, 1) X(3, 15, 0, 1)
// epl_straight.hip: the other block lengths -- KS = KM / 2 (taps half a chip apart), KI with three and with five taps, and
// the block length alone (three taps at any spacing, positions at run time, no setups)
#define SDR_EPL_ROWS_STRAIGHT(X)                                                                                                     \
    X(3, 16, 8, 0) X(3, 17, 8, 0) X(3, 18, 9, 0) X(3, 20, 10, 0) X(3, 21, 10, 0) X(3, 22, 11, 0) X(3, 23, 11, 0) X(3, 25, 12, 0)     \
    X(3, 16, 0, 1) X(3, 17, 0, 1) X(3, 18, 0, 1) X(3, 19, 0, 1) X(3, 20, 0, 1) X(3, 21, 0, 1) X(3, 22, 0, 1) X(3, 23, 0, 1) X(3, 25, 0, 1) \
    X(5, 16, 0, 1) X(5, 17, 0, 1) X(5, 18, 0, 1) X(5, 19, 0, 1) X(5, 20, 0, 1) X(5, 21, 0, 1) X(5, 22, 0, 1) X(5, 23, 0, 1) X(5, 25, 0, 1) \
    X(3, 17, 0, 0) X(3, 18, 0, 0) X(3, 19, 0, 0) X(3, 20, 0, 0) X(3, 21, 0, 0) X(3, 22, 0, 0) X(3, 23, 0, 0) X(3, 25, 0, 0)
// X(shape, boundaries...): epl2_kernel<boundaries...> with a ChipNSetup<boundaries...> per item (three taps, ci8)
#define SDR_EPL_CHIPN_SHAPES(X) X(1, 4, 9, 14, 19) X(2, 5, 11, 17, 23) X(3, 1, 3, 5, 7, 9, 11, 13, 15)

// ---- what a list gets
struct VariantInputs {
    int n_taps;                    // of the list; ItemRules::scale (2: the half-chip view) and ::s_anchor
    double scale, s_anchor;
    const double* spacing;         // [n_taps], unscaled
    double max_step, min_step;     // the list's statistics: range of scale * code_step,
    int m_lo, m_hi;                // ... of whole samples per chip,
    bool all_split;                // ... ItemStats::all_split
    int iq_fmt, lut_stride;        // the engine's ring format, row length of its replica tables,
    bool no_chip, no_split;        // ... "epl_no_chip", "epl_no_split"
};

inline int choose_variant(const VariantInputs& v) {
    bool all_ki = v.n_taps == 3 || v.n_taps == 5;   // tap t exactly (t - A) chips from the anchor (KI kernel)
    for (int t = 0; all_ki && t < v.n_taps; ++t) all_ki = v.scale * v.spacing[t] - v.s_anchor == (double)(t - v.n_taps / 2);
    const int m_lo = v.m_lo, m_hi = v.m_hi;
    const bool all_m24 = m_lo == 24 && m_hi == 24;
    const bool all_m15 = m_lo == 15 && m_hi == 15;                      // (31-32.7 MHz on the half-chip view: KM = 15, whole-chip taps)
    const bool all_m1516 = m_lo >= 15 && m_hi <= 16 && v.n_taps == 3 && v.scale == 1.0;   // (16.368 MHz: 16.0 -- 15.x or 16.x by the Doppler's sign)
    // one block length KM throughout, three taps: the straight-line kernels exist for KM = 16 .. 25 -- with the outer taps'
    // switch position floor(KM / 2) compiled in (+-0.5 chip, `all_split`) or with taps whole (half-)chips apart (`all_ki`)
    const int km_one = m_lo == m_hi && m_lo >= 16 && m_lo <= 25 && v.n_taps == 3 ? m_lo : 0;
    const bool boundary_ok = v.min_step >= kVariantFastMinStep && v.scale * v.lut_stride < kVariantFastMaxLutWords;
    int wide = !boundary_ok ? 0 : (v.max_step <= kVariantFastMaxStep ? 16 : (v.max_step <= kVariantFastMaxStep8 ? 8 : 0));
    // every item inside the chip-aligned variant's range (ci8 ring): lanes own whole chips instead of 16 samples
    // (the half-chip view only where a half chip holds 16 samples or more: at 31-32 MHz -- 15.6 per half chip -- the
    // 16-sample boundary groups of the plain list were measured faster, 0.47 against 0.37 of the roof)
    // ... unless every half chip holds 15.x samples and the taps sit whole half-chips apart: the KM = 15 whole-chip-tap kernel
    const double chip_max_step = v.scale == 2.0 && !(all_m15 && all_ki && v.n_taps == 3 && !v.no_split) ? 1.0 / 16.0 : kVariantChipMaxStep;
    if (boundary_ok && v.iq_fmt == SDR_FMT_CI8 && v.min_step >= kVariantChipMinStep && v.max_step <= chip_max_step && !v.no_chip) {
        wide = kVariantChip;
        const int km5 = m_lo == m_hi && m_lo >= 16 && m_lo <= 25 && v.n_taps == 5 ? m_lo : 0;
        if (km5 && all_ki && !v.no_split)                   // five taps whole (half-)chips apart
            wide += km5 + kVariantKI;
        else if (all_m24 && v.n_taps != 3)                  // (other tap counts: the 24 / 25 form with run-time positions alone)
            wide += 24;
        else if (km_one && v.all_split && !v.no_split)
            wide += km_one + 256 * (km_one / 2);
        else if (km_one && all_ki && !v.no_split)
            wide += km_one + kVariantKI;
        else if (all_m24 || (km_one >= 17 && !v.no_split))  // block length compiled in, tap positions at run time
            wide += all_m24 ? 24 : km_one;
        else if (all_m15 && all_ki && v.n_taps == 3 && v.scale == 2.0 && !v.no_split)
            wide += 15 + kVariantKI;
        else if (all_m1516 && !v.no_split)
            wide += kVariantKM1516;
    }
    return wide;
}

inline int variant_with_shape(int word, int shape) { return word + kVariantC2 * shape; }

// ---- what a word launches for one chunk of `nt` taps (1, 2, 3 or 5) of a ring of format `fmt`
struct EplForm {
    int shape;                             // 1 .. 3: that row of SDR_EPL_CHIPN_SHAPES (its own kernel; nothing below applies)
    int fmt, nt, w, km, wpw, ks, ki, km2;  // 0: epl_kernel<fmt, nt, w, km, wpw, ks, ki, km2>
    bool row;                              // ... which is a row of SDR_EPL_ROWS_* (else one of the general forms of epl.hip's launch_one)
    bool setups;                           // the plan holds a ChipSetup<nt> (shape: a ChipNSetup) per item
};

// wpw: waves per workgroup, 4 for long replicas.  has_setups: the plan holds its per-item setups -- the kernels that read
// them are not chosen without (plan creation asks with `true`: whether it has to make them).
inline EplForm decode(int word, int fmt, int nt, int wpw, bool has_setups) {
    EplForm f = {};
    f.fmt = fmt, f.nt = nt, f.wpw = wpw;
    const bool ci8 = fmt == SDR_FMT_CI8;
    const int low = word & 255;
    if (ci8 && has_setups && ((word / kVariantC2) & 3)) {
        f.shape = (word / kVariantC2) & 3;
        f.setups = true;
        return f;
    }
    if (!(ci8 && low >= kVariantChip)) {
        f.w = low == 16 || low == 8 ? low : 0;
        return f;
    }
    f.w = kVariantChip;
    const int km = low - kVariantChip;
    // (the compile-time tap geometries exist for one chunk of three or of five taps)
    const int ks = nt == 3 && has_setups ? (word & kVariantKSMask) / 256 : 0;
    const int ki = (word & kVariantKI) && (nt == 3 || nt == 5) && has_setups ? 1 : 0;
    f.setups = ks || ki;
    if (wpw == 4) {                   // four epochs of a channel around one staged table: the 24 / 25 forms or none
        f.km = km == 24 ? 24 : 0;
        f.ki = km == 24 ? ki : 0;
    } else if (ks || ki) {
        f.km = km, f.ks = ks, f.ki = ks ? 0 : ki, f.row = true;
    } else if (km == 24) {            // block length compiled in, tap positions at run time
        f.km = 24;
    } else if (nt == 3 && km >= 17) { // ... the same for the other lengths
        f.km = km, f.row = true;
    } else if (nt == 3 && km == kVariantKM1516) {
        f.km = 15, f.km2 = 16;
    }
    return f;
}

// (a list's word as choose_variant made it) the chip-aligned cores serve the list
inline bool variant_chip_aligned(int word) { return decode(word, SDR_FMT_CI8, 1, 1, false).w == kVariantChip; }
