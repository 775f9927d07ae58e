// Host build of the E/P/L plans' variant arithmetic (sydr_amd/csrc/epl_variant.h), as text on stdout:
//   grid    choose_variant over a grid of list statistics, engine settings and spacings, in a fixed order, run-length coded:
//           one line "count word" per run of equal words (tests/golden/epl_variant_grid.txt holds what the code chose
//           before the table existed)
//   decode  for every distinct (format, n_taps, word) of the grid: decode() of every chunk of taps, with one and with four
//           waves per workgroup, with and without setups
//   rows    the lists of compiled forms: "row unit NT KM KS KI" and "shape index boundaries"
// Test infrastructure (tests/test_epl_variant.py).
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>

#include "../../sydr_amd/csrc/epl_variant.h"

namespace {

const double kSpacings[5][5] = {{-0.5, 0, 0.5, 1.0, 1.5}, {-1, 0, 1, 2, 3}, {-0.25, 0, 0.25, 0.5, 0.75}, {-1, -0.5, 0, 0.5, 1}, {-2, -1, 0, 1, 2}};

struct StepRange { double min_step, max_step; int m_lo, m_hi; };

// 14 .. 27 whole samples per chip, one length or two neighbours; then three ranges outside the chip-aligned cores', one for
// each width of the others (16, 8, per sample), and the two lengths whose whole range of steps is not inside the cores':
// 15.6 .. 15.9 and 25.1 .. 25.8 samples per chip (theirs: 15.5 .. 25.9)
int step_ranges(StepRange* out) {
    int n = 0;
    for (int m_lo = 14; m_lo <= 27; ++m_lo)
        for (int d = 0; d < 2; ++d) out[n++] = StepRange{1.0 / (m_lo + d + 1), 1.0 / m_lo, m_lo, m_lo + d};
    out[n++] = StepRange{1.0 / 40, 1.0 / 30, 30, 39};
    out[n++] = StepRange{0.1, 0.12, 8, 9};
    out[n++] = StepRange{0.2, 0.25, 4, 4};
    out[n++] = StepRange{1.0 / 15.9, 1.0 / 15.6, 15, 15};
    out[n++] = StepRange{1.0 / 25.8, 1.0 / 25.1, 25, 25};
    return n;
}

template <class F>
void grid(F&& point) {
    StepRange ranges[40];
    const int n_ranges = step_ranges(ranges);
    const int taps[6] = {1, 2, 3, 4, 5, 8};
    const int fmts[2] = {SDR_FMT_CI8, SDR_FMT_CI16};
    const int strides[2] = {1023 + 10, kVariantFastMaxLutWords / 2};
    for (int fmt : fmts)
        for (int stride : strides)
            for (int no_chip = 0; no_chip < 2; ++no_chip)
                for (int r = 0; r < n_ranges; ++r)
                    // (thinned: the long rows with the half-chip view alone, where their doubled length is over the limit)
                    for (int scale = stride == strides[0] ? 1 : 2; scale <= 2; ++scale)
                        for (int n_taps : taps)
                            for (int no_split = 0; no_split < 2; ++no_split)
                                for (int s = 0; s < 5; ++s)
                                    for (int all_split = 0; all_split < 2; ++all_split) {
                                        double sp[8];   // the five taps of the row, continued with its last difference
                                        for (int t = 0; t < 8; ++t) sp[t] = t < 5 ? kSpacings[s][t] : sp[t - 1] + (kSpacings[s][4] - kSpacings[s][3]);
                                        VariantInputs v = {};
                                        v.n_taps = n_taps, v.scale = scale, v.spacing = sp;
                                        v.s_anchor = scale * sp[n_taps < 5 ? n_taps / 2 : 2];      // (epl_plan.h: item_rules)
                                        v.max_step = ranges[r].max_step, v.min_step = ranges[r].min_step;
                                        v.m_lo = ranges[r].m_lo, v.m_hi = ranges[r].m_hi, v.all_split = all_split != 0;
                                        v.iq_fmt = fmt, v.lut_stride = stride, v.no_chip = no_chip != 0, v.no_split = no_split != 0;
                                        point(v, choose_variant(v));
                                    }
}

void print_form(int word, int fmt, int n_taps, int nt, int wpw, int has) {
    const EplForm f = decode(word, fmt, nt, wpw, has != 0);
    printf("%d %d %d %d %d %d : %d %d %d %d %d %d %d %d %d %d %d\n", fmt, n_taps, word, nt, wpw, has, f.shape, f.fmt, f.nt, f.w, f.km, f.wpw,
           f.ks, f.ki, f.km2, f.row ? 1 : 0, f.setups ? 1 : 0);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "grid")) {
        long run = 0;
        int last = -1;
        grid([&](const VariantInputs&, int word) {
            if (word != last && run) printf("%ld %d\n", run, last), run = 0;
            last = word, ++run;
        });
        printf("%ld %d\n", run, last);
    } else if (!strcmp(argv[1], "decode")) {
        std::set<std::tuple<int, int, int>> seen;
        grid([&](const VariantInputs& v, int word) { seen.insert(std::make_tuple(v.iq_fmt, v.n_taps, word)); });
        for (const auto& k : seen) {
            const int fmt = std::get<0>(k), n_taps = std::get<1>(k), word = std::get<2>(k);
            for (int t0 = 0; t0 < n_taps;) {   // (taps are served in chunks of 5 / 3 / 2 / 1)
                const int left = n_taps - t0, nt = left >= 5 ? 5 : (left >= 3 ? 3 : left);
                for (int wpw = 1; wpw <= 4; wpw += 3)
                    for (int has = 0; has < 2; ++has) print_form(word, fmt, n_taps, nt, wpw, has);
                t0 += nt;
            }
            // a list of three taps that went per sample or to the 8-sample boundary variant may get a several-chip shape
            if (fmt == SDR_FMT_CI8 && n_taps == 3 && (word == 0 || word == 8))
                for (int shape = 1; shape <= 3; ++shape)
                    for (int has = 0; has < 2; ++has) print_form(variant_with_shape(word, shape), fmt, n_taps, 3, 1, has);
        }
    } else if (!strcmp(argv[1], "rows")) {
#define SDR_ROW(NT, KM, KS, KI) printf("row %s %d %d %d %d\n", unit, NT, KM, KS, KI);
        const char* unit = "epl";
        SDR_EPL_ROWS_HEADLINE(SDR_ROW)
        unit = "epl_straight";
        SDR_EPL_ROWS_STRAIGHT(SDR_ROW)
#undef SDR_ROW
#define SDR_SHAPE(S, ...) printf("shape %d %s\n", S, #__VA_ARGS__);
        SDR_EPL_CHIPN_SHAPES(SDR_SHAPE)
#undef SDR_SHAPE
    } else {
        return 2;
    }
    return 0;
}
