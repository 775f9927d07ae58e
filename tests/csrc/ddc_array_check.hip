// Host-side proof of the array arithmetic (sydr_amd/csrc/ddc_array.h), the code the converter's kernels decode and combine the
// elements of a frame with:
//  - the limits (ddc_array_lanes_valid, ddc_array_weights_valid): everything inside them accepted, everything outside refused;
//  - the K-element decode: for packed fields of 1, 2 and 4 bits in both bit orders, int8, int16 and float32 fields, strides up to
//    17 (frames that straddle bytes, frames wider than the 64-bit window), real and complex, with and without the swap, every
//    element of every frame < 48 against a reading written out here -- a packed stream taken apart BIT BY BIT -- and against
//    ddc_layout_load with that lane; the integer decode against the widened one;
//  - the combine: ddc_array_load against a restatement in plain doubles, every product and every sum stored to a volatile
//    double before it is used (no long double, nothing a compiler could contract), with weights that make a fused
//    multiply-add differ; and unit weights against the single element;
//  - the history: combined inputs stored and read back as they were;
//  - the covariance's slots: the upper triangle's real and imaginary parts fill distinct slots.
// Built with `hipcc --cuda-host-only`.
//   usage: ddc_array_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../sydr_amd/csrc/ddc_array.h"

using namespace sdr;

static uint64_t state = 20260020;
static uint64_t next_random() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

static int packed_field_bitwise(const std::vector<uint8_t>& bytes, int64_t f, int bits, bool msb_first, const int8_t* levels) {
    const int F = 8 / bits;
    const int64_t byte = f / F;
    const int p = (int)(f % F);
    const int low = bits * (msb_first ? F - 1 - p : p);
    int code = 0;
    for (int b = bits - 1; b >= 0; --b) {
        const int64_t n = byte * 8 + low + b;                      // (bit n of the stream)
        code = code * 2 + ((bytes[(size_t)(n / 8)] >> (n % 8)) & 1);
    }
    return levels[code];
}

// x = sum_a conj(w_a) s_a, every operation rounded to a double in memory before the next reads it.
static void combine_restated(int K, const double (*w)[2], const double* sr, const double* si, double* re, double* im) {
    volatile double r = 0.0, i = 0.0, p;
    for (int a = 0; a < K; ++a) {
        p = w[a][0] * sr[a];
        r = r + p;
        p = w[a][1] * si[a];
        r = r + p;
        p = w[a][0] * si[a];
        i = i + p;
        p = w[a][1] * sr[a];
        i = i - p;
    }
    *re = r, *im = i;
}

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }

int main() {
    long cases = 0;
    const int n_frames = 48;
    const int8_t tables[3][16] = {{1, -1}, {1, 3, -1, -3}, {0, 1, 2, 3, 4, 5, 6, 7, -8, -7, -6, -5, -4, -3, -2, -128}};
    const int strides[] = {2, 3, 4, 5, 8, 16, 17};
    long wide_frames = 0, windowed_frames = 0;
    for (int kind = kDdcFieldInt8; kind <= kDdcFieldPacked; ++kind)
        for (int bits_at = 0; bits_at < (kind == kDdcFieldPacked ? 3 : 1); ++bits_at)
            for (int msb = 0; msb <= (kind == kDdcFieldPacked ? 1 : 0); ++msb)
                for (int stride : strides)
                    for (int cplx = 0; cplx <= 1; ++cplx)
                        for (int swap = 0; swap <= cplx; ++swap) {
                            const int bits = kind == kDdcFieldPacked ? 1 << bits_at : 0;
                            const int flags = (cplx ? kDdcLayoutComplex : 0) | (swap ? kDdcLayoutSwapIq : 0) | (msb ? kDdcLayoutMsbFirst : 0);
                            const int width = cplx ? 2 : 1;
                            if (stride < 2 * width) continue;
                            const int8_t* levels = tables[bits_at];
                            const DdcLayout l = ddc_layout_make(kind, bits, stride, 0, flags, levels);
                            // the elements: as many as fit, 8 at most, from the top lane down in steps that leave gaps (out of order,
                            // not adjacent)
                            DdcArray arr;
                            memset(&arr, 0, sizeof(arr));
                            int K = 0;
                            for (int lane = stride - width; lane >= 0 && K < kDdcArrayMax; lane -= (K % 2 ? width + 1 : width)) arr.lanes[K++] = lane;
                            if (K < kDdcArrayMin) continue;
                            if (K >= 3) {
                                const int t = arr.lanes[0];
                                arr.lanes[0] = arr.lanes[2], arr.lanes[2] = t;
                            }
                            arr.K = K, arr.flags = 0;
                            if (!ddc_array_lanes_valid(l, K, 0, arr.lanes) || !ddc_array_lanes_valid(l, K, kDdcArrayMeasure, arr.lanes)) {
                                printf("valid array refused: kind=%d bits=%d stride=%d K=%d\n", kind, bits, stride, K);
                                return 1;
                            }
                            for (int a = 0; a < K; ++a) {
                                // weights whose products are inexact, so that a fused multiply-add would show
                                arr.w[a][0] = ((double)(int64_t)(next_random() % 2000001) - 1000000.0) / 3.0e5;
                                arr.w[a][1] = ((double)(int64_t)(next_random() % 2000001) - 1000000.0) / 7.0e5;
                            }
                            const int64_t n_fields = (int64_t)n_frames * stride;
                            const int field_bits = kind == kDdcFieldPacked ? bits : 8 * ddc_field_bytes(kind);
                            std::vector<uint8_t> bytes((size_t)((n_fields * field_bits + 7) / 8));
                            for (auto& b : bytes) b = (uint8_t)next_random();
                            std::vector<double> want((size_t)n_fields);
                            for (int64_t f = 0; f < n_fields; ++f) {
                                if (kind == kDdcFieldPacked) {
                                    want[(size_t)f] = packed_field_bitwise(bytes, f, bits, msb != 0, levels);
                                } else if (kind == kDdcFieldInt8) {
                                    int8_t v;
                                    memcpy(&v, &bytes[(size_t)f], 1);
                                    want[(size_t)f] = v;
                                } else if (kind == kDdcFieldInt16) {
                                    int16_t v;
                                    memcpy(&v, &bytes[(size_t)(2 * f)], 2);
                                    want[(size_t)f] = v;
                                } else {
                                    float v = (float)((int)(next_random() % 65536) - 32768) * 0.37f;
                                    memcpy(&bytes[(size_t)(4 * f)], &v, 4);
                                    want[(size_t)f] = v;
                                }
                            }
                            std::vector<double> hist(2 * (size_t)n_frames);
                            for (int64_t j = 0; j < n_frames; ++j) {
                                const DdcFrame fr = ddc_array_frame(bytes.data(), j, l);
                                if (kind == kDdcFieldPacked) (fr.whole ? windowed_frames : wide_frames)++;
                                else if (fr.whole) {
                                    printf("a frame of unpacked fields taken for a packed one\n");
                                    return 1;
                                }
                                double sr[kDdcArrayMax], si[kDdcArrayMax];
                                for (int a = 0; a < K; ++a) {
                                    const int lane = arr.lanes[a];
                                    const double x = want[(size_t)(j * stride + lane)], q = cplx ? want[(size_t)(j * stride + lane + 1)] : 0.0;
                                    const double want_re = swap ? q : x, want_im = cplx ? (swap ? x : q) : 0.0;
                                    double re = -1e300, im = -1e300, lr, li;
                                    ddc_array_element(bytes.data(), j, l, fr, lane, &re, &im);
                                    DdcLayout one = l;
                                    one.lane = lane;
                                    ddc_layout_load(bytes.data(), j, one, &lr, &li);
                                    if (!same(re, want_re) || !same(im, want_im) || !same(re, lr) || !same(im, li)) {
                                        printf("decode: kind=%d bits=%d msb=%d stride=%d lane=%d cplx=%d swap=%d j=%lld: (%g, %g), want (%g, %g), layout (%g, %g)\n",
                                               kind, bits, msb, stride, lane, cplx, swap, (long long)j, re, im, want_re, want_im, lr, li);
                                        return 1;
                                    }
                                    if (kind != kDdcFieldFloat32) {
                                        int ir = 1 << 30, ii = 1 << 30;
                                        ddc_array_element_int(bytes.data(), j, l, fr, lane, &ir, &ii);
                                        if ((double)ir != re || (double)ii != im) {
                                            printf("integer decode: kind=%d bits=%d stride=%d lane=%d j=%lld\n", kind, bits, stride, lane, (long long)j);
                                            return 1;
                                        }
                                    }
                                    sr[a] = re, si[a] = im;
                                    ++cases;
                                }
                                double re, im, wr, wi;
                                ddc_array_load(bytes.data(), j, l, arr, &re, &im);
                                combine_restated(K, arr.w, sr, si, &wr, &wi);
                                if (!same(re, wr) || !same(im, wi)) {
                                    printf("combine: kind=%d bits=%d stride=%d K=%d j=%lld: (%a, %a), want (%a, %a)\n", kind, bits, stride, K, (long long)j, re, im, wr, wi);
                                    return 1;
                                }
                                ddc_array_history_store(hist.data(), (int)j, re, im);
                                // unit weights: the element itself (a +0 where the element is zero)
                                DdcArray unit = arr;
                                const int pick = (int)(j % K);
                                for (int a = 0; a < K; ++a) unit.w[a][0] = a == pick ? 1.0 : 0.0, unit.w[a][1] = 0.0;
                                ddc_array_load(bytes.data(), j, l, unit, &re, &im);
                                if (re != sr[pick] || im != si[pick]) {
                                    printf("unit weight: kind=%d stride=%d K=%d j=%lld\n", kind, stride, K, (long long)j);
                                    return 1;
                                }
                                ++cases;
                            }
                            for (int64_t j = 0; j < n_frames; ++j) {
                                double re, im, hr, hi;
                                ddc_array_load(bytes.data(), j, l, arr, &re, &im);
                                ddc_array_history_load(hist.data(), j, &hr, &hi);
                                if (!same(re, hr) || !same(im, hi)) {
                                    printf("history: kind=%d stride=%d j=%lld\n", kind, stride, (long long)j);
                                    return 1;
                                }
                            }
                        }
    if (!wide_frames || !windowed_frames) {
        printf("the packed frames took one path only: %ld in a window, %ld field by field\n", windowed_frames, wide_frames);
        return 1;
    }
    // a contraction would show: with these numbers fma(w, s, r) differs from the rounded product added
    {
        const double w[2][2] = {{1.0, 0.0}, {1.0 + 0x1p-30, 0.0}}, sr[2] = {-1.0, 1.0 + 0x1p-30}, si[2] = {0.0, 0.0};
        double re = 0.0, im = 0.0;
        ddc_array_accumulate(w[0][0], w[0][1], sr[0], si[0], &re, &im);
        ddc_array_accumulate(w[1][0], w[1][1], sr[1], si[1], &re, &im);
        double wr, wi;
        combine_restated(2, w, sr, si, &wr, &wi);
        const double fused = std::fma(w[1][0], sr[1], std::fma(w[0][0], sr[0], 0.0));
        if (!same(re, wr) || !same(im, wi) || re == fused) {
            printf("contraction: %a against %a (fused %a)\n", re, wr, fused);
            return 1;
        }
        ++cases;
    }
    // the limits
    {
        const DdcLayout real4 = ddc_layout_make(kDdcFieldInt8, 0, 4, 0, 0, nullptr), cplx4 = ddc_layout_make(kDdcFieldInt8, 0, 4, 0, kDdcLayoutComplex, nullptr);
        struct Bad {
            const DdcLayout* l;
            int K, flags, lanes[9];
        };
        const Bad bad[] = {{&real4, 1, 0, {0}},          {&real4, 0, 0, {0}},          {&real4, -1, 0, {0}},        {&real4, 9, 0, {0, 1, 2, 3, 0, 1, 2, 3, 0}},
                           {&real4, 2, 0, {0, 0}},       {&real4, 3, 0, {1, 2, 1}},    {&real4, 2, 0, {0, 4}},      {&real4, 2, 0, {-1, 0}},
                           {&real4, 2, 2, {0, 1}},       {&real4, 2, -1, {0, 1}},      {&cplx4, 2, 0, {0, 3}},      {&cplx4, 2, 0, {3, 0}},
                           {&real4, 5, 0, {0, 1, 2, 3, 4}}};
        for (const Bad& c : bad) {
            if (ddc_array_lanes_valid(*c.l, c.K, c.flags, c.lanes)) {
                printf("bad array accepted: K=%d flags=%d lanes=%d,%d,%d\n", c.K, c.flags, c.lanes[0], c.lanes[1], c.lanes[2]);
                return 1;
            }
            ++cases;
        }
        const int ok_real[4] = {3, 0, 2, 1}, ok_cplx[2] = {2, 0};
        const DdcLayout wide = ddc_layout_make(kDdcFieldPacked, 4, 64, 0, kDdcLayoutComplex, tables[2]);
        const int ok_wide[8] = {62, 0, 7, 30, 2, 4, 50, 11};
        if (!ddc_array_lanes_valid(real4, 4, 0, ok_real) || !ddc_array_lanes_valid(cplx4, 2, 1, ok_cplx) || !ddc_array_lanes_valid(wide, 8, 1, ok_wide)) {
            printf("the ends of the domain refused\n");
            return 1;
        }
        double w[16];
        for (int k = 0; k < 16; ++k) w[k] = k - 7.5;
        if (!ddc_array_weights_valid(8, w)) {
            printf("finite weights refused\n");
            return 1;
        }
        const double nots[3] = {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity()};
        for (double v : nots)
            for (int k = 0; k < 16; ++k) {
                double c[16];
                memcpy(c, w, sizeof(c));
                c[k] = v;
                if (ddc_array_weights_valid(8, c) || (k >= 4 && !ddc_array_weights_valid(2, c))) {     // (only the first K are read)
                    printf("weight %d = %g\n", k, v);
                    return 1;
                }
                ++cases;
            }
    }
    // the covariance's slots
    {
        int seen[kDdcArrayCovSlots] = {0};
        for (int a = 0; a < kDdcArrayMax; ++a)
            for (int b = a; b < kDdcArrayMax; ++b) {
                ++seen[ddc_array_cov_re(a, b)];
                if (b > a) ++seen[ddc_array_cov_im(a, b)];
            }
        for (int s = 0; s < kDdcArrayCovSlots; ++s)
            if (seen[s] != 1) {
                printf("covariance slot %d used %d times\n", s, seen[s]);
                return 1;
            }
        ++cases;
    }
    // large indices: the frame's bit and byte are 64-bit
    {
        const DdcLayout l = ddc_layout_make(kDdcFieldPacked, 2, 6, 0, 0, tables[1]);
        std::vector<uint8_t> none(16, 0xe4);
        const DdcFrame fr = ddc_array_frame(none.data(), 5, l);     // bits 60 .. 71: bytes 7 and 8
        if (!fr.whole || fr.byte0 != 7 || fr.bits != 0xe4e4u) {
            printf("frame window: byte0=%lld bits=%llx\n", (long long)fr.byte0, (unsigned long long)fr.bits);
            return 1;
        }
        ++cases;
    }
    printf("ok %ld\n", cases);
    return 0;
}
