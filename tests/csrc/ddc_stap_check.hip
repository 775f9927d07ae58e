// Host-side proof of the space-time arithmetic (sydr_amd/csrc/ddc_stap.h), the code the converter's kernels combine T frames of K
// elements with and carry the raw tail by:
//  - the limits (ddc_stap_taps_valid, ddc_stap_weights_valid) and ddc_stap_set's layout [T][K][2] -> [8][8][2], zero outside;
//  - the combine: a stream cut into pushes -- a first push of one frame group, pushes shorter than T - 1 frames, long ones --
//    with ddc_stap_load of every input of every push against a restatement over the WHOLE stream in plain doubles, every product
//    and every sum stored to a volatile double before it is used (nothing a compiler could contract), frames before the
//    stream's first being zero, with weights that make a fused multiply-add differ; bit for bit;
//  - the raw tail: after every push, made by ddc_stap_tail_next as the history kernel makes it (every slot read before any is
//    written), slot i holds the elements of frame n - (T - 1) + i of the stream, zero before its first -- shifted, not
//    overwritten, by a short push;
//  - ddc_stap_lane against the index it replaces, the covariance's slots distinct and inside their lag.
// Fields: int8, int16, float32 and packed fields of 1, 2 and 4 bits in both bit orders; packed frames of 6, 12 and 20 bits, which
// are not whole bytes (pushes are then whole groups of frames), and of 68 bits, wider than the 64-bit window.
// Built with `hipcc --cuda-host-only`.
//   usage: ddc_stap_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../sydr_amd/csrc/ddc_stap.h"

using namespace sdr;

static uint64_t state = 20260021;
static uint64_t next_random() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

static bool same(double a, double b) { return memcmp(&a, &b, 8) == 0; }

static int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

// x_j over the whole stream's elements sr, si [n][K] (frames before 0 are zero), every operation rounded to a double in memory.
static void combine_restated(int T, int K, const double* w /*[T][K][2]*/, const std::vector<double>& sr, const std::vector<double>& si, int64_t j,
                             double* re, double* im) {
    volatile double r = 0.0, i = 0.0, p;
    for (int t = 0; t < T; ++t)
        for (int a = 0; a < K; ++a) {
            const double xr = j - t >= 0 ? sr[(size_t)((j - t) * K + a)] : 0.0, xi = j - t >= 0 ? si[(size_t)((j - t) * K + a)] : 0.0;
            const double wr = w[2 * (t * K + a)], wi = w[2 * (t * K + a) + 1];
            p = wr * xr;
            r = r + p;
            p = wi * xi;
            r = r + p;
            p = wr * xi;
            i = i + p;
            p = wi * xr;
            i = i - p;
        }
    *re = r, *im = i;
}

int main() {
    long cases = 0;
    // the limits
    for (int T = -1; T <= 10; ++T, ++cases)
        if (ddc_stap_taps_valid(T) != (T >= 1 && T <= 8)) {
            printf("taps %d\n", T);
            return 1;
        }
    {
        double w[2 * 8 * 8];
        for (int i = 0; i < 128; ++i) w[i] = 0.25 * i - 3.0;
        if (!ddc_stap_weights_valid(8, 8, w)) return printf("finite weights refused\n"), 1;
        const double bad[] = {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()};
        for (int T = 1; T <= 8; ++T)
            for (int K = 2; K <= 8; ++K)
                for (int at = 0; at < 2 * T * K; ++at, ++cases) {
                    const double keep = w[at];
                    w[at] = bad[at % 3];
                    if (ddc_stap_weights_valid(T, K, w)) return printf("weight %d of T=%d K=%d accepted\n", at, T, K), 1;
                    w[at] = keep;
                }
        for (int T = 1; T <= 8; ++T)
            for (int K = 2; K <= 8; ++K) {
                DdcStap s;
                memset(&s, 0xff, sizeof(s));
                ddc_stap_set(&s, T, K, w);
                if (s.T != T) return printf("set T\n"), 1;
                for (int t = 0; t < 8; ++t)
                    for (int a = 0; a < 8; ++a)
                        for (int c = 0; c < 2; ++c, ++cases) {
                            const double want = t < T && a < K ? w[2 * (t * K + a) + c] : 0.0;
                            if (!same(s.w[t][a][c], want)) return printf("set T=%d K=%d t=%d a=%d\n", T, K, t, a), 1;
                        }
            }
    }
    // the covariance's slots
    {
        bool seen[kDdcStapCovSlots] = {};
        for (int a = 0; a < 8; ++a)
            for (int b = 0; b < 8; ++b, ++cases)
                for (int c = 0; c < 2; ++c) {
                    const int s = ddc_stap_cov_slot(a, b) + c;
                    if (s < 0 || s >= kDdcStapCovSlots || seen[s]) return printf("slot %d %d\n", a, b), 1;
                    seen[s] = true;
                }
    }
    const int8_t tables[3][16] = {{1, -1}, {1, 3, -1, -3}, {0, 1, 2, 3, 4, 5, 6, 7, -8, -7, -6, -5, -4, -3, -2, -128}};
    struct Shape {
        int kind, bits_at, stride, cplx;
    };
    const Shape shapes[] = {{kDdcFieldInt8, 0, 4, 0},    {kDdcFieldInt8, 0, 17, 1},  {kDdcFieldInt16, 0, 7, 1}, {kDdcFieldFloat32, 0, 5, 1},
                            {kDdcFieldPacked, 0, 6, 1},  {kDdcFieldPacked, 1, 6, 1}, {kDdcFieldPacked, 1, 3, 0}, {kDdcFieldPacked, 2, 5, 1},
                            {kDdcFieldPacked, 2, 17, 1}, {kDdcFieldPacked, 1, 8, 1}};
    const int n_frames = 96;
    long short_pushes = 0, odd_frames = 0;
    for (const Shape& sh : shapes)
        for (int msb = 0; msb <= (sh.kind == kDdcFieldPacked ? 1 : 0); ++msb)
            for (int swap = 0; swap <= sh.cplx; ++swap)
                for (int T = 1; T <= kDdcStapMaxTaps; ++T) {
                    const int bits = sh.kind == kDdcFieldPacked ? 1 << sh.bits_at : 0;
                    const int flags = (sh.cplx ? kDdcLayoutComplex : 0) | (swap ? kDdcLayoutSwapIq : 0) | (msb ? kDdcLayoutMsbFirst : 0);
                    const int width = sh.cplx ? 2 : 1;
                    const DdcLayout l = ddc_layout_make(sh.kind, bits, sh.stride, 0, flags, tables[sh.bits_at]);
                    DdcArray arr;
                    memset(&arr, 0, sizeof(arr));
                    int K = 0;
                    for (int lane = sh.stride - width; lane >= 0 && K < kDdcArrayMax; lane -= (K % 2 ? width + 1 : width)) arr.lanes[K++] = lane;
                    if (K < kDdcArrayMin || !ddc_array_lanes_valid(l, K, 0, arr.lanes)) return printf("array of stride %d\n", sh.stride), 1;
                    arr.K = K;
                    for (int a = 0; a < kDdcArrayMax; ++a, ++cases)
                        if (ddc_stap_lane(arr, a) != arr.lanes[a]) return printf("lane %d\n", a), 1;
                    std::vector<double> w((size_t)(2 * T * K));
                    for (size_t i = 0; i < w.size(); ++i) w[i] = ((double)(int64_t)(next_random() % 2000001) - 1000000.0) / (i % 2 ? 7.0e5 : 3.0e5);
                    DdcStap st;
                    ddc_stap_set(&st, T, K, w.data());
                    const int field_bits = sh.kind == kDdcFieldPacked ? bits : 8 * ddc_field_bytes(sh.kind);
                    const int frame_bits = sh.stride * field_bits;
                    const int group = 8 / gcd(frame_bits, 8);                   // frames of a whole number of bytes
                    if (frame_bits % 8) ++odd_frames;
                    std::vector<uint8_t> bytes((size_t)((int64_t)n_frames * frame_bits / 8));
                    for (auto& b : bytes) b = (uint8_t)next_random();
                    if (sh.kind == kDdcFieldFloat32)
                        for (size_t f = 0; f < bytes.size() / 4; ++f) {
                            const float v = (float)((double)(int64_t)(next_random() % 200001) - 100000.0) / 64.0f;
                            memcpy(&bytes[4 * f], &v, 4);
                        }
                    // the whole stream's elements, by the array's own decode (ddc_array_check proves it)
                    std::vector<double> sr((size_t)n_frames * K), si((size_t)n_frames * K);
                    for (int64_t j = 0; j < n_frames; ++j) {
                        const DdcFrame fr = ddc_array_frame(bytes.data(), j, l);
                        for (int a = 0; a < K; ++a) ddc_array_element(bytes.data(), j, l, fr, arr.lanes[a], &sr[(size_t)(j * K + a)], &si[(size_t)(j * K + a)]);
                    }
                    // the cut: one group, then pushes shorter than T - 1 where the group allows, a long one, short ones again, the rest
                    std::vector<int> cut = {group, group, 2 * group, 40 / group * group, group, group, 3 * group};
                    std::vector<double> tail(ddc_stap_tail_bytes(T, K) / sizeof(double), 0.0), next(tail.size());
                    int64_t seen = 0;
                    for (size_t c = 0; seen < n_frames; ++c) {
                        int64_t n_in = c < cut.size() ? cut[c] : n_frames - seen;
                        if (n_in > n_frames - seen) n_in = n_frames - seen;
                        if (n_in < T - 1 && seen > 0) ++short_pushes;
                        const uint8_t* p = bytes.data() + seen * frame_bits / 8;
                        for (int64_t j = 0; j < n_in; ++j, ++cases) {
                            double re, im, wr, wi;
                            ddc_stap_load(p, tail.data(), j, l, arr, st, &re, &im);
                            combine_restated(T, K, w.data(), sr, si, seen + j, &wr, &wi);
                            if (!same(re, wr) || !same(im, wi))
                                return printf("combine: kind=%d bits=%d stride=%d T=%d K=%d input %lld: %a %a, want %a %a\n", sh.kind, bits, sh.stride, T, K,
                                              (long long)(seen + j), re, im, wr, wi), 1;
                        }
                        for (int i = 0; i < T - 1; ++i)
                            for (int a = 0; a < K; ++a)
                                ddc_stap_tail_next(p, tail.data(), n_in, l, arr, T, i, a, &next[(size_t)(2 * (i * K + a))], &next[(size_t)(2 * (i * K + a) + 1)]);
                        for (int i = 0; i < T - 1; ++i)
                            for (int a = 0; a < K; ++a) ddc_stap_tail_store(tail.data(), i, K, a, next[(size_t)(2 * (i * K + a))], next[(size_t)(2 * (i * K + a) + 1)]);
                        seen += n_in;
                        for (int i = 0; i < T - 1; ++i)
                            for (int a = 0; a < K; ++a, ++cases) {
                                const int64_t f = seen - (T - 1) + i;
                                const double wr = f >= 0 ? sr[(size_t)(f * K + a)] : 0.0, wi = f >= 0 ? si[(size_t)(f * K + a)] : 0.0;
                                double re, im;
                                ddc_stap_tail_load(tail.data(), i, K, a, &re, &im);
                                if (!same(re, wr) || !same(im, wi))
                                    return printf("tail: kind=%d stride=%d T=%d after %lld frames slot %d element %d\n", sh.kind, sh.stride, T, (long long)seen, i, a), 1;
                            }
                    }
                }
    if (short_pushes < 100 || odd_frames < 50) return printf("the cases miss short pushes (%ld) or odd frames (%ld)\n", short_pushes, odd_frames), 1;
    printf("ok %ld\n", cases);
    return 0;
}
