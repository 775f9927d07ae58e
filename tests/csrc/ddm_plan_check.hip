// Host-side proof of the arithmetic sdr_ddm shares between its checks and its kernels (sydr_amd/csrc/ddm_plan.h), built with
// `hipcc --cuda-host-only` under the address and undefined-behaviour sanitizers (`make check-sanitize`):
//  - the segments of a window tile it exactly: a_0 = 0, b_{Q-1} = W, b_q = a_{q+1}, none empty while Q <= W, lengths that
//    differ by at most one -- for small windows by brute force and for windows up to 2^31 - 1 with Q up to 4096;
//  - rem_carrier_q lies in [0, 2*pi) (2*pi itself only where Python's own % rounds up to it) and equals the plain
//    expression; rem_code_q and tau_q equal theirs; hostile values (NaN, Inf, huge) go through without a trap;
//  - ddm_bins against the formula and for bad grids; d_k is symmetric around (K-1)/2;
//  - the launch geometry: every tap belongs to exactly one (chunk, group), a group's lanes lie inside the workgroup,
//    the lanes of a tap cut any tile into adjoining pieces that cover it, and the chunks are as few as fill the device.
//   usage: ddm_plan_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../include/sydr_amd.h"
#include "../../sydr_amd/csrc/ddm_plan.h"

using namespace sdr;

static uint64_t state = 20260019;
static uint64_t next() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 11;
}

static int check_segments(int64_t W, int Q) {
    int64_t prev_b = 0, shortest = W, longest = 0;
    for (int q = 0; q < Q; ++q) {
        int64_t a, b;
        ddm_segment_bounds(W, Q, q, &a, &b);
        if (a != prev_b || b < a || b > W) return printf("segments W %lld Q %d q %d: [%lld, %lld)\n", (long long)W, Q, q, (long long)a, (long long)b), 1;
        if (Q <= W && b == a) return printf("empty segment W %lld Q %d q %d\n", (long long)W, Q, q), 1;
        shortest = b - a < shortest ? b - a : shortest;
        longest = b - a > longest ? b - a : longest;
        prev_b = b;
    }
    if (prev_b != W || longest - shortest > 1) return printf("segments W %lld Q %d: end %lld, lengths %lld..%lld\n", (long long)W, Q, (long long)prev_b, (long long)shortest, (long long)longest), 1;
    return 0;
}

int main() {
    long cases = 0;
    // ---- segments
    for (int64_t W = 1; W <= 300; ++W)
        for (int Q = 1; Q <= 300 && Q <= kDdmMaxAll; ++Q, ++cases)
            if (Q <= W && check_segments(W, Q)) return 1;
    for (int round = 0; round < 2000; ++round, ++cases) {
        const int Q = 1 + (int)(next() % kDdmMaxAll);
        int64_t W = round % 3 == 0 ? 2147483647 - (int64_t)(next() % 5000) : Q + (int64_t)(next() % 100000000);
        if (check_segments(W, Q)) return 1;
    }
    // ---- the NCO state of a segment
    const double two_pi = 2.0 * M_PI, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (int round = 0; round < 200000; ++round, ++cases) {
        const double f0 = ((double)(next() % 20000001) - 1e7) * (round % 7 == 0 ? 1e-3 : 1.0);
        const double rem = round % 5 == 0 ? -(double)(next() % 1000) * 0.37 : (double)(next() % 6283) * 1e-3;
        const int64_t a = (int64_t)(next() % 2147483647);
        const double fs = 1e6 + (double)(next() % 49000000);
        const double r = ddm_rem_carrier(f0, rem, a, fs);
        double x = rem + (-((((f0 * 2.0) * M_PI) * (double)a) / fs));
        double want = std::fmod(x, two_pi);
        if (want < 0.0) want += two_pi;
        if (!(r >= 0.0) || !(r <= two_pi) || r != want || std::signbit(r)) return printf("rem_carrier %a %a %lld %a -> %a (want %a)\n", f0, rem, (long long)a, fs, r, want), 1;
        const double step = 1.023e6 / fs, rc = -500.0 + (double)(next() % 100000) * 0.01;
        if (ddm_rem_code(rc, a, step) != rc + (double)a * step) return printf("rem_code\n"), 1;
        const int64_t b = a + 1 + (int64_t)(next() % 100000);
        if (ddm_tau(a, b, fs) != (double)(a + b - 1) / 2.0 / fs) return printf("tau\n"), 1;
    }
    if (ddm_rem_carrier(0.0, -0.0, 0, 4e6) != 0.0 || std::signbit(ddm_rem_carrier(0.0, -0.0, 0, 4e6))) return printf("rem_carrier of -0.0\n"), 1;
    {   // hostile values: no trap, no value outside [0, 2*pi] but NaN
        const double bad[] = {nan, inf, -inf, 1e308, -1e308, 5e-324, 0.0};
        for (double f0 : bad)
            for (double rem : bad)
                for (double fs : bad) {
                    const double r = ddm_rem_carrier(f0, rem, 123456789, fs);
                    if (!(r != r) && !(r >= 0.0 && r <= two_pi)) return printf("hostile rem_carrier %a\n", r), 1;
                    (void)ddm_rem_code(rem, 2147483647, f0);
                    (void)ddm_tau(0, 1, fs);
                    (void)ddm_bins(f0, rem);
                    ++cases;
                }
    }
    // ---- the frequency grid
    const double grids[][2] = {{500.0, 25.0}, {250.0, 12.5}, {125.0, 10.0}, {100.0, 7.0}, {3.0, 5.0}, {0.0, 1.0}, {2000.0, 500.0}, {51200.0, 12.5}};
    for (const auto& g : grids) {
        const int K = ddm_bins(g[0], g[1]);
        if (K != 2 * (int)std::floor(g[0] / g[1]) + 1) return printf("bins %g %g -> %d\n", g[0], g[1], K), 1;
        for (int k = 0; k < K; ++k, ++cases)
            if (ddm_offset_hz(k, K, g[1]) != -ddm_offset_hz(K - 1 - k, K, g[1]) || std::fabs(ddm_offset_hz(k, K, g[1])) > g[0])
                return printf("offset %d of %d\n", k, K), 1;
        if (ddm_offset_hz((K - 1) / 2, K, g[1]) != 0.0) return printf("centre of %d\n", K), 1;
    }
    if (ddm_bins(100.0, 0.0) || ddm_bins(-1.0, 5.0) || ddm_bins(100.0, -5.0) || ddm_bins(nan, 5.0) || ddm_bins(100.0, nan) ||
        ddm_bins(inf, 5.0) || ddm_bins(100.0, inf) || ddm_bins(1e300, 1e-300))
        return printf("a bad grid was accepted\n"), 1;
    if (ddm_spacing(-4.0, 0.25, 16) != 0.0 || ddm_spacing(1.5, 0.0, 1000) != 1.5) return printf("spacing\n"), 1;
    // ---- the launch geometry
    for (int n_cus = 0; n_cus <= 304; n_cus += 19)
        for (int T = 1; T <= SDR_CORR_MAX_TAPS; ++T)
            for (int64_t segs : {(int64_t)1, (int64_t)3, (int64_t)64, (int64_t)512, (int64_t)100000, (int64_t)kDdmMaxItems * kDdmMaxAll}) {
                const DdmGeometry g = ddm_geometry(segs, T, n_cus);
                ++cases;
                if (g.chunks < 1 || g.taps_per_group < 1 || g.taps_per_group > kDdmThreads || g.lanes_per_tap < 1 ||
                    g.taps_per_group * g.lanes_per_tap > kDdmThreads || (int64_t)g.chunks * g.taps_per_group < T ||
                    (int64_t)(g.chunks - 1) * g.taps_per_group >= T)
                    return printf("geometry segs %lld T %d cus %d: %d chunks x %d taps x %d lanes\n", (long long)segs, T, n_cus, g.chunks, g.taps_per_group, g.lanes_per_tap), 1;
                // as few chunks as fill the device: one chunk fewer would not (or would not hold the taps)
                const int64_t fill = 2 * (int64_t)(n_cus > 1 ? n_cus : 1);
                const int fewest = (T + kDdmThreads - 1) / kDdmThreads;
                if (g.chunks > fewest && segs * (g.chunks - 1) >= fill && (T + g.chunks - 2) / (g.chunks - 1) <= kDdmThreads) {
                    const int tpg = (T + g.chunks - 2) / (g.chunks - 1);
                    if ((T + tpg - 1) / tpg == g.chunks - 1) return printf("geometry segs %lld T %d cus %d: %d chunks, %d would fill\n", (long long)segs, T, n_cus, g.chunks, g.chunks - 1), 1;
                }
            }
    for (int G = 1; G <= kDdmThreads; ++G)
        for (int len : {1, 2, 7, 255, 256, 2047, 2048}) {
            int prev = 0;
            for (int g = 0; g < G; ++g, ++cases) {
                int lo, hi;
                ddm_lane_piece(len, g, G, &lo, &hi);
                if (lo != prev || hi < lo || hi > len) return printf("lane piece len %d g %d G %d\n", len, g, G), 1;
                prev = hi;
            }
            if (prev != len) return printf("lane pieces of len %d G %d end at %d\n", len, G, prev), 1;
        }
    printf("ok %ld\n", cases);
    return 0;
}
