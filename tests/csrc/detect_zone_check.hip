// Host-side proof of the arithmetic sdr_acq_deep_detect shares between its checks and its kernels
// (sydr_amd/csrc/detect_zone.h), built with `hipcc --cuda-host-only` under the address and undefined-behaviour sanitizers
// (`make check-sanitize`), against a brute-force restatement that knows nothing of the header's shortcuts:
//  - dist(n, m) for N = 8..17, every n and m: the least |n - m + k*N| over k;
//  - the zone of a peak for every peak position (bin and code), windows 0..N/2 in code and 0..B in bins: zones that wrap at
//    n = 0 / N - 1, zones that clip at bin 0 and at the last bin, and pairs of overlapping zones (the union is what the
//    kernels test: one predicate per peak, OR-ed);
//  - the run test that lets a workgroup skip the per-cell tests: never false where a column of the run lies in the window,
//    and exact while the window does not cover the whole period -- for every run [c0, c1) of those N;
//  - the noise columns of up to three peaks and the refusal n_peaks * (2*excl_code + 1) >= N: an accepted request always
//    leaves a column;
//  - the parts: every (row, column) of a map belongs to exactly one (part, pair, lane, half), parts ascend in row-major
//    order, and no pair reaches beyond its row -- for N around the part size, odd N and N = 2 mod 4.
//   usage: detect_zone_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sydr_amd/csrc/detect_zone.h"

using namespace sdr;

static int brute_dist(int n, int m, int N) {
    int best = 1 << 30;
    for (int k = -2; k <= 2; ++k) best = std::abs(n - m + k * N) < best ? std::abs(n - m + k * N) : best;
    return best;
}
static bool brute_zone(int b, int n, int bj, int nj, int N, int ec, int eb) {
    bool code = false;
    for (int t = -ec; t <= ec; ++t) code |= ((nj + t) % N + N) % N == n;     // walk the window, wrapping
    bool bin = false;
    for (int t = -eb; t <= eb; ++t) bin |= bj + t == b;                      // bins do not wrap: the window clips
    return code && bin;
}

static int check_parts(int rows, int N) {
    std::vector<int> seen((size_t)rows * N, 0);
    const int64_t n_parts = (int64_t)rows * detect_row_parts(N);
    int64_t last = -1;
    for (int64_t part = 0; part < n_parts; ++part) {
        int row, c0, c1;
        detect_part_bounds(N, part, &row, &c0, &c1);
        if (row < 0 || row >= rows || c0 < 0 || c0 >= c1 || c1 > N || c0 % 2) return printf("part %lld of N %d: row %d [%d, %d)\n", (long long)part, N, row, c0, c1), 1;
        if ((int64_t)row * N + c0 <= last) return printf("part %lld of N %d does not ascend\n", (long long)part, N), 1;
        last = (int64_t)row * N + c1 - 1;
        for (int i = 0; i < kDetectPairs; ++i)
            for (int lane = 0; lane < kDetectThreads; ++lane) {
                const int n = detect_pair_column(c0, i, lane);
                if (n % 2) return printf("odd pair column %d\n", n), 1;
                if (n + 1 < c1) {
                    ++seen[(size_t)row * N + n];
                    ++seen[(size_t)row * N + n + 1];
                } else if (n < c1) {
                    ++seen[(size_t)row * N + n];
                }
            }
    }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) return printf("N %d: cell %zu visited %d times\n", N, i, seen[i]), 1;
    return 0;
}

int main() {
    long cases = 0;
    for (int N = 8; N <= 17; ++N) {
        for (int n = 0; n < N; ++n)
            for (int m = 0; m < N; ++m, ++cases)
                if (detect_dist(n, m, N) != brute_dist(n, m, N)) return printf("dist %d %d mod %d\n", n, m, N), 1;
        const int B = 5;
        for (int ec = 0; ec <= N / 2; ++ec)
            for (int eb = 0; eb <= B; ++eb)
                for (int bj = 0; bj < B; ++bj)
                    for (int nj = 0; nj < N; ++nj) {
                        for (int b = 0; b < B; ++b)
                            for (int n = 0; n < N; ++n, ++cases)
                                if (detect_in_zone(b, n, bj, nj, N, ec, eb) != brute_zone(b, n, bj, nj, N, ec, eb))
                                    return printf("zone N %d window %d x %d peak (%d, %d) cell (%d, %d)\n", N, ec, eb, bj, nj, b, n), 1;
                        // a second, overlapping zone: the union is the OR of the predicates
                        const int bk = (bj + 1) % B, nk = (nj + ec) % N;
                        for (int b = 0; b < B; ++b)
                            for (int n = 0; n < N; ++n, ++cases) {
                                const bool got = detect_in_zone(b, n, bj, nj, N, ec, eb) || detect_in_zone(b, n, bk, nk, N, ec, eb);
                                const bool want = brute_zone(b, n, bj, nj, N, ec, eb) || brute_zone(b, n, bk, nk, N, ec, eb);
                                if (got != want) return printf("two zones N %d window %d x %d\n", N, ec, eb), 1;
                            }
                    }
        // the run test
        for (int ec = 0; ec <= N / 2; ++ec)
            for (int nj = 0; nj < N; ++nj)
                for (int c0 = 0; c0 < N; ++c0)
                    for (int c1 = c0 + 1; c1 <= N; ++c1, ++cases) {
                        bool any = false;
                        for (int n = c0; n < c1; ++n) any |= brute_dist(n, nj, N) <= ec;
                        const bool got = detect_run_touches(c0, c1, nj, N, ec);
                        if (any && !got) return printf("run [%d, %d) of %d misses the window %d +- %d\n", c0, c1, N, nj, ec), 1;
                        if (2 * ec + 1 < N && got != any) return printf("run [%d, %d) of %d, window %d +- %d: %d\n", c0, c1, N, nj, ec, (int)got), 1;
                    }
        // the refusal: an accepted request leaves a noise column whatever the peaks
        for (int n_peaks = 1; n_peaks <= 3; ++n_peaks)
            for (int ec = 0; ec <= N / 2; ++ec) {
                const bool fits = detect_windows_fit(n_peaks, ec, N);
                if (fits != (n_peaks * (2 * ec + 1) < N)) return printf("windows_fit %d %d %d\n", n_peaks, ec, N), 1;
                for (int a = 0; a < N; ++a)
                    for (int b = 0; b < N; ++b)
                        for (int c = 0; c < N; ++c, ++cases) {
                            const int at[3] = {a, b, c};
                            int left = 0;
                            for (int n = 0; n < N; ++n) {
                                bool out = false, want = false;
                                for (int j = 0; j < n_peaks; ++j) {
                                    out |= detect_dist(n, at[j], N) <= ec;
                                    want |= brute_zone(0, n, 0, at[j], N, ec, 0);
                                }
                                if (out != want) return printf("noise column %d of %d\n", n, N), 1;
                                left += !out;
                            }
                            if (fits && left < 1) return printf("no noise column: N %d, %d peaks, window %d\n", N, n_peaks, ec), 1;
                        }
            }
    }
    if (detect_windows_fit(8, 1 << 30, 1 << 24) || !detect_windows_fit(8, 4, 4000) || detect_run_touches(0, 8, 3, 16, 1 << 30) != true)
        return printf("large windows\n"), 1;
    // ---- the parts
    for (int N : {2, 3, 8, 17, 2047, 2048, 2049, 4000, 4001, 4006, 4096, 4097, 6145}) {
        for (int rows : {1, 3}) {
            if (check_parts(rows, N)) return 1;
            ++cases;
        }
        if (detect_row_parts(N) != (N + kDetectPartCells - 1) / kDetectPartCells) return printf("row parts of %d\n", N), 1;
    }
    if (kDetectPartCells != 2048 || detect_row_parts(1 << 24) > 65535) return printf("part size\n"), 1;
    printf("ok %ld\n", cases);
    return 0;
}
