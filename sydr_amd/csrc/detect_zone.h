// The arithmetic sdr_acq_deep_detect (acq_detect.hip) shares between its host checks and its kernels, as host + device
// code: the circular code distance, the exclusion zone of a peak, the test that lets a workgroup skip the per-cell zone
// tests, and how a PRN's map is cut into parts -- each exactly as include/sydr_amd.h states it.
// tests/csrc/detect_zone_check.hip compiles this file for the host alone (`make check-sanitize`) and holds it against a
// brute-force restatement; sydr_amd/dsp/deepsearch.py: deep_detect is the same statement in NumPy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sdr {

constexpr int kDetectMaxPeaks = 8;
constexpr int kDetectThreads = 256;
constexpr int kDetectPairs = 4;                                          // 16-byte loads per lane and part
constexpr int kDetectPartCells = kDetectThreads * kDetectPairs * 2;      // 2048 cells of ONE map row: a constant of the library

// A part is a run of kDetectPartCells columns of one map row (the last run of a row is shorter): parts never straddle rows,
// so a workgroup's row (group, bin) is uniform, and their number depends on the PRN's own map alone.
__host__ __device__ inline int detect_row_parts(int N) { return (N + kDetectPartCells - 1) / kDetectPartCells; }
// Part `part` < rows * detect_row_parts(N) of a PRN, in ascending (row, column) order: its row and its columns [c0, c1).
__host__ __device__ inline void detect_part_bounds(int N, int64_t part, int* row, int* c0, int* c1) {
    const int rp = detect_row_parts(N);
    *row = (int)(part / rp);
    *c0 = (int)(part - (int64_t)*row * rp) * kDetectPartCells;
    *c1 = *c0 + kDetectPartCells < N ? *c0 + kDetectPartCells : N;
}
// Lane `lane`'s i-th pair of a part that starts at column c0: columns n and n + 1 (n even relative to the row, so a pair is
// one 16-byte load where the row starts on a 16-byte boundary).
__host__ __device__ inline int detect_pair_column(int c0, int i, int lane) { return c0 + 2 * (i * kDetectThreads + lane); }

// dist(n, m): the circular distance mod N, 0 <= n, m < N.
__host__ __device__ inline int detect_dist(int n, int m, int N) {
    const int d = n > m ? n - m : m - n;
    return d < N - d ? d : N - d;
}
__host__ __device__ inline bool detect_bin_near(int b, int bj, int excl_bins) {
    const int d = b > bj ? b - bj : bj - b;
    return d <= excl_bins;
}
// Z_j: |b - b_j| <= excl_bins and dist(n, n_j) <= excl_code (every group).
__host__ __device__ inline bool detect_in_zone(int b, int n, int bj, int nj, int N, int excl_code, int excl_bins) {
    return detect_bin_near(b, bj, excl_bins) && detect_dist(n, nj, N) <= excl_code;
}
// May a column of [c0, c1) lie within excl_code of n_j?  Never false where one does (0 <= c0 < c1 <= N, 0 <= n_j < N,
// 0 <= excl_code); false for every run that lies clear of the (possibly wrapping) interval n_j +- excl_code.
__host__ __device__ inline bool detect_run_touches(int c0, int c1, int nj, int N, int excl_code) {
    if (2 * (int64_t)excl_code + 1 >= N) return true;
    const int lo = nj - excl_code, hi = nj + excl_code;      // -N < lo <= hi < 2N
    return (lo < c1 && hi >= c0) || (lo + N < c1 && hi + N >= c0) || (lo - N < c1 && hi - N >= c0);
}
// The call refuses windows that could leave no noise cell: n_peaks * (2*excl_code + 1) >= N.
__host__ __device__ inline bool detect_windows_fit(int n_peaks, int excl_code, int N) {
    return (int64_t)n_peaks * (2 * (int64_t)excl_code + 1) < (int64_t)N;
}

}  // namespace sdr
