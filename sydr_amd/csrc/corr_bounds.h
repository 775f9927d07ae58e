// The chip runs of one tap of sdr_corr_profile (corr_profile.hip), as host + device code: the reference's per-sample chip
// index (sydr/dsp/tracking.py:111-112)
//     idx_i = ceil(linspace(shift, code_step*n + shift, n, endpoint=False))_i,   shift = rem_code + spacing
// is constant over runs of samples (one run per chip wherever a chip holds a sample); a tap's sum is then a sum over runs
// of the chip's sign times a difference of prefix sums.  What is here maps (n, rem_code, code_step, spacing) to the runs as
// pairs (first sample, padded index) -- exactly the run-length encoding of NumPy's expression: a run's first sample is
// PREDICTED on the real line and then settled with the per-sample expression itself, evaluated operation for operation
// (IEEE fp64, no FMA: SURVEY.md H3).  tests/csrc/corr_bounds_check.hip compiles this file for the host alone and prints
// the runs; tests/test_corr_profile.py holds them against NumPy.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace sdr {

// np.linspace(shift, code_step*n + shift, n, endpoint=False): y_i = fl(fl(i * step) + shift)
struct CorrTap {
    double shift, step;
    double inv_step;   // 1/step: only ever PREDICTS where a run ends
};

__host__ __device__ inline CorrTap corr_tap(int n, double rem_code, double code_step, double spacing) {
    CorrTap t;
    const double nd = (double)n;
    t.shift = rem_code + spacing;   // reference arithmetic, operation for operation
    double stop = code_step * nd;
    stop = stop + t.shift;
    const double delta = stop - t.shift;
    t.step = delta / nd;
    t.inv_step = 1.0 / t.step;
    return t;
}

// Padded index of sample i (the caller keeps it inside +-2^30: sdr_corr_profile refuses what would leave that range).
__host__ __device__ inline int corr_index(const CorrTap& t, int i) {
    double y = (double)i * t.step;   // separate multiply, add, ceil
    y = y + t.shift;
    return (int)ceil(y);
}

// Chip of the code a padded index stands for: (p - 1) mod L with Python's modulo, for any p.
__host__ __device__ inline int corr_chip(int p, int L) {
    const int r = (p - 1) % L;
    return r < 0 ? r + L : r;
}

// ... and of a later index, d = p_next - p >= 0 indices on (as an unsigned: the whole range is 2^31 wide).
__host__ __device__ inline int corr_chip_advance(int q, unsigned d, int L) {
    unsigned u = (unsigned)q + d;
    if (u >= (unsigned)L) {
        u -= (unsigned)L;
        if (u >= (unsigned)L) u %= (unsigned)L;   // (more than a code period per sample)
    }
    return (int)u;
}

// Sample a has index p.  -> the first sample e in (a, b] whose index exceeds p (b: there is none before b), *p_next = its
// index (p when e == b).  The indices never decrease with i (step >= 0, rounding is monotone), so the real-line
// prediction floor((p - shift) / step) + 1 -- within one sample of the truth at receiver rates -- is walked to the exact
// boundary with the per-sample expression on both sides of it; a prediction that is far off (absurd parameters) costs
// evaluations, never exactness.
__host__ __device__ inline int corr_run_end(const CorrTap& t, int a, int b, int p, int* p_next) {
    int e = b;
    if (t.step > 0.0) {
        const double est = floor(((double)p - t.shift) * t.inv_step) + 1.0;
        e = !(est > (double)(a + 1)) ? a + 1 : (!(est < (double)b) ? b : (int)est);   // (NaN: a + 1)
    }
    int pe = p;
    if (e < b) pe = corr_index(t, e);
    if (e < b && pe <= p) {
        do {
            ++e;
            if (e == b) break;
            pe = corr_index(t, e);
        } while (pe <= p);
    } else {
        while (e > a + 1) {
            const int pm = corr_index(t, e - 1);
            if (pm <= p) break;
            --e;
            pe = pm;
        }
    }
    *p_next = e < b ? pe : p;
    return e;
}

}  // namespace sdr
