// The arithmetic sdr_ddm (ddm.hip) shares between its host checks and its kernels, as host + device code: the segments of
// an item's window, the NCO state each segment's EPL call starts from, the segment's middle, the frequency grid and the
// launch geometry of the segments kernel -- each exactly as include/sydr_amd.h states it (IEEE fp64, no contraction).
// tests/csrc/ddm_plan_check.hip compiles this file for the host alone (`make check-sanitize`) and holds it against plain
// loops and hostile arguments; sydr_amd/dsp/ddm.py: ddm_statement is the same arithmetic in NumPy.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace sdr {

constexpr int kDdmMaxSegments = 64;      // S: segments per coherent block
constexpr int kDdmMaxAll = 4096;         // Q = B * S: segments per item
constexpr int kDdmMaxBins = 4096;        // K
constexpr int kDdmMaxItems = 65535;
constexpr int kDdmThreads = 256;

struct DdmItemDev {    // what the kernels need of one item (an sdr_epl_item read as a prediction)
    int32_t slot, W;   // W = n_samples, the whole window
    int64_t base;      // start_sample modulo the ring's capacity
    double f0, rem_carrier, rem_code, code_step;
    int32_t L, reserved;
};

// K = 2 * floor(span / step) + 1; 0 for a bad grid (what sdr_ddm_bins returns).
__host__ __device__ inline int ddm_bins(double span_hz, double step_hz) {
    if (!(step_hz > 0.0) || !(span_hz >= 0.0) || !(span_hz - span_hz == 0.0) || !(step_hz - step_hz == 0.0)) return 0;
    const double half = floor(span_hz / step_hz);
    if (!(half < 1e9)) return 0;
    return 2 * (int)half + 1;
}

// Window samples [a, b) of segment q < Q: a = (q*W)/Q, b = ((q+1)*W)/Q (0 < Q <= 4096, 0 < W < 2^31: no overflow).
__host__ __device__ inline void ddm_segment_bounds(int64_t W, int Q, int q, int64_t* a, int64_t* b) {
    *a = ((int64_t)q * W) / Q;
    *b = ((int64_t)(q + 1) * W) / Q;
}

// (rem_carrier + (-(f0*2.0*pi*a/fs))) mod 2*pi with Python's modulo: the result in [0, 2*pi).
__host__ __device__ inline double ddm_rem_carrier(double f0, double rem_carrier, int64_t a, double fs) {
    const double two_pi = 2.0 * M_PI;
    double x = (((f0 * 2.0) * M_PI) * (double)a) / fs;
    x = rem_carrier + (-x);
    double r = fmod(x, two_pi);
    if (r < 0.0) r += two_pi;
    return r == 0.0 ? 0.0 : r;   // (-0.0 -> +0.0, as Python's % gives)
}

// rem_code + (double)a * code_step: the product, then the sum.
__host__ __device__ inline double ddm_rem_code(double rem_code, int64_t a, double code_step) {
    const double adv = (double)a * code_step;
    return rem_code + adv;
}

// The segment's middle in seconds into the window: (a + b - 1) / 2.0 / fs.
__host__ __device__ inline double ddm_tau(int64_t a, int64_t b, double fs) { return (double)(a + b - 1) / 2.0 / fs; }

// d_k = (k - (K-1)/2) * step_hz.
__host__ __device__ inline double ddm_offset_hz(int k, int K, double step_hz) { return (double)(k - (K - 1) / 2) * step_hz; }

// s_j = first_chips + j * step_chips: one multiply, one add.
__host__ __device__ inline double ddm_spacing(double first_chips, double step_chips, int j) {
    const double adv = (double)j * step_chips;
    return first_chips + adv;
}

// Launch geometry of the segments kernel: one workgroup of 256 lanes per (segment of an item, chunk of taps).  Every chunk
// repeats the load-and-wipe stage of its segment, so the taps are cut into as FEW chunks as still gives the device
// `fill` workgroups (two per compute unit) -- or as many as there are taps when even that does not fill it.  A chunk holds
// taps_per_group = ceil(T / chunks) <= 256 taps; lanes_per_tap = 256 / taps_per_group lanes share a tap.
struct DdmGeometry {
    int chunks, taps_per_group, lanes_per_tap;
};

__host__ __device__ inline DdmGeometry ddm_geometry(int64_t n_segments_all, int n_taps, int n_cus) {
    const int64_t fill = 2 * (int64_t)(n_cus > 1 ? n_cus : 1);
    int64_t chunks = (n_taps + kDdmThreads - 1) / kDdmThreads;            // at most 256 taps in a workgroup
    if (n_segments_all * chunks < fill) chunks = (fill + n_segments_all - 1) / n_segments_all;
    if (chunks > n_taps) chunks = n_taps;
    DdmGeometry g;
    g.taps_per_group = (int)((n_taps + chunks - 1) / chunks);
    g.chunks = (n_taps + g.taps_per_group - 1) / g.taps_per_group;      // (drop chunks the rounding left empty)
    g.lanes_per_tap = kDdmThreads / g.taps_per_group;
    return g;
}

// Samples [lo, hi) of a tile of `len` samples that lane g of the G lanes of a tap sums.
__host__ __device__ inline void ddm_lane_piece(int len, int g, int G, int* lo, int* hi) {
    *lo = (int)(((int64_t)len * g) / G);
    *hi = (int)(((int64_t)len * (g + 1)) / G);
}

}  // namespace sdr
