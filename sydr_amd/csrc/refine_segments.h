// Stage 1 of sdr_acq_refine (refine.hip) and of sdr_acq_secondary (secondary.hip): the per-segment prompt sums z[item][m][s].
// One kernel, launched by both with the same arguments: refine_segments_kernel, one wave per segment (item, period m,
// segment s), wipes code and coarse carrier off its samples of the ring with the E/P/L correlator's per-sample core
// (correlator.h correlate_epoch, one tap at spacing 0.0: the prompt tap of EPL, hence its parity with the oracle).
// What admits an item to it (RefineItemDev, refine_admit_item) is host code without the engine: secondary_request.h.
#pragma once

#include "correlator.h"
#include "secondary_request.h"

namespace sdr {

static_assert(kRefineLutPad == SDR_LUT_PAD, "refine_admit_item counts the staged row's padding");

static __constant__ double kPromptSpacing[1] = {0.0};   // (one per translation unit, as each has its own code object)

// Window samples [a, b) of segment (m, s): a = m*N + (s*N)/S, b = m*N + ((s+1)*N)/S.
__device__ __forceinline__ void segment_bounds(int N, int S, int m, int s, int64_t& a0, int64_t& a, int64_t& b) {
    a0 = ((int64_t)s * N) / S;
    a = (int64_t)m * N + a0;
    b = (int64_t)m * N + ((int64_t)(s + 1) * N) / S;
}

template <int FMT>
__global__ __launch_bounds__(64) void refine_segments_kernel(const void* __restrict__ ring, int64_t capacity,
                                                             const RefineItemDev* __restrict__ items, int M, int S,
                                                             const uint32_t* __restrict__ luts, int lut_stride, double fs,
                                                             double2* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) uint32_t refine_lut[];
    const int lane = threadIdx.x;
    const int per_item = M * S;
    const int item = blockIdx.x / per_item, q = blockIdx.x - item * per_item;
    const int m = q / S, s = q - m * S;
    const RefineItemDev it = items[item];
    // one code period of the staged replica: chip indices 0 .. L + 1 of the padded table
    stage_lut<64>(refine_lut, luts + (size_t)it.slot * lut_stride, it.lut_words, lane);

    int64_t a0, a, b;
    segment_bounds(it.N, S, m, s, a0, a, b);
    EpochParams ep;
    ep.start_sample = it.base + a;
    ep.n = (int)(b - a);
    ep.carrier_hz = it.f0;
    // the coarse carrier's phase runs on through the window: (-(f0*2.0*pi*a/fs)) mod 2*pi, in [0, 2*pi)
    double rem = fmod(-((((it.f0 * 2.0) * M_PI) * (double)a) / fs), 2.0 * M_PI);
    if (rem < 0.0) rem += 2.0 * M_PI;
    ep.rem_carrier = uniform(rem);
    ep.rem_code = (double)a0 * it.code_step;
    ep.code_step = it.code_step;
    const double dphi = carrier_step(it.f0, fs);
    EpochConsts<1> K;
    compute_constants<1>(K, ep, kPromptSpacing, dphi, 64);
    __syncthreads();   // replica staged

    double accr[1], acci[1];
    correlate_epoch<FMT, 1>(ring, capacity, ep, dphi, K, refine_lut, lane, 64, lane, accr, acci);
    const double re = wave_sum(accr[0]), im = wave_sum(acci[0]);
    if (lane == 0) z[blockIdx.x] = make_double2(re, im);
}

// Stage 1 of either call on the engine's stream: the segment sums of n_items admitted items into z.
inline int refine_launch_segments(sdr_engine* e, const RefineItemDev* d_items, int n_items, int M, int S, int max_words, double fs,
                                  double2* d_z) {
    const dim3 grid((unsigned)(n_items * M * S)), block(64);
    const size_t shmem = (size_t)((max_words + 3) & ~3) * sizeof(uint32_t);
    with_fmt(e->iq_fmt, [&](auto fmt) {
        hipLaunchKernelGGL(refine_segments_kernel<decltype(fmt)::value>, grid, block, shmem, e->stream, (const void*)e->iq,
                           e->iq_capacity, d_items, M, S, e->luts, e->lut_stride, fs, d_z);
    });
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

// (value, index) records order by value, then by the LOWER index: the first maximum in row-major (h, k) order.
// A NaN never wins a comparison: a window that holds NaN / Inf samples (a float ring) keeps the initial record.
__device__ __forceinline__ bool better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

}  // namespace sdr
