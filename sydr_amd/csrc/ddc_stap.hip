// Space-time adaptive weights in the array down-converter (sdr_ddc_create_stap, sdr_ddc_stap_weights, sdr_ddc_stap_covariance):
// a T-tap FIR per antenna element in front of the mixer, x_j = sum_t sum_a conj(w[t][a]) s_a[j - t], combined where
// ddc.hip's converter kernel loads its inputs (DdcStapLoad, ddc_handle.h; the arithmetic and the raw tail are ddc_stap.h).
// The time taps give nulls that depend on frequency: two elements remove several partial-band jammers from different
// directions.  This file holds the handle's entry points and the opt-in lag-covariance pass; what both must give is stated in
// include/sydr_amd.h and, as NumPy, in sydr_amd/signal/stap.py.
//
// The 64 weights are a kernel argument by value (DdcStap, 1 KiB): a queued push keeps the weights it was queued with, and with
// the tap and element loops unrolled on constant indices they are read by scalar loads where they are used.  The T frames of an
// input are decoded per input -- a frame is decoded T times in all; for the packed and 8-bit fields this is for, a frame is one
// or two loads.
//
// ddc_stap_cov_kernel: ddc_array_cov_kernel's shape with the lag as the grid's second dimension.  Workgroup (x, tau) takes
// kCovChunk consecutive frames j of the push and keeps the K x K complex entries of sum_j s_a[j] conj(s_b[j - tau]) in
// registers -- all of them, a lag's matrix is not Hermitian.  The partner frame j - tau is decoded from the staged bytes, or,
// before the push's first frame, read from the raw tail, which the history kernel BEHIND this pass brings up to date.  The
// exactness is the array pass's: INT8 and PACKED entries grow by at most 2 * 128 * 128 = 2^15 per frame, so int32 partials hold
// a lane's 64 frames (2^21), a wave (2^27) and the workgroup's four waves (2^29); INT16 fields are widened before the product and
// every partial is int64; ONE 64-bit integer atomic add per entry per workgroup reaches memory.  FLOAT32 fields: fp64 partials,
// a workgroup stores its row of a slab [x][tau][slots] and ddc_stap_cov_finish_kernel adds the rows in ascending x.
#include "engine_internal.h"
#include "ddc_cov.h"

#include <cmath>
#include <new>

using namespace sdr;

namespace {

// The K elements of frame f of the push (f >= 0: the staged bytes; f < 0: slot T - 1 + f of the raw tail, whose doubles hold the
// integers of an integer field exactly).
template <int K, int MODE>
__device__ __forceinline__ void cov_elements(const void* __restrict__ in, const double* __restrict__ tail, int64_t f, int T, const DdcLayout& lay,
                                             const DdcArray& arr, typename CovTypes<MODE>::el* sr, typename CovTypes<MODE>::el* si) {
    typedef typename CovTypes<MODE>::el El;
    if (f >= 0) {
        const DdcFrame fr = ddc_array_frame(in, f, lay);
#pragma unroll
        for (int a = 0; a < K; ++a) {
            if (MODE == kCovFloat) {
                double re, im;
                ddc_array_element(in, f, lay, fr, arr.lanes[a], &re, &im);
                sr[a] = (El)re, si[a] = (El)im;
            } else {
                int re, im;
                ddc_array_element_int(in, f, lay, fr, arr.lanes[a], &re, &im);
                sr[a] = (El)re, si[a] = (El)im;
            }
        }
    } else {
        const int slot = T - 1 + (int)f;
#pragma unroll
        for (int a = 0; a < K; ++a) {
            double re, im;
            ddc_stap_tail_load(tail, slot, K, a, &re, &im);
            sr[a] = (El)re, si[a] = (El)im;
        }
    }
}

// `out`: the T x kDdcStapCovSlots running sums (integer modes: added to atomically) or the slab [workgroups x][T][slots].
template <int K, int MODE>
__global__ __launch_bounds__(kCovThreads) void ddc_stap_cov_kernel(const void* __restrict__ in, const double* __restrict__ tail, int64_t n_in, int T,
                                                                   DdcLayout lay, DdcArray arr, void* __restrict__ out) {
    typedef typename CovTypes<MODE>::acc Acc;
    typedef typename CovTypes<MODE>::el El;
    __shared__ Acc part[kCovWaves][kDdcStapCovSlots];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tau = blockIdx.y;
    Acc acc[2 * K * K];     // (a, b): the real part at 2 (a K + b), the imaginary part behind it
#pragma unroll
    for (int s = 0; s < 2 * K * K; ++s) acc[s] = 0;
    const int64_t base = (int64_t)blockIdx.x * kCovChunk;
    for (int r = 0; r < kCovRun; ++r) {
        const int64_t j = base + (int64_t)r * kCovThreads + tid;
        if (j >= n_in) break;
        El sr[K], si[K], pr[K], pi[K];
        cov_elements<K, MODE>(in, tail, j, T, lay, arr, sr, si);
        if (tau == 0) {
#pragma unroll
            for (int a = 0; a < K; ++a) pr[a] = sr[a], pi[a] = si[a];
        } else {
            cov_elements<K, MODE>(in, tail, j - tau, T, lay, arr, pr, pi);
        }
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = 0; b < K; ++b) {
                // (wide: an INT16 product reaches 2^30 and a sum of two 2^31, so each is formed in 64 bits)
                acc[2 * (a * K + b)] += (Acc)sr[a] * (Acc)pr[b] + (Acc)si[a] * (Acc)pi[b];
                acc[2 * (a * K + b) + 1] += (Acc)si[a] * (Acc)pr[b] - (Acc)sr[a] * (Acc)pi[b];
            }
    }
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const Acc t = cov_wave_add(acc[2 * (a * K + b) + c]);
                if (lane == 0) part[wave][ddc_stap_cov_slot(a, b) + c] = t;
            }
    __syncthreads();
    if (tid < kDdcStapCovSlots) {
        const bool used = (tid >> 4) < K && ((tid >> 1) & 7) < K;
        Acc t = 0;
        if (used)
            for (int w = 0; w < kCovWaves; ++w) t += part[w][tid];
        const size_t row = (size_t)tau * kDdcStapCovSlots + tid;
        if (MODE == kCovFloat) ((double*)out)[(size_t)blockIdx.x * T * kDdcStapCovSlots + row] = (double)t;
        else if (used) atomicAdd((unsigned long long*)out + row, (unsigned long long)(long long)t);     // (two's complement: the signed sum)
    }
}

// The float pass's rows in workgroup order onto the running sums: a workgroup per lag, one lane per slot.
__global__ __launch_bounds__(kDdcStapCovSlots) void ddc_stap_cov_finish_kernel(const double* __restrict__ slab, int64_t rows, int T,
                                                                               double* __restrict__ cov) {
    const size_t c = (size_t)blockIdx.x * kDdcStapCovSlots + threadIdx.x;
    double t = cov[c];
    for (int64_t r = 0; r < rows; ++r) t += slab[(size_t)r * T * kDdcStapCovSlots + c];
    cov[c] = t;
}

}  // namespace

void sdr::ddc_stap_cov_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in) {
    ProfScope ps(e, "ddc_stap_cov_kernel");
    const int mode = cov_mode(d->layout);
    const unsigned grid = (unsigned)cov_workgroups(n_in);
    const void* in = (const void*)e->ddc_stage.ptr;
    void* out = mode == kCovFloat ? d->cov_slab.ptr : d->cov;
    cov_dispatch(d->array.K, mode, [&](auto k, auto m) {
        hipLaunchKernelGGL((ddc_stap_cov_kernel<decltype(k)::value, decltype(m)::value>), dim3(grid, (unsigned)d->stap.T), dim3(kCovThreads), 0,
                           e->stream, in, (const double*)d->tail, n_in, d->stap.T, d->layout, d->array, out);
    });
    if (mode == kCovFloat)
        hipLaunchKernelGGL(ddc_stap_cov_finish_kernel, dim3((unsigned)d->stap.T), dim3(kDdcStapCovSlots), 0, e->stream, (const double*)d->cov_slab.ptr,
                           (int64_t)grid, d->stap.T, (double*)d->cov);
    d->cov_n += n_in;
}

extern "C" {

int sdr_ddc_create_stap(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, const sdr_ddc_layout* layout, const sdr_ddc_array* array,
                        int n_taps, const double* w, sdr_ddc** out) {
    return ddc_create(e, kDdcKindStap, cfg, interpolation, layout, array, n_taps, w, out);
}

int sdr_ddc_stap_weights(sdr_engine* e, sdr_ddc* d, const double* w) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->kind != kDdcKindStap) return sdr_fail(SDR_ERR_INVALID, "the converter was not made by sdr_ddc_create_stap");
    if (!w) return sdr_fail(SDR_ERR_INVALID, "weights is NULL");
    if (!ddc_stap_weights_valid(d->stap.T, d->array.K, w)) return sdr_fail(SDR_ERR_INVALID, "a weight is not finite");
    // the kernels take the weights by value with every launch: the pushes queued so far keep theirs, the next one has these
    ddc_stap_set(&d->stap, d->stap.T, d->array.K, w);
    return SDR_OK;
}

int sdr_ddc_stap_covariance(sdr_engine* e, sdr_ddc* d, double* C, int64_t* n, int clear) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->kind != kDdcKindStap) return sdr_fail(SDR_ERR_INVALID, "the converter was not made by sdr_ddc_create_stap");
    if (!C || !n) return sdr_fail(SDR_ERR_INVALID, "no result block for the covariance or its count");
    if (!d->cov) return sdr_fail(SDR_ERR_STATE, "the converter was made without SDR_DDC_ARRAY_MEASURE");
    int64_t slots[kDdcStapMaxTaps * kDdcStapCovSlots];
    const int T = d->stap.T, K = d->array.K;
    const size_t bytes = (size_t)T * kDdcStapCovSlots * sizeof(int64_t);
    SDR_HIP(hipMemcpyAsync(slots, d->cov, bytes, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    const bool is_float = d->layout.kind == kDdcFieldFloat32;
    const double* as_double = (const double*)slots;
    for (int tau = 0; tau < T; ++tau)
        for (int a = 0; a < K; ++a)
            for (int b = 0; b < K; ++b)
                for (int c = 0; c < 2; ++c) {
                    // each sum converted to double once, here
                    const int at = tau * kDdcStapCovSlots + ddc_stap_cov_slot(a, b) + c;
                    C[2 * ((tau * K + a) * K + b) + c] = is_float ? as_double[at] : (double)slots[at];
                }
    *n = d->cov_n;
    if (clear) {
        SDR_HIP(hipMemsetAsync(d->cov, 0, bytes, e->stream));
        d->cov_n = 0;
    }
    return SDR_OK;
}

}  // extern "C"
