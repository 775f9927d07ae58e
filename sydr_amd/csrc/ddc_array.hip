// Antenna arrays in the down-converter (sdr_ddc_create_array, sdr_ddc_array_weights, sdr_ddc_array_covariance): the K elements of
// a multi-element recording are combined, x = w^H s, where ddc.hip's converter kernel loads its inputs (DdcArrayLoad,
// ddc_handle.h; the arithmetic is ddc_array.h) -- before the mixer, the FIR, the mitigator and the ring, so nothing downstream
// changes and a packed array recording stays packed over the link and in HBM.  This file holds the handle's new entry points
// and the opt-in covariance pass; what both must give is stated in include/sydr_amd.h and, as NumPy, in
// sydr_amd/signal/array.py.
//
// ddc_array_cov_kernel: one pass over the staged bytes of a push, behind the converter's kernel on the same stream.  A workgroup
// takes kCovChunk consecutive frames, a lane the frames kCovThreads apart of them (kCovRun at most), and keeps the K (K + 1) / 2
// Hermitian entries of sum_j s_a conj(s_b) in registers; the wave adds by a butterfly of shuffles, the workgroup through LDS,
// and ONE 64-bit integer atomic add per entry per workgroup reaches memory.  Integer adds commute: the sums are exact and the
// same on every run (probe.hip's moments are made the same way).
// Partial sums of INT8 and PACKED fields are int32: an entry grows by |sr_a sr_b + si_a si_b| <= 2 * 128 * 128 = 2^15 per frame, a
// lane's kCovRun = 64 frames give at most 2^21, a wave's 64 lanes 2^27, the workgroup's four waves 2^29 < 2^31: nothing can
// overflow before the one conversion to 64 bits in front of the atomic.  INT16 fields reach 2^31 in ONE frame, so their
// products are widened before they are added and every partial is int64.
// FLOAT32 fields take the same shape with fp64 partials (the wave's butterfly and the waves' order are fixed) but no float
// atomics: a workgroup stores its 64 sums as a row of a slab and ddc_array_cov_finish_kernel adds the rows in ascending order
// onto the running sums -- the same pushes give the same bits.
#include "engine_internal.h"
#include "ddc_cov.h"

#include <cmath>
#include <new>

using namespace sdr;

namespace {

// `out`: the 64 running sums (integer modes: added to atomically) or the slab [workgroups][64] (float: row blockIdx.x stored).
template <int K, int MODE>
__global__ __launch_bounds__(kCovThreads) void ddc_array_cov_kernel(const void* __restrict__ in, int64_t n_in, DdcLayout lay, DdcArray arr,
                                                                    void* __restrict__ out) {
    typedef typename CovTypes<MODE>::acc Acc;
    __shared__ Acc part[kCovWaves][kDdcArrayCovSlots];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Acc acc[K * K];     // (a, b), a <= b: the real part at a * K + b, the imaginary part (a < b) at b * K + a
#pragma unroll
    for (int s = 0; s < K * K; ++s) acc[s] = 0;
    const int64_t base = (int64_t)blockIdx.x * kCovChunk;
    for (int r = 0; r < kCovRun; ++r) {
        const int64_t j = base + (int64_t)r * kCovThreads + tid;
        if (j >= n_in) break;
        const DdcFrame fr = ddc_array_frame(in, j, lay);
        Acc sr[K], si[K];
#pragma unroll
        for (int a = 0; a < K; ++a) {
            if (MODE == kCovFloat) {
                double re, im;
                ddc_array_element(in, j, lay, fr, arr.lanes[a], &re, &im);
                sr[a] = (Acc)re, si[a] = (Acc)im;
            } else {
                int re, im;
                ddc_array_element_int(in, j, lay, fr, arr.lanes[a], &re, &im);
                sr[a] = (Acc)re, si[a] = (Acc)im;     // (wide: the products below are formed in 64 bits)
            }
        }
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
            for (int b = a; b < K; ++b) {
                acc[a * K + b] += sr[a] * sr[b] + si[a] * si[b];
                if (b > a) acc[b * K + a] += si[a] * sr[b] - sr[a] * si[b];
            }
    }
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) {
            const Acc t = cov_wave_add(acc[a * K + b]);
            if (lane == 0) part[wave][a * kDdcArrayMax + b] = t;     // (slot a * 8 + b: ddc_array_cov_re / _im with K = 8's stride)
        }
    __syncthreads();
    if (tid < kDdcArrayCovSlots) {
        const bool used = (tid >> 3) < K && (tid & 7) < K;
        Acc t = 0;
        if (used)
            for (int w = 0; w < kCovWaves; ++w) t += part[w][tid];
        if (MODE == kCovFloat) ((double*)out)[(size_t)blockIdx.x * kDdcArrayCovSlots + tid] = (double)t;
        else if (used) atomicAdd((unsigned long long*)out + tid, (unsigned long long)(long long)t);     // (two's complement: the signed sum)
    }
}

// The float pass's rows in workgroup order onto the running sums: one lane per slot.
__global__ __launch_bounds__(kDdcArrayCovSlots) void ddc_array_cov_finish_kernel(const double* __restrict__ slab, int64_t rows, double* __restrict__ cov) {
    const int c = threadIdx.x;
    double t = cov[c];
    for (int64_t r = 0; r < rows; ++r) t += slab[(size_t)r * kDdcArrayCovSlots + c];
    cov[c] = t;
}

}  // namespace

void sdr::ddc_array_cov_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in) {
    ProfScope ps(e, "ddc_array_cov_kernel");
    const int mode = cov_mode(d->layout);
    const unsigned grid = (unsigned)cov_workgroups(n_in);
    const void* in = (const void*)e->ddc_stage.ptr;
    void* out = mode == kCovFloat ? d->cov_slab.ptr : d->cov;
    cov_dispatch(d->array.K, mode, [&](auto k, auto m) {
        hipLaunchKernelGGL((ddc_array_cov_kernel<decltype(k)::value, decltype(m)::value>), dim3(grid), dim3(kCovThreads), 0, e->stream, in, n_in,
                           d->layout, d->array, out);
    });
    if (mode == kCovFloat)
        hipLaunchKernelGGL(ddc_array_cov_finish_kernel, dim3(1), dim3(kDdcArrayCovSlots), 0, e->stream, (const double*)d->cov_slab.ptr, (int64_t)grid,
                           (double*)d->cov);
    d->cov_n += n_in;
}

extern "C" {

int sdr_ddc_create_array(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, const sdr_ddc_layout* layout, const sdr_ddc_array* array,
                         sdr_ddc** out) {
    return ddc_create(e, kDdcKindArray, cfg, interpolation, layout, array, 0, nullptr, out);
}

int sdr_ddc_array_weights(sdr_engine* e, sdr_ddc* d, const double* w) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->kind < kDdcKindArray) return sdr_fail(SDR_ERR_INVALID, "the converter has no array");
    if (d->kind == kDdcKindStap) return sdr_fail(SDR_ERR_INVALID, "a space-time converter takes sdr_ddc_stap_weights and sdr_ddc_stap_covariance");
    if (!w) return sdr_fail(SDR_ERR_INVALID, "weights is NULL");
    if (!ddc_array_weights_valid(d->array.K, w)) return sdr_fail(SDR_ERR_INVALID, "a weight is not finite");
    // the kernels take the weights by value with every launch: the pushes queued so far keep theirs, the next one has these
    for (int a = 0; a < d->array.K; ++a) d->array.w[a][0] = w[2 * a], d->array.w[a][1] = w[2 * a + 1];
    return SDR_OK;
}

int sdr_ddc_array_covariance(sdr_engine* e, sdr_ddc* d, double* R, int64_t* n, int clear) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->kind < kDdcKindArray) return sdr_fail(SDR_ERR_INVALID, "the converter has no array");
    if (d->kind == kDdcKindStap) return sdr_fail(SDR_ERR_INVALID, "a space-time converter takes sdr_ddc_stap_weights and sdr_ddc_stap_covariance");
    if (!R || !n) return sdr_fail(SDR_ERR_INVALID, "no result block for the covariance or its count");
    if (!d->cov) return sdr_fail(SDR_ERR_STATE, "the converter was made without SDR_DDC_ARRAY_MEASURE");
    int64_t slots[kDdcArrayCovSlots];
    SDR_HIP(hipMemcpyAsync(slots, d->cov, sizeof(slots), hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    const int K = d->array.K;
    const bool is_float = d->layout.kind == kDdcFieldFloat32;
    const double* as_double = (const double*)slots;
    for (int a = 0; a < K; ++a)
        for (int b = a; b < K; ++b) {
            // each sum converted to double once, here; the lower triangle is the conjugate of the upper
            const int re_at = ddc_array_cov_re(a, b), im_at = ddc_array_cov_im(a, b);
            double re, im, im_low;
            if (is_float) re = as_double[re_at], im = a == b ? 0.0 : as_double[im_at], im_low = a == b ? 0.0 : -im;
            else re = (double)slots[re_at], im = a == b ? 0.0 : (double)slots[im_at], im_low = a == b ? 0.0 : (double)-slots[im_at];
            R[2 * (a * K + b)] = re, R[2 * (a * K + b) + 1] = im;
            R[2 * (b * K + a)] = re, R[2 * (b * K + a) + 1] = im_low;
        }
    *n = d->cov_n;
    if (clear) {
        SDR_HIP(hipMemsetAsync(d->cov, 0, sizeof(slots), e->stream));
        d->cov_n = 0;
    }
    return SDR_OK;
}

}  // extern "C"
