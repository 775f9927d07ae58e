// Rational-rate resampling in the down-converter (sdr_ddc_create_rational): interpolation by L, a prototype FIR at the
// up-sampled rate, decimation by M -- a 16.368 MHz recording enters the ring at 12 MHz (250 / 341).  The mixer is ddc.hip's;
// of the zero-stuffed stream only the non-zero products are formed: output m takes the K_p taps h[p + k L] of its phase
// p = (m M) mod L against the inputs z_{q-k}, q = (m M) div L.  What the ring must hold is stated in include/sydr_amd.h and,
// as NumPy, in sydr_amd/signal/downconvert.py: the same products added in the same order whatever tile or push an output
// falls into, so the ring does not depend on how the stream was cut into pushes, bit for bit.
// Lanes of consecutive outputs sit on different phases, so the taps are no longer wave-uniform: they come by per-lane
// (vector) loads from a table laid out [k][r], r the output's index within the period of L' = L / gcd(L, M) outputs -- for a
// fixed k the loads of a wave are one contiguous run (a wrap at L' aside).  Every index comes from resample_tiles.h.
#include "engine_internal.h"
#include "ddc_handle.h"
#include "resample_tiles.h"
#include "sincos_reduced.h"

#include <cmath>
#include <new>
#include <vector>

using namespace sdr;

// One workgroup per tile of outputs.  Phase 1 is ddc_kernel's: the tile's inputs, each loaded (the push's block or the raw
// history) and mixed once, into LDS as fp64 complex.  Phase 2: a lane per output, its K_p taps down its column of the table,
// k ascending, product then sum (no contraction: the NumPy statement's own operations); then gain and the store in the ring's
// format, a ci8 ring's bytes sign-flipped.
// `load` reads an input as ddc.hip's kernels do: one of the four formats (resample_kernel), a layout's frames
// (resample_layout_kernel), an array's combined elements (resample_array_kernel) or a space-time array's (resample_stap_kernel).
template <class Load>
__device__ __forceinline__ void resample_kernel_body(double2* z, const void* __restrict__ in, const void* __restrict__ hist,
                                                     const double* __restrict__ table, void* __restrict__ ring, const RsPush& push, int tile,
                                                     const Load& load, int out_fmt, uint64_t fcw, double gain, int64_t ring_offset,
                                                     int64_t capacity) {
    const RsTile t = rs_tile(push, tile, blockIdx.x);
    for (int i = threadIdx.x; i < t.span; i += kRsThreads) {
        const int64_t j = t.j0 + i;
        const int64_t src = rs_source(push, j);
        double xr = 0.0, xi = 0.0;
        if (src < 0) load.history(hist, ~src, &xr, &xi);
        else if (src < push.n_in) load.block(in, src, &xr, &xi);
        const uint64_t p = (uint64_t)j * fcw;                       // (j < 0: x = 0 whatever the phasor)
        const double turn = (double)(p >> 11) * 0x1p-53;
        double s, c;
        sincos_reduced(6.283185307179586 * turn, &s, &c);
        z[i] = make_double2(xr * c + xi * s, xi * c - xr * s);
    }
    __syncthreads();
    const int Lp = push.Lp;
    for (int o = threadIdx.x; o < t.count; o += kRsThreads) {
        const RsOutput w = rs_output(push, t, o);
        const double2* zo = z + w.at;
        const double* h_col = table + w.r;
        double ar = 0.0, ai = 0.0;
        for (int k = 0; k < w.K; ++k) {
            const double h = h_col[(size_t)k * Lp];
            const double2 v = zo[-k];
            ar += h * v.x;
            ai += h * v.y;
        }
        ar *= gain, ai *= gain;
        const int64_t pos = ddc_ring_pos(ring_offset, t.i0 + o, capacity);
        switch (out_fmt) {
            case SDR_FMT_CI8: {
                const int re = (int)ddc_clip_rint(ar, 127.0), im = (int)ddc_clip_rint(ai, 127.0);
                ((uint16_t*)ring)[pos] = (uint16_t)((((unsigned)re & 0xffu) | (((unsigned)im & 0xffu) << 8)) ^ 0x8080u);
                break;
            }
            case SDR_FMT_CI16: {
                const int re = (int)ddc_clip_rint(ar, 32767.0), im = (int)ddc_clip_rint(ai, 32767.0);
                ((uint32_t*)ring)[pos] = ((unsigned)re & 0xffffu) | (((unsigned)im & 0xffffu) << 16);
                break;
            }
            case SDR_FMT_CF32: ((float2*)ring)[pos] = make_float2((float)ar, (float)ai); break;
            default: ((double2*)ring)[pos] = make_double2(ar, ai); break;
        }
    }
}

__global__ __launch_bounds__(kRsThreads) void resample_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                              const double* __restrict__ table, void* __restrict__ ring, RsPush push, int tile,
                                                              int in_fmt, int out_fmt, uint64_t fcw, double gain, int64_t ring_offset,
                                                              int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    resample_kernel_body((double2*)rs_smem, in, hist, table, ring, push, tile, DdcFormatLoad{in_fmt}, out_fmt, fcw, gain, ring_offset, capacity);
}

__global__ __launch_bounds__(kRsThreads) void resample_layout_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                                     const double* __restrict__ table, void* __restrict__ ring, RsPush push,
                                                                     int tile, DdcLayout lay, int out_fmt, uint64_t fcw, double gain,
                                                                     int64_t ring_offset, int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    resample_kernel_body((double2*)rs_smem, in, hist, table, ring, push, tile, DdcLayoutLoad{lay, ddc_layout_history(lay)}, out_fmt, fcw, gain,
                         ring_offset, capacity);
}

__global__ __launch_bounds__(kRsThreads) void resample_array_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                                    const double* __restrict__ table, void* __restrict__ ring, RsPush push,
                                                                    int tile, DdcLayout lay, DdcArray arr, int out_fmt, uint64_t fcw, double gain,
                                                                    int64_t ring_offset, int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    resample_kernel_body((double2*)rs_smem, in, hist, table, ring, push, tile, DdcArrayLoad{lay, arr}, out_fmt, fcw, gain, ring_offset, capacity);
}

__global__ __launch_bounds__(kRsThreads) void resample_stap_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                                   const double* __restrict__ tail, const double* __restrict__ table,
                                                                   void* __restrict__ ring, RsPush push, int tile, DdcLayout lay, DdcArray arr,
                                                                   DdcStap stap, int out_fmt, uint64_t fcw, double gain, int64_t ring_offset,
                                                                   int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char rs_smem[];
    resample_kernel_body((double2*)rs_smem, in, hist, table, ring, push, tile, DdcStapLoad{lay, arr, stap, tail}, out_fmt, fcw, gain, ring_offset,
                         capacity);
}

namespace sdr {

// sdr_ddc_push / _queue of a converter with L > 1: ddc.hip's push with the resampler's counts and kernels.
int rs_push_impl(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t off, int64_t* n_out, bool wait) {
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (n_in < 0) return sdr_fail(SDR_ERR_INVALID, "negative input count");
    if (!in && n_in > 0) return sdr_fail(SDR_ERR_INVALID, "host pointer is NULL");
    const int64_t cap = e->iq_capacity;
    if (off < 0 || off >= cap) return sdr_fail(SDR_ERR_RANGE, "ring offset %lld outside the ring of %lld samples", (long long)off, (long long)cap);
    if (!rs_in_range(d->n_seen, n_in, d->L))
        return sdr_fail(SDR_ERR_RANGE, "%lld inputs behind %lld take the up-sampled index past 2^62", (long long)n_in, (long long)d->n_seen);
    const RsPush push = rs_push(d->n_seen, n_in, d->L, d->D, d->T);
    if (push.n_out > cap)
        return sdr_fail(SDR_ERR_RANGE, "%lld outputs exceed the ring capacity %lld", (long long)push.n_out, (long long)cap);
    size_t bytes = 0;
    if (int rc = ddc_push_bytes(d, n_in, &bytes)) return rc;
    if (n_out) *n_out = push.n_out;
    if (n_in == 0) return SDR_OK;
    ProfScope whole(e, "call_ddc_push");
    if (int rc = sdr_devbuf_reserve(e, &e->ddc_stage, bytes)) return rc;
    if (d->has_array)
        if (int rc = ddc_array_cov_reserve(e, d, n_in)) return rc;
    // with a mitigator the kernel's destination is its linear cf64 work buffer, the first output behind the kept state
    void* dst = e->iq;
    int dst_fmt = e->iq_fmt;
    int64_t dst_off = off, dst_cap = cap;
    if (d->mit && push.n_out > 0) {
        if (int rc = mit_push_begin(e, d->mit, push.m_first, push.n_out, &dst, &dst_off, &dst_cap)) return rc;
        dst_fmt = SDR_FMT_CF64;
    }
    SDR_HIP(hipMemcpyAsync(e->ddc_stage.ptr, in, bytes, hipMemcpyHostToDevice, e->stream));
    if (push.n_out > 0) {
        sdr_iq_mark_written(e, off, push.n_out);
        const int tile = rs_tile_outputs(d->L, d->D, d->T);
        const int64_t tiles = rs_tiles(push, tile);
        const size_t lds = (size_t)rs_tile_span_max(d->L, d->D, d->T, tile) * sizeof(double2);
        ProfScope ps(e, "resample_kernel");
        if (d->has_stap)
            hipLaunchKernelGGL(resample_stap_kernel, dim3((unsigned)tiles), dim3(kRsThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->tail, (const double*)d->taps, dst, push, tile, d->layout, d->array, d->stap,
                               dst_fmt, d->fcw, d->gain, dst_off, dst_cap);
        else if (d->has_array)
            hipLaunchKernelGGL(resample_array_kernel, dim3((unsigned)tiles), dim3(kRsThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->taps, dst, push, tile, d->layout, d->array, dst_fmt, d->fcw, d->gain, dst_off,
                               dst_cap);
        else if (d->has_layout)
            hipLaunchKernelGGL(resample_layout_kernel, dim3((unsigned)tiles), dim3(kRsThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->taps, dst, push, tile, d->layout, dst_fmt, d->fcw, d->gain, dst_off, dst_cap);
        else
            hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles), dim3(kRsThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->taps, dst, push, tile, d->in_fmt, dst_fmt, d->fcw, d->gain, dst_off, dst_cap);
    }
    if (d->mit && push.n_out > 0)
        if (int rc = mit_push_finish(e, d->mit, push.m_first, push.n_out, off)) return rc;
    if (d->has_array) ddc_array_cov_launch(e, d, n_in);
    if (push.Tp > 1 || (d->has_stap && d->stap.T > 1)) ddc_history_launch(e, d, n_in);     // (the last Tp - 1 raw inputs: the integer converter's splice and kernel)
    SDR_HIP(hipGetLastError());
    d->n_seen += n_in;
    if (wait) SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

}  // namespace sdr

extern "C" int sdr_ddc_create_rational(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, sdr_ddc** out) {
    if (interpolation == 1) return sdr_ddc_create(e, cfg, out);     // the integer converter itself: ddc_kernel, its launches, its bytes
    if (int rc = sdr_set_device(e)) return rc;
    if (!cfg || !out) return sdr_fail(SDR_ERR_INVALID, "NULL configuration or result pointer");
    *out = nullptr;
    const int L = interpolation, M = cfg->decimation, T = cfg->n_taps;
    if (cfg->in_fmt < SDR_DDC_IN_R8 || cfg->in_fmt > SDR_DDC_IN_CI16) return sdr_fail(SDR_ERR_INVALID, "unknown input format %d", cfg->in_fmt);
    if (!rs_valid(L, M, T))
        return sdr_fail(SDR_ERR_INVALID, "interpolation %d (1..%d), decimation %d (1..%d, at most %d L) or %d taps (1..%d, at most %d per phase) out of range",
                        L, kRsMaxInterpolation, M, kRsMaxDecimation, kRsMaxRatio, T, kRsMaxTaps, kRsMaxPhaseTaps);
    if (cfg->flags) return sdr_fail(SDR_ERR_INVALID, "unknown flags 0x%x", cfg->flags);
    if (!cfg->taps) return sdr_fail(SDR_ERR_INVALID, "taps is NULL");
    if (!std::isfinite(cfg->gain)) return sdr_fail(SDR_ERR_INVALID, "gain is not finite");
    for (int k = 0; k < T; ++k)
        if (!std::isfinite(cfg->taps[k])) return sdr_fail(SDR_ERR_INVALID, "tap %d is not finite", k);
    sdr_ddc* d = new (std::nothrow) sdr_ddc();
    if (!d) return sdr_fail(SDR_ERR_NOMEM, "host allocation failed");
    d->engine = e, d->in_fmt = cfg->in_fmt, d->D = M, d->T = T, d->fcw = cfg->fcw, d->gain = cfg->gain, d->L = L;
    const RsPush shape = rs_push(0, 0, L, M, T);
    d->Tp = shape.Tp;
    std::vector<double> table((size_t)shape.Tp * shape.Lp);
    for (int k = 0; k < shape.Tp; ++k)
        for (int r = 0; r < shape.Lp; ++r) {
            const int at = rs_table_tap(L, M, T, k, r);
            table[(size_t)k * shape.Lp + r] = at >= 0 ? cfg->taps[at] : 0.0;
        }
    const size_t hist_bytes = (size_t)(d->Tp > 1 ? d->Tp - 1 : 1) * ddc_in_bytes(d->in_fmt);
    hipError_t err = hipMalloc((void**)&d->taps, table.size() * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&d->hist, hist_bytes);
    if (err == hipSuccess) err = hipMemcpyAsync(d->taps, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipMemsetAsync(d->hist, 0, hist_bytes, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);     // (the table is the host's again)
    if (err != hipSuccess) {
        if (d->taps) (void)hipFree(d->taps);
        if (d->hist) (void)hipFree(d->hist);
        delete d;
        return sdr_fail(SDR_ERR_HIP, "sdr_ddc_create_rational: %s", hipGetErrorString(err));
    }
    *out = d;
    return SDR_OK;
}
