// Digital down-converter between the host's slab and the ring (sdr_ddc_*): mixer, FIR low-pass, decimator.  Real or complex
// recordings at an intermediate frequency and wide-band recordings are converted where they enter the ring; nothing
// downstream of the ring knows.  What the ring must hold is stated in include/sydr_amd.h and, as NumPy, in
// sydr_amd/signal/downconvert.py: the phasor is a pure function of the absolute input index, every output is the same T
// products added in the same order whatever tile or push it falls into -- so the ring does not depend on how the stream was
// cut into pushes, bit for bit.
// A converter with a mitigator attached (sdr_ddc_mitigate: pulse blanker, narrow-band excisor -- mitigate.hip) has the same
// ddc_kernel write its outputs as cf64 into the mitigator's work buffer in place of the ring; without one a push makes the
// launches it always made.
// A converter made by sdr_ddc_create_rational with interpolation L > 1 keeps its handle here and its kernels in resample.hip.
// A converter made by sdr_ddc_create_array (ddc_array.hip) runs the same kernels with a third loader, DdcArrayLoad, one made by
// sdr_ddc_create_stap (ddc_stap.hip) with a fourth, DdcStapLoad.
#include "engine_internal.h"
#include "ddc_handle.h"
#include "ddc_tiles.h"
#include "mitigate.h"
#include "resample_tiles.h"
#include "sincos_reduced.h"

#include <cmath>
#include <new>

using namespace sdr;

// One workgroup per tile of outputs (ddc_tiles.h).  Phase 1: the tile's inputs, each mixed once, into LDS as fp64 complex.
// Phase 2: a lane per output, the taps by wave-uniform (scalar) loads, k ascending, product then sum (no contraction: the
// NumPy statement's own operations); the store in the ring's format, a ci8 ring's bytes sign-flipped.
// `load` reads an input of the push's block or of the history: one of the four formats (ddc_kernel), or a layout's frames,
// decoded here and nowhere else (ddc_layout_kernel).
template <class Load>
__device__ __forceinline__ void ddc_kernel_body(double2* z, const void* __restrict__ in, const void* __restrict__ hist,
                                                const double* __restrict__ taps, void* __restrict__ ring, const DdcPush& push, int tile,
                                                const Load& load, int out_fmt, uint64_t fcw, double gain, int64_t ring_offset,
                                                int64_t capacity) {
    const DdcTile t = ddc_tile(push, tile, blockIdx.x);
    for (int i = threadIdx.x; i < t.span; i += kDdcThreads) {
        const int64_t j = t.j0 + i;
        const int64_t src = ddc_source(push, j);
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
    const int T = push.T, D = push.D;
    for (int o = threadIdx.x; o < t.count; o += kDdcThreads) {
        const double2* zo = z + (o * D + (T - 1));
        double ar = 0.0, ai = 0.0;
        for (int k = 0; k < T; ++k) {
            const double h = taps[k];
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

__global__ __launch_bounds__(kDdcThreads) void ddc_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                          const double* __restrict__ taps, void* __restrict__ ring, DdcPush push, int tile,
                                                          int in_fmt, int out_fmt, uint64_t fcw, double gain, int64_t ring_offset,
                                                          int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char ddc_smem[];
    ddc_kernel_body((double2*)ddc_smem, in, hist, taps, ring, push, tile, DdcFormatLoad{in_fmt}, out_fmt, fcw, gain, ring_offset, capacity);
}

// The same kernel over a converter with an input layout (sdr_ddc_create_layout): `in` is the recording's bytes as they are.
__global__ __launch_bounds__(kDdcThreads) void ddc_layout_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                                 const double* __restrict__ taps, void* __restrict__ ring, DdcPush push,
                                                                 int tile, DdcLayout lay, int out_fmt, uint64_t fcw, double gain,
                                                                 int64_t ring_offset, int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char ddc_smem[];
    ddc_kernel_body((double2*)ddc_smem, in, hist, taps, ring, push, tile, DdcLayoutLoad{lay, ddc_layout_history(lay)}, out_fmt, fcw, gain,
                    ring_offset, capacity);
}

// The same kernel over a converter with an array (sdr_ddc_create_array): the K elements of every frame combined where it is loaded.
__global__ __launch_bounds__(kDdcThreads) void ddc_array_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                                const double* __restrict__ taps, void* __restrict__ ring, DdcPush push,
                                                                int tile, DdcLayout lay, DdcArray arr, int out_fmt, uint64_t fcw, double gain,
                                                                int64_t ring_offset, int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char ddc_smem[];
    ddc_kernel_body((double2*)ddc_smem, in, hist, taps, ring, push, tile, DdcArrayLoad{lay, arr}, out_fmt, fcw, gain, ring_offset, capacity);
}

// The same kernel over a converter with space-time weights (sdr_ddc_create_stap): T frames of K elements combined per input.
__global__ __launch_bounds__(kDdcThreads) void ddc_stap_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                               const double* __restrict__ tail, const double* __restrict__ taps,
                                                               void* __restrict__ ring, DdcPush push, int tile, DdcLayout lay, DdcArray arr,
                                                               DdcStap stap, int out_fmt, uint64_t fcw, double gain, int64_t ring_offset,
                                                               int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char ddc_smem[];
    ddc_kernel_body((double2*)ddc_smem, in, hist, taps, ring, push, tile, DdcStapLoad{lay, arr, stap, tail}, out_fmt, fcw, gain, ring_offset,
                    capacity);
}

// The history after a push: one workgroup, every lane reads its element (out of the block, or -- a push shorter than T-1 --
// further up the old history) before any lane writes.  `unit` = bytes per raw input.
__global__ __launch_bounds__(kDdcMaxTaps) void ddc_history_kernel(const void* __restrict__ in, void* hist, int64_t n_in, int T, int unit) {
    const int i = threadIdx.x;
    uint32_t v = 0;
    if (i < T - 1) {
        const int64_t src = ddc_hist_source(n_in, T, i);
        const void* from = src >= 0 ? in : (const void*)hist;
        const int64_t at = src >= 0 ? src : ~src;
        v = unit == 1 ? ((const uint8_t*)from)[at] : unit == 2 ? ((const uint16_t*)from)[at] : ((const uint32_t*)from)[at];
    }
    __syncthreads();
    if (i < T - 1) {
        if (unit == 1) ((uint8_t*)hist)[i] = (uint8_t)v;
        else if (unit == 2) ((uint16_t*)hist)[i] = (uint16_t)v;
        else ((uint32_t*)hist)[i] = v;
    }
}

// The same for a converter with an input layout: an element out of the block is decoded, one out of the old history is read as
// the history holds it; both are stored decoded.
__global__ __launch_bounds__(kDdcMaxTaps) void ddc_layout_history_kernel(const void* __restrict__ in, void* hist, int64_t n_in, int T, DdcLayout lay) {
    const int i = threadIdx.x;
    const DdcLayout h = ddc_layout_history(lay);
    double re = 0.0, im = 0.0;
    if (i < T - 1) {
        const int64_t src = ddc_hist_source(n_in, T, i);
        if (src >= 0) ddc_layout_load(in, src, lay, &re, &im);
        else ddc_layout_load((const void*)hist, ~src, h, &re, &im);
    }
    __syncthreads();
    if (i < T - 1) ddc_layout_history_store(hist, i, h, re, im);
}

// The same for a converter with an array: an element out of the block is combined with the push's weights, one out of the old
// history keeps the value it was combined to; both are stored as cf64.
__global__ __launch_bounds__(kDdcMaxTaps) void ddc_array_history_kernel(const void* __restrict__ in, void* hist, int64_t n_in, int T, DdcLayout lay,
                                                                        DdcArray arr) {
    const int i = threadIdx.x;
    double re = 0.0, im = 0.0;
    if (i < T - 1) {
        const int64_t src = ddc_hist_source(n_in, T, i);
        if (src >= 0) ddc_array_load(in, src, lay, arr, &re, &im);
        else ddc_array_history_load((const void*)hist, ~src, &re, &im);
    }
    __syncthreads();
    if (i < T - 1) ddc_array_history_store(hist, i, re, im);
}

// The same for a converter with space-time weights, and its raw tail: lane i < Tp - 1 takes element i of the history as the
// array's kernel does, lane i < (T - 1) K element i % K of slot i / K of the tail -- out of the block, or, of a push shorter than
// T - 1 frames, further up the old tail (a shift, ddc_stap_tail_next).  Every lane reads before any lane writes.
__global__ __launch_bounds__(kDdcMaxTaps) void ddc_stap_history_kernel(const void* __restrict__ in, void* hist, double* tail, int64_t n_in, int Tp,
                                                                       DdcLayout lay, DdcArray arr, DdcStap stap) {
    const int i = threadIdx.x;
    const int slot = i / arr.K, a = i - slot * arr.K;
    const bool in_tail = i < (stap.T - 1) * arr.K;
    double re = 0.0, im = 0.0, tr = 0.0, ti = 0.0;
    if (i < Tp - 1) {
        const int64_t src = ddc_hist_source(n_in, Tp, i);
        if (src >= 0) ddc_stap_load(in, tail, src, lay, arr, stap, &re, &im);
        else ddc_array_history_load((const void*)hist, ~src, &re, &im);
    }
    if (in_tail) ddc_stap_tail_next(in, tail, n_in, lay, arr, stap.T, slot, a, &tr, &ti);
    __syncthreads();
    if (i < Tp - 1) ddc_array_history_store(hist, i, re, im);
    if (in_tail) ddc_stap_tail_store(tail, slot, arr.K, a, tr, ti);
}

void sdr::ddc_history_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in) {
    ProfScope ps(e, "ddc_history_kernel");
    if (d->has_stap) {
        hipLaunchKernelGGL(ddc_stap_history_kernel, dim3(1), dim3(kDdcMaxTaps), 0, e->stream, (const void*)e->ddc_stage.ptr, d->hist, d->tail, n_in,
                           d->Tp, d->layout, d->array, d->stap);
        return;
    }
    if (d->has_array) {
        hipLaunchKernelGGL(ddc_array_history_kernel, dim3(1), dim3(kDdcMaxTaps), 0, e->stream, (const void*)e->ddc_stage.ptr, d->hist, n_in,
                           d->Tp, d->layout, d->array);
        return;
    }
    if (d->has_layout) {
        hipLaunchKernelGGL(ddc_layout_history_kernel, dim3(1), dim3(kDdcMaxTaps), 0, e->stream, (const void*)e->ddc_stage.ptr, d->hist, n_in,
                           d->Tp, d->layout);
        return;
    }
    hipLaunchKernelGGL(ddc_history_kernel, dim3(1), dim3(kDdcMaxTaps), 0, e->stream, (const void*)e->ddc_stage.ptr, d->hist, n_in, d->Tp,
                       (int)ddc_in_bytes(d->in_fmt));
}

int sdr::ddc_push_bytes(const sdr_ddc* d, int64_t n_in, size_t* bytes) {
    if (!d->has_layout) {
        *bytes = (size_t)n_in * ddc_in_bytes(d->in_fmt);
        return SDR_OK;
    }
    if (n_in > kDdcLayoutMaxFrames) return sdr_fail(SDR_ERR_RANGE, "%lld frames in one push", (long long)n_in);
    const int64_t b = ddc_layout_push_bytes(d->layout, n_in);
    if (b < 0)
        return sdr_fail(SDR_ERR_INVALID, "%lld frames of %d fields of %d bit(s) are not whole bytes", (long long)n_in, d->layout.stride, d->layout.bits);
    *bytes = (size_t)b;
    return SDR_OK;
}

static int ddc_push_impl(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t off, int64_t* n_out, bool wait) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->L != 1) return rs_push_impl(e, d, in, n_in, off, n_out, wait);     // a rational resampler: resample.hip
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (n_in < 0) return sdr_fail(SDR_ERR_INVALID, "negative input count");
    if (!in && n_in > 0) return sdr_fail(SDR_ERR_INVALID, "host pointer is NULL");
    const int64_t cap = e->iq_capacity;
    if (off < 0 || off >= cap) return sdr_fail(SDR_ERR_RANGE, "ring offset %lld outside the ring of %lld samples", (long long)off, (long long)cap);
    if (n_in / d->D > cap) return sdr_fail(SDR_ERR_RANGE, "%lld inputs make more outputs than the ring of %lld samples holds", (long long)n_in, (long long)cap);
    const DdcPush push = ddc_push(d->n_seen, n_in, d->D, d->T);
    if (push.n_out > cap)
        return sdr_fail(SDR_ERR_RANGE, "%lld outputs exceed the ring capacity %lld", (long long)push.n_out, (long long)cap);
    size_t bytes = 0;
    if (int rc = ddc_push_bytes(d, n_in, &bytes)) return rc;
    if (n_out) *n_out = push.n_out;
    if (n_in == 0) return SDR_OK;
    ProfScope whole(e, "call_ddc_push");
    // one copy command brings the raw inputs into the engine's staging buffer in HBM (no kernel reads host memory), the
    // kernels follow it on the same stream -- whose order is all the guard the buffer and the history need
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
        const int tile = ddc_tile_outputs(d->D, d->T);
        const int64_t tiles = ddc_tiles(push, tile);
        const size_t lds = (size_t)((tile - 1) * d->D + d->T) * sizeof(double2);
        ProfScope ps(e, "ddc_kernel");
        if (d->has_stap)
            hipLaunchKernelGGL(ddc_stap_kernel, dim3((unsigned)tiles), dim3(kDdcThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->tail, (const double*)d->taps, dst, push, tile, d->layout, d->array, d->stap,
                               dst_fmt, d->fcw, d->gain, dst_off, dst_cap);
        else if (d->has_array)
            hipLaunchKernelGGL(ddc_array_kernel, dim3((unsigned)tiles), dim3(kDdcThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->taps, dst, push, tile, d->layout, d->array, dst_fmt, d->fcw, d->gain, dst_off,
                               dst_cap);
        else if (d->has_layout)
            hipLaunchKernelGGL(ddc_layout_kernel, dim3((unsigned)tiles), dim3(kDdcThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->taps, dst, push, tile, d->layout, dst_fmt, d->fcw, d->gain, dst_off, dst_cap);
        else
            hipLaunchKernelGGL(ddc_kernel, dim3((unsigned)tiles), dim3(kDdcThreads), lds, e->stream, (const void*)e->ddc_stage.ptr,
                               (const void*)d->hist, (const double*)d->taps, dst, push, tile, d->in_fmt, dst_fmt, d->fcw, d->gain, dst_off, dst_cap);
    }
    if (d->mit && push.n_out > 0)
        if (int rc = mit_push_finish(e, d->mit, push.m_first, push.n_out, off)) return rc;
    if (d->has_array) ddc_array_cov_launch(e, d, n_in);
    if (d->T > 1 || (d->has_stap && d->stap.T > 1)) ddc_history_launch(e, d, n_in);     // (a space-time converter's raw tail too)
    SDR_HIP(hipGetLastError());
    d->n_seen += n_in;
    if (wait) SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

extern "C" {

int sdr_ddc_create(sdr_engine* e, const sdr_ddc_cfg* cfg, sdr_ddc** out) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!cfg || !out) return sdr_fail(SDR_ERR_INVALID, "NULL configuration or result pointer");
    *out = nullptr;
    if (cfg->in_fmt < SDR_DDC_IN_R8 || cfg->in_fmt > SDR_DDC_IN_CI16) return sdr_fail(SDR_ERR_INVALID, "unknown input format %d", cfg->in_fmt);
    if (cfg->decimation < 1 || cfg->decimation > kDdcMaxDecimation)
        return sdr_fail(SDR_ERR_INVALID, "decimation %d outside 1..%d", cfg->decimation, kDdcMaxDecimation);
    if (cfg->n_taps < 1 || cfg->n_taps > kDdcMaxTaps) return sdr_fail(SDR_ERR_INVALID, "%d taps outside 1..%d", cfg->n_taps, kDdcMaxTaps);
    if (cfg->flags) return sdr_fail(SDR_ERR_INVALID, "unknown flags 0x%x", cfg->flags);
    if (!cfg->taps) return sdr_fail(SDR_ERR_INVALID, "taps is NULL");
    if (!std::isfinite(cfg->gain)) return sdr_fail(SDR_ERR_INVALID, "gain is not finite");
    for (int k = 0; k < cfg->n_taps; ++k)
        if (!std::isfinite(cfg->taps[k])) return sdr_fail(SDR_ERR_INVALID, "tap %d is not finite", k);
    sdr_ddc* d = new (std::nothrow) sdr_ddc();
    if (!d) return sdr_fail(SDR_ERR_NOMEM, "host allocation failed");
    d->engine = e, d->in_fmt = cfg->in_fmt, d->D = cfg->decimation, d->T = cfg->n_taps, d->fcw = cfg->fcw, d->gain = cfg->gain;
    d->Tp = d->T;
    const size_t hist_bytes = (size_t)(d->T > 1 ? d->T - 1 : 1) * ddc_in_bytes(d->in_fmt);
    hipError_t err = hipMalloc((void**)&d->taps, (size_t)d->T * sizeof(double));
    if (err == hipSuccess) err = hipMalloc(&d->hist, hist_bytes);
    if (err == hipSuccess) err = hipMemcpyAsync(d->taps, cfg->taps, (size_t)d->T * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipMemsetAsync(d->hist, 0, hist_bytes, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);     // (cfg->taps is the caller's again)
    if (err != hipSuccess) {
        if (d->taps) (void)hipFree(d->taps);
        if (d->hist) (void)hipFree(d->hist);
        delete d;
        return sdr_fail(SDR_ERR_HIP, "sdr_ddc_create: %s", hipGetErrorString(err));
    }
    *out = d;
    return SDR_OK;
}

static bool layout_of(const sdr_ddc_layout* in, DdcLayout* out) {
    if (!in || !ddc_layout_valid(in->field, in->bits, in->stride, in->lane, in->flags, in->reserved)) return false;
    *out = ddc_layout_make(in->field, in->bits, in->stride, in->lane, in->flags, in->levels);
    return true;
}

int64_t sdr_ddc_layout_bytes(const sdr_ddc_layout* layout, int64_t n_in) {
    DdcLayout lay;
    if (!layout_of(layout, &lay)) return sdr_fail(SDR_ERR_INVALID, "the input layout is NULL or outside its limits");
    if (n_in < 0) return sdr_fail(SDR_ERR_INVALID, "negative input count");
    if (n_in > kDdcLayoutMaxFrames) return sdr_fail(SDR_ERR_RANGE, "%lld frames in one push", (long long)n_in);
    const int64_t b = ddc_layout_push_bytes(lay, n_in);
    if (b < 0) return sdr_fail(SDR_ERR_INVALID, "%lld frames of %d fields of %d bit(s) are not whole bytes", (long long)n_in, lay.stride, lay.bits);
    return b;
}

int sdr_ddc_create_layout(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, const sdr_ddc_layout* layout, sdr_ddc** out) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!cfg || !out) return sdr_fail(SDR_ERR_INVALID, "NULL configuration or result pointer");
    *out = nullptr;
    DdcLayout lay;
    if (!layout_of(layout, &lay)) return sdr_fail(SDR_ERR_INVALID, "the input layout is NULL or outside its limits");
    // the converter itself is sdr_ddc_create_rational's, every check of cfg included (cfg->in_fmt is not read: the layout says
    // what an input is); its history then takes the layout's form
    sdr_ddc_cfg c = *cfg;
    c.in_fmt = SDR_DDC_IN_R8;
    sdr_ddc* d = nullptr;
    if (int rc = sdr_ddc_create_rational(e, &c, interpolation, &d)) return rc;
    d->has_layout = true, d->layout = lay;
    const size_t hist_bytes = (size_t)(d->Tp > 1 ? d->Tp - 1 : 1) * ddc_hist_unit(d);
    void* hist = nullptr;
    hipError_t err = hipMalloc(&hist, hist_bytes);
    if (err == hipSuccess) err = hipMemsetAsync(hist, 0, hist_bytes, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) {
        if (hist) (void)hipFree(hist);
        sdr_ddc_destroy(e, d);
        return sdr_fail(SDR_ERR_HIP, "sdr_ddc_create_layout: %s", hipGetErrorString(err));
    }
    (void)hipFree(d->hist);
    d->hist = hist;
    *out = d;
    return SDR_OK;
}

void sdr_ddc_destroy(sdr_engine* e, sdr_ddc* d) {
    if (!d) return;
    if (e && sdr_set_device(e) == SDR_OK) (void)hipStreamSynchronize(e->stream);     // (a queued push may still read them)
    if (d->taps) (void)hipFree(d->taps);
    if (d->hist) (void)hipFree(d->hist);
    if (d->cov) (void)hipFree(d->cov);
    if (d->cov_slab.ptr) (void)hipFree(d->cov_slab.ptr);
    if (d->tail) (void)hipFree(d->tail);
    mit_destroy(nullptr, d->mit);
    delete d;
}

int sdr_ddc_reset(sdr_engine* e, sdr_ddc* d) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    const size_t hist_bytes = (size_t)(d->Tp > 1 ? d->Tp - 1 : 1) * ddc_hist_unit(d);
    SDR_HIP(hipMemsetAsync(d->hist, 0, hist_bytes, e->stream));
    if (d->cov) SDR_HIP(hipMemsetAsync(d->cov, 0, ddc_cov_bytes(d), e->stream));     // (the weights stay)
    if (d->tail) SDR_HIP(hipMemsetAsync(d->tail, 0, ddc_stap_tail_bytes(d->stap.T, d->array.K), e->stream));
    d->cov_n = 0;
    if (d->mit)
        if (int rc = mit_reset(e, d->mit)) return rc;
    d->n_seen = 0;
    return SDR_OK;
}

int sdr_ddc_push(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t ring_offset, int64_t* n_out) {
    return ddc_push_impl(e, d, in, n_in, ring_offset, n_out, true);
}

int sdr_ddc_push_queue(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t ring_offset, int64_t* n_out) {
    return ddc_push_impl(e, d, in, n_in, ring_offset, n_out, false);
}

int64_t sdr_ddc_out_count(const sdr_ddc* d, int64_t n_in) {
    if (!d) return sdr_fail(SDR_ERR_INVALID, "converter is NULL");
    if (n_in < 0) return sdr_fail(SDR_ERR_INVALID, "negative input count");
    if (d->L != 1) {
        if (!rs_in_range(d->n_seen, n_in, d->L)) return sdr_fail(SDR_ERR_RANGE, "%lld inputs take the up-sampled index past 2^62", (long long)n_in);
        return rs_push(d->n_seen, n_in, d->L, d->D, d->T).n_out;
    }
    return ddc_push(d->n_seen, n_in, d->D, d->T).n_out;
}

int sdr_ddc_mitigate(sdr_engine* e, sdr_ddc* d, const sdr_mit_cfg* cfg) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->n_seen != 0) return sdr_fail(SDR_ERR_STATE, "the converter has seen %lld inputs since its creation or reset", (long long)d->n_seen);
    Mitigator* fresh = nullptr;
    if (cfg)
        if (int rc = mit_create(e, cfg, &fresh)) return rc;
    mit_destroy(e, d->mit);
    d->mit = fresh;
    return SDR_OK;
}

int64_t sdr_ddc_delay(const sdr_ddc* d) {
    if (!d) return sdr_fail(SDR_ERR_INVALID, "converter is NULL");
    return d->mit ? mit_delay_of(d->mit) : 0;
}

int sdr_ddc_mitigation_stats(sdr_engine* e, sdr_ddc* d, sdr_mit_stats* stats, int64_t* bins) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (!stats) return sdr_fail(SDR_ERR_INVALID, "no result block for the counters");
    if (!d->mit) return sdr_fail(SDR_ERR_STATE, "the converter has no mitigator");
    return mit_stats(e, d->mit, ddc_ceil_div(d->n_seen * d->L, d->D), stats, bins);
}

}  // extern "C"
