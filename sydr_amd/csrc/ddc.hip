// Digital down-converter between the host's slab and the ring (sdr_ddc_*): mixer, FIR low-pass, decimator.  Real or complex
// recordings at an intermediate frequency and wide-band recordings are converted where they enter the ring; nothing
// downstream of the ring knows.  What the ring must hold is stated in include/sydr_amd.h and, as NumPy, in
// sydr_amd/signal/downconvert.py: the phasor is a pure function of the absolute input index, every output is the same T
// products added in the same order whatever tile or push it falls into -- so the ring does not depend on how the stream was
// cut into pushes, bit for bit.
// One of everything, for every input form: one converter kernel over (filter, loader), one history kernel over the loader, one
// push, one constructor behind the five sdr_ddc_create*.  The filter is the integer FIR (L = 1; profiler scope "ddc_kernel") or
// the polyphase one of a rational resampler (L > 1; "resample_kernel", resample.hip says what it computes); the loader
// (ddc_handle.h) is picked from the converter's kind in one place: the four raw formats, an input layout, an antenna array
// (ddc_array.hip) or a space-time array (ddc_stap.hip).
// An array or space-time converter with BEAMS attached (sdr_ddc_beam_attach, ddc_beams.hip) runs the same two kernel bodies
// once more with the beam as the grid's second dimension: the staged bytes are decoded again from HBM per beam, combined with
// the beam's weights, and written into the beam's target ring.
// A converter with a mitigator attached (sdr_ddc_mitigate: pulse blanker, narrow-band excisor -- mitigate.hip) has the same
// kernel write its outputs as cf64 into the mitigator's work buffer in place of the ring; without one a push makes the
// launches it always made.
#include "engine_internal.h"
#include "ddc_cov.h"
#include "ddc_handle.h"
#include "ddc_tiles.h"
#include "mitigate.h"
#include "resample_tiles.h"
#include "sincos_reduced.h"

#include <cmath>
#include <new>
#include <vector>

using namespace sdr;

// The two FILTERS of the converter kernel, each a kernel argument by value: a push's geometry (`source`, `tile_of`) and the tap
// loop of one output (`output`) for the device; the range check, the launch's sizes and the profiler's scope for the push.  The
// tap loops are kept apart because they load their taps differently (docs/notes/resample.md).
//
// The integer FIR (L = 1, ddc_tiles.h): the taps by wave-uniform (scalar) loads.
struct DdcFir {
    DdcPush push;
    int tile;
    typedef DdcTile Tile;
    static constexpr const char* kScope = "ddc_kernel";
    static constexpr const char* kBeamScope = "ddc_beam_kernel";
    static int check(const sdr_ddc* d, int64_t n_in, int64_t cap) {
        if (n_in / d->D > cap) return sdr_fail(SDR_ERR_RANGE, "%lld inputs make more outputs than the ring of %lld samples holds", (long long)n_in, (long long)cap);
        return SDR_OK;
    }
    DdcFir(const sdr_ddc* d, int64_t n_in) : push(ddc_push(d->n_seen, n_in, d->D, d->T)), tile(ddc_tile_outputs(d->D, d->T)) {}
    int64_t tiles() const { return ddc_tiles(push, tile); }
    size_t lds_inputs() const { return (size_t)((tile - 1) * push.D + push.T); }
    __device__ __forceinline__ Tile tile_of(int64_t b) const { return ddc_tile(push, tile, b); }
    __device__ __forceinline__ int64_t source(int64_t j) const { return ddc_source(push, j); }
    // k ascending, product then sum (no contraction: the NumPy statement's own operations), then the gain
    __device__ __forceinline__ double2 output(const Tile&, int o, const double2* z, const double* __restrict__ taps, double gain) const {
        const int T = push.T, D = push.D;
        const double2* zo = z + (o * D + (T - 1));
        double ar = 0.0, ai = 0.0;
        for (int k = 0; k < T; ++k) {
            const double h = taps[k];
            const double2 v = zo[-k];
            ar += h * v.x;
            ai += h * v.y;
        }
        ar *= gain, ai *= gain;
        return make_double2(ar, ai);
    }
};

// The polyphase one (L > 1, resample_tiles.h): lanes of consecutive outputs sit on different
// phases, so a lane takes its K_p taps down its column of the table [k][r] by per-lane (vector) loads.
struct DdcPolyphase {
    RsPush push;
    int tile;
    typedef RsTile Tile;
    static constexpr const char* kScope = "resample_kernel";
    static constexpr const char* kBeamScope = "resample_beam_kernel";
    static int check(const sdr_ddc* d, int64_t n_in, int64_t) {
        if (!rs_in_range(d->n_seen, n_in, d->L))
            return sdr_fail(SDR_ERR_RANGE, "%lld inputs behind %lld take the up-sampled index past 2^62", (long long)n_in, (long long)d->n_seen);
        return SDR_OK;
    }
    DdcPolyphase(const sdr_ddc* d, int64_t n_in) : push(rs_push(d->n_seen, n_in, d->L, d->D, d->T)), tile(rs_tile_outputs(d->L, d->D, d->T)) {}
    int64_t tiles() const { return rs_tiles(push, tile); }
    size_t lds_inputs() const { return (size_t)rs_tile_span_max(push.L, push.M, push.T, tile); }
    __device__ __forceinline__ Tile tile_of(int64_t b) const { return rs_tile(push, tile, b); }
    __device__ __forceinline__ int64_t source(int64_t j) const { return rs_source(push, j); }
    // the same operations in the same order
    __device__ __forceinline__ double2 output(const Tile& t, int o, const double2* z, const double* __restrict__ table, double gain) const {
        const int Lp = push.Lp;
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
        return make_double2(ar, ai);
    }
};

static_assert(kRsThreads == kDdcThreads, "one converter kernel: one workgroup size");

// Input j (absolute) of a push, loaded from the block or the history and mixed: the phasor from the absolute index.
template <class Filter, class Load>
__device__ __forceinline__ double2 ddc_mixed_input(const Filter& filter, const Load& load, const void* __restrict__ in, const void* __restrict__ hist,
                                                   int64_t j, uint64_t fcw) {
    const int64_t src = filter.source(j);
    double xr = 0.0, xi = 0.0;
    if (src < 0) load.history(hist, ~src, &xr, &xi);
    else if (src < filter.push.n_in) load.block(in, src, &xr, &xi);
    const uint64_t p = (uint64_t)j * fcw;                       // (j < 0: x = 0 whatever the phasor)
    const double turn = (double)(p >> 11) * 0x1p-53;
    double s, c;
    sincos_reduced(6.283185307179586 * turn, &s, &c);
    return make_double2(xr * c + xi * s, xi * c - xr * s);
}

// THE converter kernel, over (filter, loader).  One workgroup per tile of outputs.  Phase 1: the tile's inputs, each loaded and
// mixed once, into LDS as fp64 complex.  Phase 2: a lane per output, the filter's tap loop, the store.  With a mitigator attached
// `ring` is its linear cf64 work buffer.
// The body is a function of its own for its __restrict__ parameters: inlined, they tell the compiler that a store into z cannot
// reach what `load` is read from, so a layout's level words and an array's lanes are read once at the kernel's entry; written
// straight into the kernel the same statements re-read them from the argument segment at every use (docs/notes/downconvert.md).
template <class Filter, class Load>
__device__ __forceinline__ void ddc_convert_body(double2* z, const void* __restrict__ in, const void* __restrict__ hist, const double* __restrict__ taps,
                                                 void* __restrict__ ring, const Filter& filter, const Load& load, int out_fmt, uint64_t fcw, double gain,
                                                 int64_t ring_offset, int64_t capacity) {
    const typename Filter::Tile t = filter.tile_of(blockIdx.x);
    for (int i = threadIdx.x; i < t.span; i += kDdcThreads) z[i] = ddc_mixed_input(filter, load, in, hist, t.j0 + i, fcw);
    __syncthreads();
    for (int o = threadIdx.x; o < t.count; o += kDdcThreads) {
        const double2 a = filter.output(t, o, z, taps, gain);
        ring_write(ring, out_fmt, ddc_ring_pos(ring_offset, t.i0 + o, capacity), a.x, a.y);   // (the ring, or the mitigator's work buffer)
    }
}

template <class Filter, class Load>
__global__ __launch_bounds__(kDdcThreads) void ddc_convert_kernel(const void* __restrict__ in, const void* __restrict__ hist,
                                                                  const double* __restrict__ taps, void* __restrict__ ring, Filter filter, Load load,
                                                                  int out_fmt, uint64_t fcw, double gain, int64_t ring_offset, int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char ddc_smem[];
    ddc_convert_body((double2*)ddc_smem, in, hist, taps, ring, filter, load, out_fmt, fcw, gain, ring_offset, capacity);
}

// The attached beams of a push in one launch: workgroup (x, b) is tile x of beam b + 1 -- the body above with that beam's weights
// (a row of the table in device memory), history, ring and ring format.
template <class Filter, class Load>
__global__ __launch_bounds__(kDdcThreads) void ddc_beam_kernel(const void* __restrict__ in, const double* __restrict__ taps, Filter filter, Load load,
                                                               DdcBeamDst dst, uint64_t fcw, double gain, int64_t ring_offset, int64_t capacity) {
    extern __shared__ __attribute__((aligned(16))) char ddc_smem[];
    const int b = blockIdx.y;
    ddc_convert_body((double2*)ddc_smem, in, (const void*)dst.hist[b], taps, dst.ring[b], filter, load.beam(b), dst.fmt[b], fcw, gain, ring_offset,
                     capacity);
}

// THE history kernel, over the loader: the history after a push is its last Tp - 1 inputs as the loader keeps them.  One
// workgroup; every lane reads its element (out of the block, or -- a push shorter than Tp - 1 -- further up the old history)
// before any lane writes; a loader with a raw tail brings that up to date the same way.
template <class Load>
__device__ __forceinline__ void ddc_history_body(const void* __restrict__ in, void* hist, int64_t n_in, int Tp, const Load& load) {
    const int i = threadIdx.x;
    typename Load::Kept v = {};
    double2 tv = {};
    if (i < Tp - 1) {
        const int64_t src = ddc_hist_source(n_in, Tp, i);
        if (src >= 0) v = load.kept_block(in, src);
        else v = load.kept_history((const void*)hist, ~src);
    }
    if constexpr (Load::kTail) tv = load.tail_next(in, n_in, i);
    __syncthreads();
    if (i < Tp - 1) load.keep(hist, i, v);
    if constexpr (Load::kTail) load.tail_keep(i, tv);
}

template <class Load>
__global__ __launch_bounds__(kDdcMaxTaps) void ddc_history_kernel(const void* __restrict__ in, void* hist, int64_t n_in, int Tp, Load load) {
    ddc_history_body(in, hist, n_in, Tp, load);
}

// ... and the attached beams' histories: workgroup (0, b) is beam b + 1.
template <class Load>
__global__ __launch_bounds__(kDdcMaxTaps) void ddc_beam_history_kernel(const void* __restrict__ in, DdcBeamDst dst, int64_t n_in, int Tp, Load load) {
    ddc_history_body(in, dst.hist[blockIdx.y], n_in, Tp, load.beam(blockIdx.y));
}

// The bytes a push of n_in >= 0 inputs copies to the staging buffer; of a converter with a layout SDR_ERR_INVALID when they are
// not whole (nothing has changed then).
static int ddc_push_bytes(const sdr_ddc* d, int64_t n_in, size_t* bytes) {
    if (d->kind == kDdcKindFormat) {
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

// THE push, of either filter.
template <class Filter>
static int ddc_push_impl(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t off, int64_t* n_out, bool wait) {
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (n_in < 0) return sdr_fail(SDR_ERR_INVALID, "negative input count");
    if (!in && n_in > 0) return sdr_fail(SDR_ERR_INVALID, "host pointer is NULL");
    const int64_t cap = e->iq_capacity;
    for (const DdcBeam& b : d->beams)
        if (!b.target->iq || b.target->iq_capacity != cap)
            return sdr_fail(SDR_ERR_STATE, "an attached beam's ring is gone or no longer holds the %lld samples of the converter's", (long long)cap);
    if (off < 0 || off >= cap) return sdr_fail(SDR_ERR_RANGE, "ring offset %lld outside the ring of %lld samples", (long long)off, (long long)cap);
    if (int rc = Filter::check(d, n_in, cap)) return rc;
    const Filter filter(d, n_in);
    const int64_t n = filter.push.n_out, m_first = filter.push.m_first;
    if (n > cap) return sdr_fail(SDR_ERR_RANGE, "%lld outputs exceed the ring capacity %lld", (long long)n, (long long)cap);
    size_t bytes = 0;
    if (int rc = ddc_push_bytes(d, n_in, &bytes)) return rc;
    if (n_out) *n_out = n;
    if (n_in == 0) return SDR_OK;
    ProfScope whole(e, "call_ddc_push");
    // one copy command brings the raw inputs into the engine's staging buffer in HBM (no kernel reads host memory), the
    // kernels follow it on the same stream -- whose order is all the guard the buffer and the history need
    if (int rc = sdr_devbuf_reserve(e, &e->ddc_stage, bytes)) return rc;
    if (int rc = ddc_cov_reserve(e, d, n_in)) return rc;
    // with a mitigator the kernel's destination is its linear cf64 work buffer, the first output behind the kept state
    void* dst = e->iq;
    int dst_fmt = e->iq_fmt;
    int64_t dst_off = off, dst_cap = cap;
    if (d->mit && n > 0) {
        if (int rc = mit_push_begin(e, d->mit, m_first, n, &dst, &dst_off, &dst_cap)) return rc;
        dst_fmt = SDR_FMT_CF64;
    }
    SDR_HIP(hipMemcpyAsync(e->ddc_stage.ptr, in, bytes, hipMemcpyHostToDevice, e->stream));
    const void* staged = (const void*)e->ddc_stage.ptr;
    const unsigned n_beams = (unsigned)d->beams.size();
    DdcBeamDst beam_dst = {};
    for (unsigned b = 0; b < n_beams; ++b)
        beam_dst.ring[b] = d->beams[b].target->iq, beam_dst.hist[b] = d->beams[b].hist, beam_dst.fmt[b] = d->beams[b].target->iq_fmt;
    if (n > 0) {
        sdr_iq_mark_written(e, off, n);
        ProfScope ps(e, Filter::kScope);
        ddc_with_loader(d, [&](auto load) {
            hipLaunchKernelGGL((ddc_convert_kernel<Filter, decltype(load)>), dim3((unsigned)filter.tiles()), dim3(kDdcThreads),
                               filter.lds_inputs() * sizeof(double2), e->stream, staged, (const void*)d->hist, (const double*)d->taps, dst, filter, load,
                               dst_fmt, d->fcw, d->gain, dst_off, dst_cap);
        });
    }
    if (d->mit && n > 0)
        if (int rc = mit_push_finish(e, d->mit, m_first, n, off)) return rc;
    if (n_beams && n > 0) {
        // every beam's ring behind what its engine has queued on it, the beams' kernels, and the targets' streams behind those
        for (const DdcBeam& b : d->beams) {
            SDR_HIP(hipEventRecord(b.ready, b.target->stream));
            SDR_HIP(hipStreamWaitEvent(e->stream, b.ready, 0));
        }
        {
            ProfScope ps(e, Filter::kBeamScope);
            ddc_with_beam_loader(d, [&](auto load) {
                hipLaunchKernelGGL((ddc_beam_kernel<Filter, decltype(load)>), dim3((unsigned)filter.tiles(), n_beams), dim3(kDdcThreads),
                                   filter.lds_inputs() * sizeof(double2), e->stream, staged, (const double*)d->taps, filter, load, beam_dst, d->fcw, d->gain,
                                   off, cap);
            });
        }
        SDR_HIP(hipEventRecord(d->beams_done, e->stream));
        for (const DdcBeam& b : d->beams) {
            SDR_HIP(hipStreamWaitEvent(b.target->stream, d->beams_done, 0));
            sdr_iq_mark_written(b.target, off, n);
        }
    }
    ddc_cov_launch(e, d, n_in);
    if (d->Tp > 1 || (d->kind == kDdcKindStap && d->stap.T > 1)) {     // (a space-time converter's raw tail too)
        ProfScope ps(e, "ddc_history_kernel");
        // (the beams' histories first: their last inputs reach into the raw tail as it was before this push)
        if (n_beams && d->Tp > 1)
            ddc_with_beam_loader(d, [&](auto load) {
                hipLaunchKernelGGL((ddc_beam_history_kernel<decltype(load)>), dim3(1, n_beams), dim3(kDdcMaxTaps), 0, e->stream, staged, beam_dst, n_in, d->Tp,
                                   load);
            });
        ddc_with_loader(d, [&](auto load) {
            hipLaunchKernelGGL((ddc_history_kernel<decltype(load)>), dim3(1), dim3(kDdcMaxTaps), 0, e->stream, staged, d->hist, n_in, d->Tp, load);
        });
    }
    SDR_HIP(hipGetLastError());
    d->n_seen += n_in;
    if (wait) SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

static int ddc_push_any(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t off, int64_t* n_out, bool wait) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    // (what the push does for its own engine it does for every beam's: a resident tick server leaves, a parked slab goes into the ring)
    for (const DdcBeam& b : d->beams)
        if (int rc = sdr_set_device(b.target)) return rc;
    return d->L == 1 ? ddc_push_impl<DdcFir>(e, d, in, n_in, off, n_out, wait) : ddc_push_impl<DdcPolyphase>(e, d, in, n_in, off, n_out, wait);
}

static bool layout_of(const sdr_ddc_layout* in, DdcLayout* out) {
    if (!in || !ddc_layout_valid(in->field, in->bits, in->stride, in->lane, in->flags, in->reserved)) return false;
    *out = ddc_layout_make(in->field, in->bits, in->stride, in->lane, in->flags, in->levels);
    return true;
}

static void ddc_free(sdr_ddc* d) {
    if (d->taps) (void)hipFree(d->taps);
    if (d->hist) (void)hipFree(d->hist);
    if (d->cov) (void)hipFree(d->cov);
    if (d->cov_slab.ptr) (void)hipFree(d->cov_slab.ptr);
    if (d->tail) (void)hipFree(d->tail);
    ddc_beams_release(d);
    mit_destroy(nullptr, d->mit);
    delete d;
}

// Checked outermost part first: the space-time weights, the array, the layout, then cfg (cfg->in_fmt only of a converter without
// a layout, whose inputs it describes).  Every device buffer is allocated once, at its size, and zeroed; one wait.
int sdr::ddc_create(sdr_engine* e, DdcKind kind, const sdr_ddc_cfg* cfg, int L, const sdr_ddc_layout* layout, const sdr_ddc_array* array, int stap_taps,
                    const double* stap_w, sdr_ddc** out) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!cfg || !out) return sdr_fail(SDR_ERR_INVALID, "NULL configuration or result pointer");
    *out = nullptr;
    DdcLayout lay = {};
    if (kind >= kDdcKindArray) {
        if (!layout || !array) return sdr_fail(SDR_ERR_INVALID, "NULL layout or array");
        const int K = array->n_elements;
        if (kind == kDdcKindStap) {
            if (!ddc_stap_taps_valid(stap_taps))
                return sdr_fail(SDR_ERR_INVALID, "%d taps per element outside %d..%d", stap_taps, kDdcStapMinTaps, kDdcStapMaxTaps);
            if (!stap_w) return sdr_fail(SDR_ERR_INVALID, "weights is NULL");
            if (K < kDdcArrayMin || K > kDdcArrayMax) return sdr_fail(SDR_ERR_INVALID, "%d elements outside %d..%d", K, kDdcArrayMin, kDdcArrayMax);
            if (!ddc_stap_weights_valid(stap_taps, K, stap_w)) return sdr_fail(SDR_ERR_INVALID, "a weight is not finite");
        }
        // the frame is the layout's; its own lane is not read (every element brings one)
        sdr_ddc_layout frame = *layout;
        frame.lane = 0;
        if (!layout_of(&frame, &lay)) return sdr_fail(SDR_ERR_INVALID, "the input layout is outside its limits");
        if (!ddc_array_lanes_valid(lay, K, array->flags, array->lanes))
            return sdr_fail(SDR_ERR_INVALID, "%d elements outside %d..%d, unknown flags 0x%x, or a repeated or out-of-frame lane", K, kDdcArrayMin,
                            kDdcArrayMax, array->flags);
        if (kind == kDdcKindArray && !ddc_array_weights_valid(K, &array->weights[0][0])) return sdr_fail(SDR_ERR_INVALID, "a weight is not finite");
    } else if (kind == kDdcKindLayout) {
        if (!layout_of(layout, &lay)) return sdr_fail(SDR_ERR_INVALID, "the input layout is NULL or outside its limits");
    }
    const int in_fmt = kind == kDdcKindFormat ? cfg->in_fmt : SDR_DDC_IN_R8, M = cfg->decimation, T = cfg->n_taps;
    if (in_fmt < SDR_DDC_IN_R8 || in_fmt > SDR_DDC_IN_CI16) return sdr_fail(SDR_ERR_INVALID, "unknown input format %d", in_fmt);
    if (L == 1) {     // the integer converter's limits ...
        if (M < 1 || M > kDdcMaxDecimation) return sdr_fail(SDR_ERR_INVALID, "decimation %d outside 1..%d", M, kDdcMaxDecimation);
        if (T < 1 || T > kDdcMaxTaps) return sdr_fail(SDR_ERR_INVALID, "%d taps outside 1..%d", T, kDdcMaxTaps);
    } else if (!rs_valid(L, M, T)) {     // ... or the resampler's
        return sdr_fail(SDR_ERR_INVALID, "interpolation %d (1..%d), decimation %d (1..%d, at most %d L) or %d taps (1..%d, at most %d per phase) out of range",
                        L, kRsMaxInterpolation, M, kRsMaxDecimation, kRsMaxRatio, T, kRsMaxTaps, kRsMaxPhaseTaps);
    }
    if (cfg->flags) return sdr_fail(SDR_ERR_INVALID, "unknown flags 0x%x", cfg->flags);
    if (!cfg->taps) return sdr_fail(SDR_ERR_INVALID, "taps is NULL");
    if (!std::isfinite(cfg->gain)) return sdr_fail(SDR_ERR_INVALID, "gain is not finite");
    for (int k = 0; k < T; ++k)
        if (!std::isfinite(cfg->taps[k])) return sdr_fail(SDR_ERR_INVALID, "tap %d is not finite", k);

    sdr_ddc* d = new (std::nothrow) sdr_ddc();
    if (!d) return sdr_fail(SDR_ERR_NOMEM, "host allocation failed");
    d->engine = e, d->kind = kind, d->in_fmt = in_fmt, d->D = M, d->T = T, d->fcw = cfg->fcw, d->gain = cfg->gain, d->L = L;
    d->Tp = rs_phase_taps(L, T);
    d->layout = lay;
    if (kind >= kDdcKindArray) {
        // (a space-time converter's array weights are tap 0's; no kernel of it reads them)
        const double* w = kind == kDdcKindStap ? stap_w : &array->weights[0][0];
        d->array.K = array->n_elements, d->array.flags = array->flags;
        for (int a = 0; a < d->array.K; ++a) d->array.lanes[a] = array->lanes[a], d->array.w[a][0] = w[2 * a], d->array.w[a][1] = w[2 * a + 1];
    }
    if (kind == kDdcKindStap) ddc_stap_set(&d->stap, stap_taps, d->array.K, stap_w);
    // the taps as the device holds them: the T taps, or (L > 1) the table [Tp][L'] of resample_tiles.h
    std::vector<double> table;
    const double* taps = cfg->taps;
    size_t n_taps = (size_t)T;
    if (L != 1) {
        const int Lp = L / rs_gcd(L, M);
        table.resize((size_t)d->Tp * Lp);
        for (int k = 0; k < d->Tp; ++k)
            for (int r = 0; r < Lp; ++r) {
                const int at = rs_table_tap(L, M, T, k, r);
                table[(size_t)k * Lp + r] = at >= 0 ? cfg->taps[at] : 0.0;
            }
        taps = table.data(), n_taps = table.size();
    }
    hipError_t err = hipMalloc((void**)&d->taps, n_taps * sizeof(double));
    auto zeroed = [&](void** p, size_t bytes) {
        if (err == hipSuccess) err = hipMalloc(p, bytes);
        if (err == hipSuccess) err = hipMemsetAsync(*p, 0, bytes, e->stream);
    };
    zeroed(&d->hist, ddc_hist_bytes(d));
    if (kind >= kDdcKindArray && (array->flags & kDdcArrayMeasure)) zeroed(&d->cov, ddc_cov_bytes(d));
    if (kind == kDdcKindStap) zeroed((void**)&d->tail, ddc_stap_tail_bytes(stap_taps, d->array.K));
    if (err == hipSuccess) err = hipMemcpyAsync(d->taps, taps, n_taps * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);     // (the taps are the caller's again)
    if (err != hipSuccess) {
        ddc_free(d);
        return sdr_fail(SDR_ERR_HIP, "sdr_ddc_create: %s", hipGetErrorString(err));
    }
    *out = d;
    return SDR_OK;
}

extern "C" {

int sdr_ddc_create(sdr_engine* e, const sdr_ddc_cfg* cfg, sdr_ddc** out) { return ddc_create(e, kDdcKindFormat, cfg, 1, nullptr, nullptr, 0, nullptr, out); }

int sdr_ddc_create_layout(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, const sdr_ddc_layout* layout, sdr_ddc** out) {
    return ddc_create(e, kDdcKindLayout, cfg, interpolation, layout, nullptr, 0, nullptr, out);
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

void sdr_ddc_destroy(sdr_engine* e, sdr_ddc* d) {
    if (!d) return;
    if (e && sdr_set_device(e) == SDR_OK) (void)hipStreamSynchronize(e->stream);     // (a queued push may still read them)
    ddc_free(d);
}

int sdr_ddc_reset(sdr_engine* e, sdr_ddc* d) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    SDR_HIP(hipMemsetAsync(d->hist, 0, ddc_hist_bytes(d), e->stream));
    if (d->cov) SDR_HIP(hipMemsetAsync(d->cov, 0, ddc_cov_bytes(d), e->stream));     // (the weights stay)
    if (d->tail) SDR_HIP(hipMemsetAsync(d->tail, 0, ddc_stap_tail_bytes(d->stap.T, d->array.K), e->stream));
    for (const DdcBeam& b : d->beams) SDR_HIP(hipMemsetAsync(b.hist, 0, ddc_hist_bytes(d), e->stream));     // (every beam's weights stay)
    d->cov_n = 0;
    if (d->mit)
        if (int rc = mit_reset(e, d->mit)) return rc;
    d->n_seen = 0;
    return SDR_OK;
}

int sdr_ddc_push(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t ring_offset, int64_t* n_out) {
    return ddc_push_any(e, d, in, n_in, ring_offset, n_out, true);
}

int sdr_ddc_push_queue(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t ring_offset, int64_t* n_out) {
    return ddc_push_any(e, d, in, n_in, ring_offset, n_out, false);
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
    if (cfg && !d->beams.empty())
        return sdr_fail(SDR_ERR_UNSUPPORTED, "the converter has beams attached: a mitigator's state is per stream, and there is one mitigator");
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
