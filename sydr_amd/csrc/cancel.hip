// Successive interference cancellation on the ring (sdr_iq_cancel, include/sydr_amd.h): the replicas of up to 64 tracked
// signals -- per epoch an sdr_epl_item and a complex amplitude -- subtracted from a window of the ring in one streaming pass,
// in place or into another engine's ring.  The NumPy statement is sydr_amd/signal/cancel.py.
//
// One workgroup of 256 lanes per tile of 256 granules of the SOURCE ring; a lane owns one 16-byte granule (8 ci8 samples,
// 4 ci16, 2 cf32, 1 cf64: probe_window.h numbers the granules of a window that may cross the ring's end and says which of a
// granule's samples belong to it).  It loads its granule once with one 16-byte load, widens the samples to fp64 in
// registers, subtracts channel after channel in the statement's order and stores the granule: one 16-byte store where the
// whole granule belongs to the window and lands on a granule of the destination (always, in place, away from the window's
// two ragged ends), else sample by sample -- never a sample outside the window.  Every output sample is written by exactly
// one lane, which has read its own input before: in place is safe, no atomics touch the samples, two identical calls
// return identical bits.
// Per (tile, channel) one lane finds, by binary search over `off + n` of the channel's dense item list (cancel_plan.h), the
// first epoch that reaches into the tile and leaves its number in LDS; the lanes walk forward from there.  At receiver
// rates a tile sits inside one epoch and the walk is wave-uniform; epochs shorter than a tile, or than a lane's granule,
// are served by the same walk.
// Per covered sample and channel, the statement's operations in its order (no contraction): t = i / fs, theta = -(w * t) +
// rem_carrier, sincos_reduced, the chip index ceil(i * step + shift) of corr_bounds.h (modulo L in integers, advanced
// from the lane's previous sample of the same epoch), four multiplies and two add/subs, the subtraction.
// The counters are integers, added per workgroup and once per workgroup into the result: their order is free.
#include <algorithm>
#include <cmath>

#include "cancel_plan.h"
#include "corr_bounds.h"
#include "correlator.h"
#include "probe_window.h"

#pragma clang fp contract(off)

namespace {

using namespace sdr;

constexpr int kThreads = 256;

struct CancelArgs {
    const void* src;                 // (may be dst: no __restrict__)
    void* dst;
    int64_t src_cap, dst_cap;
    int64_t base, dst_base;          // ring index of the window's first sample in either ring, inside the ring
    ProbeWindow win;                 // the window's granules in the source ring
    const CancelItemDev* items;      // [n_ch][n_epochs]
    const int32_t* count;            // [n_ch]
    int n_ch, n_epochs;
    const int8_t* codes;
    int code_stride;
    int in_place;
    double fs;
    unsigned long long* stats;       // [2]: samples changed, components clipped
};

// sample j of a granule's four words, widened
template <int FMT>
__device__ __forceinline__ void sample_get(const uint32_t (&w)[4], int j, double& xr, double& xi) {
    if (FMT == SDR_FMT_CI8) {
        const int v = ci8_native((int)w[j >> 1]) >> (16 * (j & 1));
        xr = (double)(int)(int8_t)v;
        xi = (double)(int)(int8_t)(v >> 8);
    } else if (FMT == SDR_FMT_CI16) {
        xr = (double)(int)(int16_t)w[j];
        xi = (double)((int)w[j] >> 16);
    } else if (FMT == SDR_FMT_CF32) {
        xr = (double)__uint_as_float(w[2 * j]);
        xi = (double)__uint_as_float(w[2 * j + 1]);
    } else {
        xr = __hiloint2double((int)w[1], (int)w[0]);
        xi = __hiloint2double((int)w[3], (int)w[2]);
    }
}

// ring_format.h clip_rint, counting the components that the rails change
__device__ __forceinline__ int quantise(double v, double lim, unsigned& clipped) {
    const double r = rint(v);
    clipped += fabs(r) > lim ? 1u : 0u;
    return (int)fmin(fmax(r, -lim), lim);
}

// ... and back into the granule's words in the ring's format (a ci8 ring's bytes sign-flipped)
template <int FMT>
__device__ __forceinline__ void sample_put(uint32_t (&w)[4], int j, double yr, double yi, unsigned& clipped) {
    if (FMT == SDR_FMT_CI8) {
        constexpr double lim = ring_rail(SDR_FMT_CI8);
        const unsigned re = (unsigned)quantise(yr, lim, clipped) & 0xffu, im = (unsigned)quantise(yi, lim, clipped) & 0xffu;
        const unsigned h = (re | (im << 8)) ^ (kCi8Flip & 0xffffu);
        const int sh = 16 * (j & 1);
        w[j >> 1] = (w[j >> 1] & ~(0xffffu << sh)) | (h << sh);
    } else if (FMT == SDR_FMT_CI16) {
        constexpr double lim = ring_rail(SDR_FMT_CI16);
        const unsigned re = (unsigned)quantise(yr, lim, clipped) & 0xffffu, im = (unsigned)quantise(yi, lim, clipped) & 0xffffu;
        w[j] = re | (im << 16);
    } else if (FMT == SDR_FMT_CF32) {
        w[2 * j] = __float_as_uint((float)yr);
        w[2 * j + 1] = __float_as_uint((float)yi);
    } else {
        w[0] = (uint32_t)__double2loint(yr), w[1] = (uint32_t)__double2hiint(yr);
        w[2] = (uint32_t)__double2loint(yi), w[3] = (uint32_t)__double2hiint(yi);
    }
}

// sample j of the words to ring sample `pos` of dst
template <int FMT>
__device__ __forceinline__ void sample_store(void* dst, int64_t pos, const uint32_t (&w)[4], int j) {
    if (FMT == SDR_FMT_CI8) ((uint16_t*)dst)[pos] = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
    else if (FMT == SDR_FMT_CI16) ((uint32_t*)dst)[pos] = w[j];
    else if (FMT == SDR_FMT_CF32) ((uint2*)dst)[pos] = make_uint2(w[2 * j], w[2 * j + 1]);
    else ((uint4*)dst)[pos] = make_uint4(w[0], w[1], w[2], w[3]);
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void cancel_kernel(const CancelArgs a) {
    constexpr int S = ring_granule_samples(FMT);
    __shared__ int first[SDR_CANCEL_MAX_CHANNELS];   // per channel: the first epoch that reaches into this tile
    __shared__ unsigned red[2][kThreads / 64];
    const int tid = threadIdx.x;
    const int64_t tile0 = (int64_t)blockIdx.x * kThreads;   // (< win.total: the grid is sized by it)

    if (tid < a.n_ch) {
        int64_t lo, hi;
        probe_granule(a.win, tile0, S, &lo, &hi);
        int64_t m_tile = lo - a.base;    // window offset of the tile's first sample
        if (m_tile < 0) m_tile += a.src_cap;
        const CancelItemDev* row = a.items + (size_t)tid * (size_t)a.n_epochs;
        int l = 0, r = a.count[tid];
        while (l < r) {
            const int mid = (l + r) >> 1;
            if (row[mid].off + row[mid].n <= m_tile) l = mid + 1;
            else r = mid;
        }
        first[tid] = l;
    }
    __syncthreads();

    unsigned changed = 0, clipped = 0;
    const int64_t gi = tile0 + tid;
    if (gi < a.win.total) {
        int64_t lo, hi;
        const int64_t g = probe_granule(a.win, gi, S, &lo, &hi);
        const int j0 = (int)(lo - g * S), j1 = (int)(hi - g * S);   // samples [j0, j1) of the granule belong to the window
        int64_t m_lo = lo - a.base;                                 // window offset of sample j0
        if (m_lo < 0) m_lo += a.src_cap;
        const uint4 v = ((const uint4*)a.src)[g];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        double yr[S], yi[S];
#pragma unroll
        for (int j = 0; j < S; ++j) sample_get<FMT>(w, j, yr[j], yi[j]);
        unsigned cov = 0;

        for (int ch = 0; ch < a.n_ch; ++ch) {
            const CancelItemDev* row = a.items + (size_t)ch * (size_t)a.n_epochs;
            const int cnt = a.count[ch];
            int k = first[ch];
            if (k >= cnt) continue;
            CancelItemDev it = row[k];
            if (it.off >= m_lo + (j1 - j0)) continue;   // (the epoch starts behind this granule; so do all later ones)
            const int8_t* chips = a.codes + (size_t)it.slot * (size_t)a.code_stride;
            bool fresh = true;
            int p_prev = 0, q = 0;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (j < j0 || j >= j1) continue;
                const int64_t m = m_lo + (j - j0);
                while (k < cnt && it.off + it.n <= m) {
                    if (++k < cnt) {
                        it = row[k];
                        chips = a.codes + (size_t)it.slot * (size_t)a.code_stride;
                        fresh = true;
                    }
                }
                if (k >= cnt || m < it.off) continue;
                const int i = (int)(m - it.off);
                CorrTap T;
                T.shift = it.shift, T.step = it.step, T.inv_step = 0.0;
                const int p = corr_index(T, i);
                q = fresh ? corr_chip(p, it.L) : corr_chip_advance(q, (unsigned)p - (unsigned)p_prev, it.L);
                fresh = false;
                p_prev = p;
                const double t = (double)i / a.fs;
                const double th = -(it.w * t) + it.rem_carrier;
                double sn, cs;
                sincos_reduced(th, &sn, &cs);
                const double chip = (double)chips[q];
                const double r_re = chip * (it.a_re * cs + it.a_im * sn);
                const double r_im = chip * (it.a_im * cs - it.a_re * sn);
                yr[j] -= r_re;
                yi[j] -= r_im;
                cov |= 1u << j;
            }
        }

        changed = (unsigned)__popc(cov);
#pragma unroll
        for (int j = 0; j < S; ++j)
            if (cov & (1u << j)) sample_put<FMT>(w, j, yr[j], yi[j], clipped);
        if (cov || !a.in_place) {
            int64_t d0 = a.dst_base + m_lo;   // ring sample of dst that takes sample j0
            if (d0 >= a.dst_cap) d0 -= a.dst_cap;
            if (j0 == 0 && j1 == S && d0 % S == 0) {   // (a ring is a whole number of granules: such a store ends inside it)
                ((uint4*)a.dst)[d0 / S] = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    if (j < j0 || j >= j1) continue;
                    if (a.in_place && !(cov & (1u << j))) continue;
                    int64_t d = d0 + (j - j0);
                    if (d >= a.dst_cap) d -= a.dst_cap;
                    sample_store<FMT>(a.dst, d, w, j);
                }
            }
        }
    }

    // the two counters: per wave, per workgroup, once into the result
    for (int d = 32; d > 0; d >>= 1) {
        changed += __shfl_down(changed, d);
        clipped += __shfl_down(clipped, d);
    }
    if ((tid & 63) == 0) red[0][tid >> 6] = changed, red[1][tid >> 6] = clipped;
    __syncthreads();
    if (tid < 2) {
        unsigned long long s = 0;
        for (int k = 0; k < kThreads / 64; ++k) s += red[tid][k];
        if (s) atomicAdd(a.stats + tid, s);
    }
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int sdr_iq_cancel(sdr_engine* e, const sdr_epl_item* items, const double* amps, int n_ch, int n_epochs, double fs,
                  int64_t window_start, int64_t window_samples, sdr_engine* dst, int64_t dst_offset, sdr_cancel_stats* stats) {
    if (!e) return sdr_fail(SDR_ERR_INVALID, "engine is NULL");
    if (!dst) dst = e, dst_offset = window_start;
    if (dst != e)
        if (int rc = sdr_set_device(dst)) return rc;   // (a resident tick server leaves, a parked slab goes into its ring)
    if (int rc = sdr_set_device(e)) return rc;
    if (!e->iq || !dst->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if (!items || !amps) return sdr_fail(SDR_ERR_INVALID, "no items or no amplitudes to cancel");
    if (n_ch < 1 || n_ch > SDR_CANCEL_MAX_CHANNELS)
        return sdr_fail(SDR_ERR_INVALID, "n_ch %d outside 1..%d", n_ch, SDR_CANCEL_MAX_CHANNELS);
    if (n_epochs < 1) return sdr_fail(SDR_ERR_INVALID, "n_epochs %d", n_epochs);
    if (!(fs > 0.0) || !std::isfinite(fs)) return sdr_fail(SDR_ERR_INVALID, "bad sampling frequency");
    if (dst->device != e->device) return sdr_fail(SDR_ERR_INVALID, "the destination engine is on another device");
    if (dst->iq_fmt != e->iq_fmt) return sdr_fail(SDR_ERR_INVALID, "the destination ring has another format");
    if (window_start < 0 || dst_offset < 0) return sdr_fail(SDR_ERR_RANGE, "negative window_start or dst_offset");
    const int64_t W = window_samples, cap = e->iq_capacity, dcap = dst->iq_capacity;
    if (W < 1) return sdr_fail(SDR_ERR_INVALID, "a window of %lld samples", (long long)W);
    if (W > cap || W > dcap)
        return sdr_fail(SDR_ERR_RANGE, "a window of %lld samples, the rings hold %lld and %lld", (long long)W, (long long)cap, (long long)dcap);
    const int64_t base = window_start % cap, dbase = dst_offset % dcap;
    const bool in_place = dst == e && dbase == base;
    if (dst == e && !in_place && cancel_windows_overlap(base, dbase, W, cap))
        return sdr_fail(SDR_ERR_INVALID, "the destination window overlaps the source window in the same ring");

    CancelPlan plan;
    if (int bad = cancel_plan(items, amps, n_ch, n_epochs, window_start, W, cap, e->n_slots, e->code_len_host.data(), &plan))
        return sdr_fail(bad == CANCEL_RANGE ? SDR_ERR_RANGE : bad == CANCEL_UNSUPPORTED ? SDR_ERR_UNSUPPORTED : SDR_ERR_INVALID, "%s",
                        plan.text);

    // one workspace: [items][counts][the two counters]
    const size_t b_items = round16(plan.items.size() * sizeof(CancelItemDev)), b_count = round16((size_t)n_ch * sizeof(int32_t));
    if (int rc = sdr_devbuf_reserve(e, &e->cancel_ws, b_items + b_count + 16)) return rc;
    CancelArgs a;
    a.src = e->iq, a.dst = dst->iq, a.src_cap = cap, a.dst_cap = dcap, a.base = base, a.dst_base = dbase;
    a.items = (const CancelItemDev*)e->cancel_ws.ptr;
    a.count = (const int32_t*)((char*)e->cancel_ws.ptr + b_items);
    a.stats = (unsigned long long*)((char*)e->cancel_ws.ptr + b_items + b_count);
    a.n_ch = n_ch, a.n_epochs = n_epochs, a.codes = e->codes, a.code_stride = e->code_stride, a.in_place = in_place ? 1 : 0, a.fs = fs;
    const int spg = ring_granule_samples(e->iq_fmt);
    a.win = probe_window(base, W, cap, spg);
    const int64_t tiles = (a.win.total + kThreads - 1) / kThreads;
    if (tiles > 0x7fffffff) return sdr_fail(SDR_ERR_UNSUPPORTED, "a window of %lld samples needs more tiles than one launch has", (long long)W);

    if (dst != e) SDR_HIP(hipStreamSynchronize(dst->stream));   // (whatever dst has queued on its ring comes first)
    if (int rc = sdr_iq_order_reader(e, &e->ctx0)) return rc;
    unsigned long long counters[2] = {0, 0};
    {
        ProfScope whole(e, "call_iq_cancel");
        {
            ProfScope ps(e, "cancel_items_upload");
            SDR_HIP(hipMemcpyAsync((void*)a.items, plan.items.data(), plan.items.size() * sizeof(CancelItemDev), hipMemcpyHostToDevice, e->stream));
            SDR_HIP(hipMemcpyAsync((void*)a.count, plan.count.data(), (size_t)n_ch * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
            SDR_HIP(hipMemsetAsync(a.stats, 0, 16, e->stream));
        }
        {
            ProfScope ps(e, "cancel_kernel");
            if (dst == e) sdr_iq_mark_written(e, dbase, W);
            with_fmt(e->iq_fmt, [&](auto fmt) {
                hipLaunchKernelGGL(cancel_kernel<decltype(fmt)::value>, dim3((unsigned)tiles), dim3(kThreads), 0, e->stream, a);
            });
            SDR_HIP(hipGetLastError());
        }
    }
    // (the pageable sources of the uploads above are this call's own: it waits here before they go)
    SDR_HIP(hipMemcpyAsync(counters, a.stats, sizeof counters, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    if (stats) {
        stats->samples_written = W;
        stats->samples_changed = (int64_t)counters[0];
        stats->clipped_components = (int64_t)counters[1];
    }
    return SDR_OK;
}

}  // extern "C"
