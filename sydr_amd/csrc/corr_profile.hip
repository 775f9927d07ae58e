// The correlation function on a dense tap grid (sdr_corr_profile, include/sydr_amd.h): what EPL returns for every spacing
// s_j = first_chips + j * step_chips, j < n_taps <= 1024, in one pass over the samples.
//
// One workgroup of 256 lanes per (item, chunk of taps); per segment of 4096 samples of the epoch:
//   stage A  every lane loads 16 consecutive samples once, wipes the carrier off them (the replica and the operation order
//            of correlator.h correlate_epoch) and the workgroup leaves their prefix sums P_0 = 0 .. P_len in LDS (the
//            prefix restarts per segment: |P| stays small, the differences accurate);
//   stage B  taps across lanes: G = 256 / (taps of the chunk) lanes share a tap, each walks the chip runs of its tap
//            inside its piece of the segment (corr_bounds.h: predicted on the real line, settled with the reference's own
//            per-sample expression) and adds c[chip] * (P[run end] - P[run start]) to two accumulators it keeps in
//            registers across segments.
// A tap costs ~a term per chip instead of one per sample.  Below ~8 samples per chip the walk saves nothing: there
// (PER_SAMPLE, or forced by the option "corr_profile_per_sample") stage A leaves the wiped samples themselves in LDS and a
// lane adds c[idx_i] * w_i sample by sample -- the same definition.  The chips are indexed modulo the code length here
// (the raw +-1 table of the slot, staged into LDS): taps many chips out and epochs of several code periods need no
// periodic staging.  The G partial sums of a tap are added in lane order: no atomics, two identical calls return
// identical bits.  Shares nothing with the tracking kernels.
#include <algorithm>
#include <cmath>

#include "corr_bounds.h"
#include "correlator.h"

namespace {

using namespace sdr;

constexpr int kThreads = 256;
constexpr int kPerLane = 16;                       // consecutive samples of a lane in stage A
constexpr int kSegment = kThreads * kPerLane;      // 4096 samples
// P_k lives in slot k + (k >> 4): a lane's 16 stores are 17 slots (272 B) from its neighbour's, an odd multiple of 16 B
// (a stride of 256 B would put every lane of a 16-byte store on the same banks)
constexpr int kPrefixSlots = kSegment + kSegment / 16 + 1;
constexpr int kMinTapsLog2 = 2, kMaxTapsLog2 = 8;  // taps per workgroup: 4 (a wave per tap) .. 256 (a lane per tap)
constexpr double kWalkMaxCodeStep = 1.0 / 8.0;     // fewer than 8 samples per chip: the per-sample form

__device__ __forceinline__ int prefix_slot(int k) { return k + (k >> 4); }

struct CorrItemDev {   // what the kernel needs of one sdr_epl_item
    int32_t slot, n;
    int64_t base;      // start_sample modulo the ring's capacity
    double carrier_hz, rem_carrier, rem_code, code_step;
    int32_t L, reserved;
};

constexpr size_t kMaxLds = 160 * 1024;   // LDS of a gfx950 compute unit: what one workgroup may ask for
constexpr size_t kFixedLds = (size_t)(kPrefixSlots + kThreads + 16 + 16) * sizeof(double2);

template <int FMT, bool PER_SAMPLE>
__global__ __launch_bounds__(kThreads) void corr_profile_kernel(const void* __restrict__ ring, int64_t capacity,
                                                                const CorrItemDev* __restrict__ items,
                                                                const int8_t* __restrict__ codes, int code_stride,
                                                                double first_chips, double step_chips, int n_taps,
                                                                int taps_log2, double fs, double2* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char corr_lds[];
    double2* P = reinterpret_cast<double2*>(corr_lds);   // prefix sums (or the wiped samples) of the segment
    double2* tot = P + kPrefixSlots;                     // [256] lane totals of the scan; the taps' partial sums at the end
    double2* grp = tot + kThreads;                       // [16]  totals of 16 lanes
    double2* rot = grp + 16;                             // [16]  exp(-1j * j * dphi)
    int8_t* chips = reinterpret_cast<int8_t*>(rot + 16); // [L]   the slot's +-1 chips

    const int tid = threadIdx.x;
    const CorrItemDev it = items[blockIdx.x];
    const int8_t* src = codes + (size_t)it.slot * code_stride;
    for (int q = tid; q < it.L; q += kThreads) chips[q] = src[q];
    const double dphi = carrier_step(it.carrier_hz, fs);
    if (tid < kPerLane) {
        double sn, cs;
        sincos_reduced(-(double)tid * dphi, &sn, &cs);
        rot[tid] = make_double2(cs, sn);
    }
    if (tid == 0) P[0] = make_double2(0.0, 0.0);

    // this lane's tap and its share of it
    const int lanes_log2 = 8 - taps_log2, G = 1 << lanes_log2;
    const int g = tid & (G - 1);
    const int tap = (blockIdx.y << taps_log2) + (tid >> lanes_log2);
    const bool live = tap < n_taps;
    double spacing = (double)(live ? tap : n_taps - 1) * step_chips;   // s_j = first + j * step: one multiply, one add
    spacing = first_chips + spacing;
    const CorrTap T = corr_tap(it.n, it.rem_code, it.code_step, spacing);
    double accr = 0.0, acci = 0.0;
    __syncthreads();

    for (int s0 = 0; s0 < it.n; s0 += kSegment) {
        const int len = it.n - s0 < kSegment ? it.n - s0 : kSegment;
        {   // ---- stage A
            const int l0 = tid * kPerLane, i0 = s0 + l0;
            const int v = it.n - i0;   // samples of this lane that belong to the epoch: 16 or more = all
            double wr[kPerLane], wi[kPerLane];
            if (v > 0) {
                int64_t pos = it.base + i0;
                if (pos >= capacity) pos -= capacity;
                double sb, cb;
                sincos_reduced(__builtin_fma(-(double)i0, dphi, it.rem_carrier), &sb, &cb);
                auto wipe = [&](int j, double ar, double ai) {
                    const double2 r = rot[j];
                    const double zr = __builtin_fma(-ai, r.y, ar * r.x);
                    const double zi = __builtin_fma(ai, r.x, ar * r.y);
                    wr[j] = __builtin_fma(cb, zr, -sb * zi);
                    wi[j] = __builtin_fma(cb, zi, sb * zr);
                };
                // Unaligned on purpose: an epoch starts at any sample, so these 16-byte loads are aligned to the sample size
                // only (2 B for ci8).  gfx950's global path serves them (correlator.h single_load relies on the same: "16-byte
                // loads from any 2-byte aligned address"); aligning the lanes to the ring instead would need a head pass through
                // ring_read in every segment and a prefix array that starts inside a lane's 16 samples.
                if (pos + kPerLane <= capacity) {   // (what lies behind the epoch's end is still inside the ring)
                    Raw8<FMT> raw[2];
                    raw[0].load(ring, pos);
                    raw[1].load(ring, pos + kGroup);
#pragma unroll
                    for (int j = 0; j < kPerLane; ++j) {
                        double ar, ai;
                        raw[j >> 3].get(j & 7, ar, ai);
                        wipe(j, ar, ai);
                        if (j >= v) wr[j] = wi[j] = 0.0;
                    }
                } else {                            // the window crosses the ring's end inside these 16 samples
#pragma unroll
                    for (int j = 0; j < kPerLane; ++j) {
                        wr[j] = wi[j] = 0.0;
                        if (j < v) {
                            const int64_t pj = pos + j >= capacity ? pos + j - capacity : pos + j;
                            const double2 x = ring_read<FMT>(ring, pj);
                            wipe(j, x.x, x.y);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) wr[j] = wi[j] = 0.0;
            }
            if (PER_SAMPLE) {
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) P[prefix_slot(l0 + j)] = make_double2(wr[j], wi[j]);
            } else {
#pragma unroll
                for (int j = 1; j < kPerLane; ++j) {
                    wr[j] += wr[j - 1];
                    wi[j] += wi[j - 1];
                }
                tot[tid] = make_double2(wr[kPerLane - 1], wi[kPerLane - 1]);
                __syncthreads();
                if (tid < 16) {
                    double sr = 0.0, si = 0.0;
                    for (int k = 0; k < 16; ++k) {
                        const double2 t = tot[16 * tid + k];
                        sr += t.x, si += t.y;
                    }
                    grp[tid] = make_double2(sr, si);
                }
                __syncthreads();
                double offr = 0.0, offi = 0.0;   // sum of everything in front of this lane, in a fixed order
                for (int k = 0; k < (tid >> 4); ++k) {
                    const double2 t = grp[k];
                    offr += t.x, offi += t.y;
                }
                for (int k = tid & ~15; k < tid; ++k) {
                    const double2 t = tot[k];
                    offr += t.x, offi += t.y;
                }
#pragma unroll
                for (int j = 0; j < kPerLane; ++j) P[prefix_slot(l0 + j + 1)] = make_double2(offr + wr[j], offi + wi[j]);
            }
        }
        __syncthreads();
        // ---- stage B: samples [a, b) of the epoch are this lane's piece of its tap
        int a = s0 + ((len * g) >> lanes_log2);
        const int b = s0 + ((len * (g + 1)) >> lanes_log2);
        if (live && a < b) {
            int p = corr_index(T, a);
            int q = corr_chip(p, it.L);
            if (PER_SAMPLE) {
                for (;;) {
                    const double c = (double)chips[q];
                    const double2 w = P[prefix_slot(a - s0)];
                    accr = __builtin_fma(c, w.x, accr);
                    acci = __builtin_fma(c, w.y, acci);
                    if (++a == b) break;
                    const int pn = corr_index(T, a);
                    q = corr_chip_advance(q, (unsigned)pn - (unsigned)p, it.L);
                    p = pn;
                }
            } else {
                double2 pa = P[prefix_slot(a - s0)];
                while (a < b) {
                    int pn;
                    const int e = corr_run_end(T, a, b, p, &pn);
                    const double2 pe = P[prefix_slot(e - s0)];
                    const double c = (double)chips[q];
                    accr = __builtin_fma(c, pe.x - pa.x, accr);
                    acci = __builtin_fma(c, pe.y - pa.y, acci);
                    q = corr_chip_advance(q, (unsigned)pn - (unsigned)p, it.L);
                    p = pn;
                    a = e;
                    pa = pe;
                }
            }
        }
        __syncthreads();   // (the next segment overwrites P)
    }

    // the G partial sums of a tap, in lane order
    tot[tid] = make_double2(accr, acci);
    __syncthreads();
    if (live && g == 0) {
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < G; ++k) {
            const double2 t = tot[tid + k];
            sr += t.x, si += t.y;
        }
        out[(size_t)blockIdx.x * n_taps + tap] = make_double2(sr, si);
    }
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

template <int FMT>
const void* kernel_of(bool per_sample) {
    return per_sample ? (const void*)corr_profile_kernel<FMT, true> : (const void*)corr_profile_kernel<FMT, false>;
}

}  // namespace

extern "C" {

int sdr_corr_profile(sdr_engine* e, const sdr_epl_item* items, int n_items, double first_chips, double step_chips, int n_taps,
                     double fs, double* out) {
    if (int rc = sdr_set_device(e)) return rc;   // (a resident tick server leaves, a parked slab goes into the ring)
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if (!items || !out || n_items < 1) return sdr_fail(SDR_ERR_INVALID, "no item or no output for the correlation profile");
    if (n_taps < 1 || n_taps > SDR_CORR_MAX_TAPS)
        return sdr_fail(SDR_ERR_INVALID, "n_taps %d outside 1..%d", n_taps, SDR_CORR_MAX_TAPS);
    if (!std::isfinite(first_chips) || !std::isfinite(step_chips)) return sdr_fail(SDR_ERR_INVALID, "non-finite tap grid");
    if (!(fs > 0.0) || !std::isfinite(fs)) return sdr_fail(SDR_ERR_INVALID, "bad sampling frequency");

    double s_last = (double)(n_taps - 1) * step_chips;
    s_last = first_chips + s_last;
    const double s_min = std::min(first_chips, s_last), s_max = std::max(first_chips, s_last);
    e->corr_host.resize((size_t)n_items * sizeof(CorrItemDev));
    CorrItemDev* host = reinterpret_cast<CorrItemDev*>(e->corr_host.data());
    int max_len = 0;
    double max_step = 0.0;
    for (int i = 0; i < n_items; ++i) {
        const sdr_epl_item& it = items[i];
        if (it.code_slot < 0 || it.code_slot >= e->n_slots || e->code_len_host[it.code_slot] <= 0)
            return sdr_fail(SDR_ERR_INVALID, "item %d: code slot %d is not staged", i, it.code_slot);
        if (it.n_samples < 1) return sdr_fail(SDR_ERR_INVALID, "item %d: n_samples %d", i, it.n_samples);
        if (!(it.code_step > 0.0) || !std::isfinite(it.code_step) || !std::isfinite(it.rem_code) ||
            !std::isfinite(it.rem_carrier) || !std::isfinite(it.carrier_hz))
            return sdr_fail(SDR_ERR_INVALID, "item %d: non-finite NCO parameters or non-positive code_step", i);
        if (it.start_sample < 0) return sdr_fail(SDR_ERR_RANGE, "item %d: negative start_sample", i);
        if (it.n_samples > e->iq_capacity)
            return sdr_fail(SDR_ERR_RANGE, "item %d: a window of %d samples, ring holds %lld", i, it.n_samples,
                            (long long)e->iq_capacity);
        // every padded index of every tap inside +-2^30 (false for NaN / Inf as well)
        const double lo = std::ceil(it.rem_code + s_min);
        const double hi = std::ceil(it.code_step * (double)it.n_samples + it.rem_code + s_max);
        if (!(lo >= -1073741824.0) || !(hi <= 1073741824.0))
            return sdr_fail(SDR_ERR_UNSUPPORTED, "item %d: chip indices %.3g .. %.3g leave +-2^30", i, lo, hi);
        const int L = e->code_len_host[it.code_slot];
        if (kFixedLds + round16((size_t)L) > kMaxLds)
            return sdr_fail(SDR_ERR_UNSUPPORTED, "item %d: a code of %d chips (at most %zu fit the LDS beside the prefix sums)", i, L,
                            kMaxLds - kFixedLds);
        max_len = std::max(max_len, L);
        max_step = std::max(max_step, it.code_step);
        host[i] = CorrItemDev{it.code_slot, it.n_samples, it.start_sample % e->iq_capacity, it.carrier_hz, it.rem_carrier,
                              it.rem_code, it.code_step, L, 0};
    }
    const bool per_sample = e->corr_per_sample || max_step > kWalkMaxCodeStep;

    // taps per workgroup: as few (as many lanes per tap) as leaves the launch at two workgroups per compute unit or fewer
    int taps_log2 = kMinTapsLog2;
    const long long budget = 2LL * std::max(e->n_cus, 1);
    while (taps_log2 < kMaxTapsLog2 && (long long)n_items * ((n_taps + (1 << taps_log2) - 1) >> taps_log2) > budget) ++taps_log2;
    const int chunks = (n_taps + (1 << taps_log2) - 1) >> taps_log2;

    // one workspace: [items][out: n_items * n_taps complex]
    const size_t b_items = round16((size_t)n_items * sizeof(CorrItemDev));
    const size_t b_out = (size_t)n_items * n_taps * sizeof(double2);
    if (int rc = sdr_devbuf_reserve(e, &e->corr_ws, b_items + b_out)) return rc;
    CorrItemDev* d_items = (CorrItemDev*)e->corr_ws.ptr;
    double2* d_out = (double2*)((char*)e->corr_ws.ptr + b_items);

    const void* kernel = sdr::with_fmt(e->iq_fmt, [&](auto fmt) { return kernel_of<decltype(fmt)::value>(per_sample); });
    const size_t shmem = kFixedLds + round16((size_t)max_len);
    // (above the 64 KB a kernel gets unasked: raised once per kernel of this engine, and again only for a longer code)
    size_t& lds_allowed = e->corr_lds_allowed[(e->iq_fmt & 3) * 2 + (per_sample ? 1 : 0)];
    if (shmem > lds_allowed) {
        SDR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        lds_allowed = shmem;
    }

    if (int rc = sdr_iq_order_reader(e, &e->ctx0)) return rc;   // (behind the uploads queued on the engine's stream so far)
    {
        ProfScope whole(e, "call_corr_profile");
        {
            ProfScope ps(e, "corr_items_upload");
            SDR_HIP(hipMemcpyAsync(d_items, host, (size_t)n_items * sizeof(CorrItemDev), hipMemcpyHostToDevice, e->stream));
        }
        {
            ProfScope ps(e, per_sample ? "corr_per_sample_kernel" : "corr_walk_kernel");
            const void* ring = e->iq;
            int64_t capacity = e->iq_capacity;
            const int8_t* codes = e->codes;
            int code_stride = e->code_stride;
            void* args[] = {&ring, &capacity, &d_items, &codes, &code_stride, &first_chips, &step_chips, &n_taps, &taps_log2, &fs, &d_out};
            SDR_HIP(hipLaunchKernel(kernel, dim3((unsigned)n_items, (unsigned)chunks), dim3(kThreads), args, shmem, e->stream));
        }
    }
    SDR_HIP(hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

}  // extern "C"
