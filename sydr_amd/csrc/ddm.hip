// A delay-Doppler map around a known code phase and carrier (sdr_ddm, include/sydr_amd.h): taps, segments and
// frequencies together -- what a reacquisition, a warm start, a check of the tracked peak and reflectometry search.
//
//   stage 1  ddm_segments_kernel: one workgroup of 256 lanes per (item, segment q, chunk of taps).  The segment is an
//            EPL call of its own (its own linspace, rem_carrier_q, rem_code_q: ddm_plan.h), summed for every tap of the
//            chunk with sdr_corr_profile's two forms, tile by tile of 2048 samples: the carrier is wiped once per tile and
//            either the prefix sums of the wiped samples go to LDS and a tap is a term per chip run (corr_bounds.h), or --
//            below 8 samples per chip, or with the option "ddm_per_sample" -- the wiped samples go there and a tap is a
//            term per sample.  The accumulators stay in registers across the tiles of a segment; the lanes that share a
//            tap are added in lane order -> z[item][q][tap].
//   stage 2  ddm_map_kernel: one workgroup per (item, frequency k): the Q phasors exp(-2j*pi*d_k*tau_q) once, in LDS,
//            shared by all taps; a lane per tap adds the segments of a block coherently (s ascending) and the blocks'
//            powers (b ascending) -> map[item][k][tap].
//   stage 3  ddm_peak_kernel: one workgroup per item: the first maximum in row-major (k, tap) order, then the maximum and
//            the mean of the entries a chip or more from the peak's tap.
// All on the engine's stream, nothing crosses the host in between, no atomics: every sum has a fixed order.
#include <algorithm>
#include <cmath>

#include "corr_bounds.h"
#include "correlator.h"
#include "ddm_plan.h"

namespace {

using namespace sdr;

constexpr int kThreads = kDdmThreads;
constexpr int kPerLane = 8;                      // consecutive samples of a lane in the wipe: one Raw8 load
constexpr int kTile = kThreads * kPerLane;       // 2048 samples: 42 KB of LDS with a C/A code, three workgroups per compute unit
// P_k lives in slot k + (k >> 3): a lane's 8 stores are 9 slots (144 B = 36 banks) from its neighbour's, so the 8 lanes a
// 16-byte store serves together fall on 8 different bank quads (a stride of 128 B would put them all on one)
constexpr int kPrefixSlots = kTile + kTile / 8 + 1;
constexpr double kWalkMaxCodeStep = 1.0 / 8.0;   // fewer than 8 samples per chip: the per-sample form

__device__ __forceinline__ int prefix_slot(int k) { return k + (k >> 3); }

constexpr size_t kMaxLds = 160 * 1024;
constexpr size_t kFixedLds = (size_t)(kPrefixSlots + kThreads + 16 + kPerLane) * sizeof(double2);

template <int FMT, bool PER_SAMPLE>
__global__ __launch_bounds__(kThreads) void ddm_segments_kernel(const void* __restrict__ ring, int64_t capacity,
                                                                const DdmItemDev* __restrict__ items,
                                                                const int8_t* __restrict__ codes, int code_stride, int Q,
                                                                double first_chips, double step_chips, int n_taps,
                                                                int taps_per_group, int G, double fs,
                                                                double2* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) char ddm_lds[];
    double2* P = reinterpret_cast<double2*>(ddm_lds);      // prefix sums (or the wiped samples) of the tile
    double2* tot = P + kPrefixSlots;                       // [256] lane totals of the scan; the taps' partial sums at the end
    double2* grp = tot + kThreads;                         // [16]  totals of 16 lanes
    double2* rot = grp + 16;                               // [8]   exp(-1j * j * dphi)
    int8_t* chips = reinterpret_cast<int8_t*>(rot + kPerLane);   // [L] the slot's +-1 chips

    const int tid = threadIdx.x;
    const int item = blockIdx.x / Q, q = blockIdx.x - item * Q;
    const DdmItemDev it = items[item];
    const int8_t* src = codes + (size_t)it.slot * code_stride;
    for (int c = tid; c < it.L; c += kThreads) chips[c] = src[c];

    // the segment as an EPL call of its own
    int64_t a_q, b_q;
    ddm_segment_bounds(it.W, Q, q, &a_q, &b_q);
    const int n = (int)(b_q - a_q);
    int64_t base = it.base + a_q;                          // both below the capacity: one subtraction wraps it
    if (base >= capacity) base -= capacity;
    const double rem_carrier = ddm_rem_carrier(it.f0, it.rem_carrier, a_q, fs);
    const double rem_code = ddm_rem_code(it.rem_code, a_q, it.code_step);
    const double dphi = carrier_step(it.f0, fs);
    if (tid < kPerLane) {
        double sn, cs;
        sincos_reduced(-(double)tid * dphi, &sn, &cs);
        rot[tid] = make_double2(cs, sn);
    }
    if (tid == 0) P[0] = make_double2(0.0, 0.0);

    // this lane's tap and its share of it (lanes behind the last group of G idle in stage B)
    const int t_in = tid / G, g = tid - t_in * G;
    const int tap = blockIdx.y * taps_per_group + t_in;
    const bool live = t_in < taps_per_group && tap < n_taps;
    const double spacing = ddm_spacing(first_chips, step_chips, live ? tap : 0);
    const CorrTap T = corr_tap(n, rem_code, it.code_step, spacing);
    double accr = 0.0, acci = 0.0;
    __syncthreads();

    // (n may lie within a tile of 2^31: no sum below passes n, the counter stops before it would)
    for (int s0 = 0;; s0 += kTile) {
        const int len = n - s0 < kTile ? n - s0 : kTile;
        {   // ---- stage A: load, wipe the carrier, leave the tile in LDS
            const int l0 = tid * kPerLane;
            const int v = (n - s0) - l0;   // samples of this lane that belong to the segment: 8 or more = all
            const int i0 = v > 0 ? s0 + l0 : 0;
            double wr[kPerLane], wi[kPerLane];
            if (v > 0) {
                int64_t pos = base + i0;
                if (pos >= capacity) pos -= capacity;
                double sb, cb;
                sincos_reduced(__builtin_fma(-(double)i0, dphi, rem_carrier), &sb, &cb);
                auto wipe = [&](int j, double ar, double ai) {
                    const double2 r = rot[j];
                    const double zr = __builtin_fma(-ai, r.y, ar * r.x);
                    const double zi = __builtin_fma(ai, r.x, ar * r.y);
                    wr[j] = __builtin_fma(cb, zr, -sb * zi);
                    wi[j] = __builtin_fma(cb, zi, sb * zr);
                };
                // 16-byte loads aligned to the sample size only (2 B for ci8): a segment starts at any sample.  gfx950's
                // global path serves them; corr_profile.hip stage A has the precedent and the reasons.
                if (pos + kPerLane <= capacity) {   // (what lies behind the segment's end is still inside the ring)
                    Raw8<FMT> raw;
                    raw.load(ring, pos);
#pragma unroll
                    for (int j = 0; j < kPerLane; ++j) {
                        double ar, ai;
                        raw.get(j, ar, ai);
                        wipe(j, ar, ai);
                        if (j >= v) wr[j] = wi[j] = 0.0;
                    }
                } else {                            // the window crosses the ring's end inside these 8 samples
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
        // ---- stage B: samples [a, b) of the segment are this lane's piece of its tap in this tile
        int lo, hi;
        ddm_lane_piece(len, g, G, &lo, &hi);
        int a = s0 + lo;
        const int b = s0 + hi;
        if (live && a < b) {
            int p = corr_index(T, a);
            int c = corr_chip(p, it.L);
            if (PER_SAMPLE) {
                for (;;) {
                    const double sign = (double)chips[c];
                    const double2 w = P[prefix_slot(a - s0)];
                    accr = __builtin_fma(sign, w.x, accr);
                    acci = __builtin_fma(sign, w.y, acci);
                    if (++a == b) break;
                    const int pn = corr_index(T, a);
                    c = corr_chip_advance(c, (unsigned)pn - (unsigned)p, it.L);
                    p = pn;
                }
            } else {
                double2 pa = P[prefix_slot(a - s0)];
                while (a < b) {
                    int pn;
                    const int e = corr_run_end(T, a, b, p, &pn);
                    const double2 pe = P[prefix_slot(e - s0)];
                    const double sign = (double)chips[c];
                    accr = __builtin_fma(sign, pe.x - pa.x, accr);
                    acci = __builtin_fma(sign, pe.y - pa.y, acci);
                    c = corr_chip_advance(c, (unsigned)pn - (unsigned)p, it.L);
                    p = pn;
                    a = e;
                    pa = pe;
                }
            }
        }
        __syncthreads();   // (the next tile overwrites P)
        if (n - s0 <= kTile) break;
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
        z[(size_t)blockIdx.x * n_taps + tap] = make_double2(sr, si);
    }
}

// One workgroup per (item, frequency k).  The phasor of (k, q) is computed once and shared by every tap.
__global__ __launch_bounds__(kThreads) void ddm_map_kernel(const DdmItemDev* __restrict__ items, int B, int S, int K, int n_taps,
                                                           double step_hz, double fs, const double2* __restrict__ z,
                                                           double* __restrict__ map) {
    extern __shared__ __attribute__((aligned(16))) double2 ph[];   // [Q]
    const int tid = threadIdx.x, item = blockIdx.x, k = blockIdx.y;
    const int Q = B * S;
    const int64_t W = items[item].W;
    const double w = -2.0 * M_PI * ddm_offset_hz(k, K, step_hz);
    for (int q = tid; q < Q; q += kThreads) {
        int64_t a, b;
        ddm_segment_bounds(W, Q, q, &a, &b);
        double sn, cs;
        sincos_reduced(w * ddm_tau(a, b, fs), &sn, &cs);
        ph[q] = make_double2(cs, sn);
    }
    __syncthreads();
    const double2* zi = z + (size_t)item * Q * n_taps;
    for (int j = tid; j < n_taps; j += kThreads) {
        double power = 0.0;
        for (int b = 0; b < B; ++b) {
            double sr = 0.0, si = 0.0;
            for (int s = 0; s < S; ++s) {
                const double2 v = zi[(size_t)(b * S + s) * n_taps + j];
                const double2 r = ph[b * S + s];
                sr += v.x * r.x - v.y * r.y;
                si += v.x * r.y + v.y * r.x;
            }
            power += sr * sr + si * si;
        }
        map[((size_t)item * K + k) * n_taps + j] = power;
    }
}

// (value, index) records order by value, then by the LOWER index: the first maximum in row-major (k, tap) order
// (refine.hip's order).
__device__ __forceinline__ bool better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// One workgroup per item.  A map that holds a NaN or an Inf (a float ring's window held one) is reported, not searched.
__global__ __launch_bounds__(kThreads) void ddm_peak_kernel(const DdmItemDev* __restrict__ items, int K, int n_taps,
                                                            double first_chips, double step_chips, double step_hz,
                                                            const double* __restrict__ map, sdr_ddm_result* __restrict__ results) {
    __shared__ double red_v[kThreads], red_s[kThreads];
    __shared__ int red_i[kThreads], red_n[kThreads];
    __shared__ int peak_index;
    const int tid = threadIdx.x, item = blockIdx.x;
    const int n = K * n_taps;   // <= 4096 * 1024
    const double* m = map + (size_t)item * n;
    const int half = (K - 1) / 2;

    double bv = -1.0;
    int bi = 0, bad = 0;
    for (int i = tid; i < n; i += kThreads) {
        const double v = m[i];
        if (!(v - v == 0.0)) bad = 1;
        if (better(v, i, bv, bi)) bv = v, bi = i;
    }
    red_v[tid] = bv, red_i[tid] = bi, red_n[tid] = bad;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
            if (better(red_v[tid + d], red_i[tid + d], red_v[tid], red_i[tid])) red_v[tid] = red_v[tid + d], red_i[tid] = red_i[tid + d];
            red_n[tid] |= red_n[tid + d];
        }
        __syncthreads();
    }
    const bool found = red_n[0] == 0 && red_v[0] >= 0.0;
    const double peak_value = red_v[0];
    if (tid == 0) peak_index = found ? red_i[0] : half * n_taps;
    __syncthreads();
    const int pk = peak_index / n_taps, pj = peak_index - pk * n_taps;
    const double s_peak = ddm_spacing(first_chips, step_chips, pj);

    // the entries a chip or more from the peak's tap, any k: their maximum and their mean
    double ov = -1.0, os = 0.0;
    int on = 0;
    for (int i = tid; i < n; i += kThreads) {
        const int j = i % n_taps;
        if (fabs(ddm_spacing(first_chips, step_chips, j) - s_peak) >= 1.0) {
            const double v = m[i];
            if (v > ov) ov = v;
            os += v;
            ++on;
        }
    }
    red_v[tid] = ov, red_s[tid] = os, red_n[tid] = on;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
            if (red_v[tid + d] > red_v[tid]) red_v[tid] = red_v[tid + d];
            red_s[tid] += red_s[tid + d];
            red_n[tid] += red_n[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        sdr_ddm_result r;
        r.peak_bin = pk;
        r.peak_tap = pj;
        r.peak_hz = items[item].f0 + ddm_offset_hz(pk, K, step_hz);
        r.peak_chips = s_peak;
        r.peak_value = found ? peak_value : NAN;
        r.second_value = !found ? NAN : (red_n[0] > 0 ? red_v[0] : 0.0);
        r.noise_mean = !found ? NAN : (red_n[0] > 0 ? red_s[0] / (double)red_n[0] : 0.0);
        results[item] = r;
    }
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

template <int FMT>
const void* kernel_of(bool per_sample) {
    return per_sample ? (const void*)ddm_segments_kernel<FMT, true> : (const void*)ddm_segments_kernel<FMT, false>;
}

}  // namespace

extern "C" {

int sdr_ddm_bins(double span_hz, double step_hz) { return ddm_bins(span_hz, step_hz); }

int sdr_ddm(sdr_engine* e, const sdr_epl_item* items, int n_items, const sdr_ddm_cfg* cfg, sdr_ddm_result* results, double* map,
            double* segment_sums) {
    if (int rc = sdr_set_device(e)) return rc;   // (a resident tick server leaves, a parked slab goes into the ring)
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if (!items || !cfg || !results || n_items < 1 || n_items > kDdmMaxItems)
        return sdr_fail(SDR_ERR_INVALID, "no item, no configuration or no results for the delay-Doppler map");
    const int T = cfg->n_taps, B = cfg->n_blocks, S = cfg->n_segments;
    const double fs = cfg->fs, first_chips = cfg->first_chips, step_chips = cfg->step_chips;
    if (T < 1 || T > SDR_CORR_MAX_TAPS) return sdr_fail(SDR_ERR_INVALID, "n_taps %d outside 1..%d", T, SDR_CORR_MAX_TAPS);
    if (!std::isfinite(first_chips) || !std::isfinite(step_chips)) return sdr_fail(SDR_ERR_INVALID, "non-finite tap grid");
    if (!(fs > 0.0) || !std::isfinite(fs)) return sdr_fail(SDR_ERR_INVALID, "bad sampling frequency");
    const int K = ddm_bins(cfg->span_hz, cfg->step_hz);
    if (K <= 0) return sdr_fail(SDR_ERR_INVALID, "bad frequency grid");
    if (B < 1) return sdr_fail(SDR_ERR_INVALID, "n_blocks %d", B);
    if (S < 1 || S > kDdmMaxSegments) return sdr_fail(SDR_ERR_INVALID, "n_segments %d outside 1..%d", S, kDdmMaxSegments);
    if (S == 1 && K > 1)
        return sdr_fail(SDR_ERR_INVALID, "one segment per block carries no frequency information (%d frequencies asked for)", K);
    if (K > kDdmMaxBins) return sdr_fail(SDR_ERR_UNSUPPORTED, "a grid of %d frequencies (at most %d)", K, kDdmMaxBins);
    if ((int64_t)B * S > kDdmMaxAll)
        return sdr_fail(SDR_ERR_UNSUPPORTED, "%lld segments per item (at most %d)", (long long)B * S, kDdmMaxAll);
    const int Q = B * S;

    const double s_last = ddm_spacing(first_chips, step_chips, T - 1);
    const double s_min = std::min(first_chips, s_last), s_max = std::max(first_chips, s_last);
    e->ddm_host.resize((size_t)n_items * sizeof(DdmItemDev));
    DdmItemDev* host = reinterpret_cast<DdmItemDev*>(e->ddm_host.data());
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
        if (Q > it.n_samples)
            return sdr_fail(SDR_ERR_UNSUPPORTED, "item %d: %d segments in a window of %d samples", i, Q, it.n_samples);
        // every padded index of every tap of every segment inside +-2^30 (false for NaN / Inf as well): the indices grow
        // along the window, so its two ends bound them -- one chip of room for the segments' own rounding
        const double lo = std::ceil(it.rem_code + s_min);
        const double hi = std::ceil(it.code_step * (double)it.n_samples + it.rem_code + s_max) + 1.0;
        if (!(lo >= -1073741824.0) || !(hi <= 1073741824.0))
            return sdr_fail(SDR_ERR_UNSUPPORTED, "item %d: chip indices %.3g .. %.3g leave +-2^30", i, lo, hi);
        const int L = e->code_len_host[it.code_slot];
        if (kFixedLds + round16((size_t)L) > kMaxLds)
            return sdr_fail(SDR_ERR_UNSUPPORTED, "item %d: a code of %d chips (at most %zu fit the LDS beside the prefix sums)", i, L,
                            kMaxLds - kFixedLds);
        max_len = std::max(max_len, L);
        max_step = std::max(max_step, it.code_step);
        host[i] = DdmItemDev{it.code_slot, it.n_samples, it.start_sample % e->iq_capacity, it.carrier_hz, it.rem_carrier,
                             it.rem_code, it.code_step, L, 0};
    }
    const bool per_sample = e->ddm_per_sample || max_step > kWalkMaxCodeStep;
    const DdmGeometry geo = ddm_geometry((int64_t)n_items * Q, T, e->n_cus);

    // one workspace: [items][z: n*Q*T complex][map: n*K*T][results]
    const size_t b_items = round16((size_t)n_items * sizeof(DdmItemDev));
    const size_t b_z = (size_t)n_items * Q * T * sizeof(double2);
    const size_t b_map = round16((size_t)n_items * K * T * sizeof(double));
    const size_t b_res = (size_t)n_items * sizeof(sdr_ddm_result);
    if (int rc = sdr_devbuf_reserve(e, &e->ddm_ws, b_items + b_z + b_map + b_res)) return rc;
    char* ws = (char*)e->ddm_ws.ptr;
    DdmItemDev* d_items = (DdmItemDev*)ws;
    double2* d_z = (double2*)(ws + b_items);
    double* d_map = (double*)(ws + b_items + b_z);
    sdr_ddm_result* d_res = (sdr_ddm_result*)(ws + b_items + b_z + b_map);

    const void* kernel = sdr::with_fmt(e->iq_fmt, [&](auto fmt) { return kernel_of<decltype(fmt)::value>(per_sample); });
    const size_t shmem = kFixedLds + round16((size_t)max_len);
    // (above the 64 KB a kernel gets unasked: raised once per kernel of this engine, and again only for a longer code)
    size_t& lds_allowed = e->ddm_lds_allowed[(e->iq_fmt & 3) * 2 + (per_sample ? 1 : 0)];
    if (shmem > 64 * 1024 && shmem > lds_allowed) {
        SDR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        lds_allowed = shmem;
    }

    if (int rc = sdr_iq_order_reader(e, &e->ctx0)) return rc;   // (behind the uploads queued on the engine's stream so far)
    {
        ProfScope whole(e, "call_ddm");
        {
            ProfScope ps(e, "ddm_items_upload");
            SDR_HIP(hipMemcpyAsync(d_items, host, (size_t)n_items * sizeof(DdmItemDev), hipMemcpyHostToDevice, e->stream));
        }
        {
            ProfScope ps(e, "ddm_segments_kernel");
            const void* ring = e->iq;
            int64_t capacity = e->iq_capacity;
            const int8_t* codes = e->codes;
            int code_stride = e->code_stride, q_arg = Q, t_arg = T, tpg = geo.taps_per_group, lanes = geo.lanes_per_tap;
            double first = first_chips, step = step_chips, rate = fs;
            void* args[] = {&ring, &capacity, &d_items, &codes, &code_stride, &q_arg, &first, &step, &t_arg, &tpg, &lanes, &rate, &d_z};
            SDR_HIP(hipLaunchKernel(kernel, dim3((unsigned)(n_items * Q), (unsigned)geo.chunks), dim3(kThreads), args, shmem, e->stream));
        }
        {
            ProfScope ps(e, "ddm_map_kernel");
            hipLaunchKernelGGL(ddm_map_kernel, dim3((unsigned)n_items, (unsigned)K), dim3(kThreads), (size_t)Q * sizeof(double2), e->stream, d_items, B, S, K, T,
                               cfg->step_hz, fs, d_z, d_map);
            SDR_HIP(hipGetLastError());
        }
        {
            ProfScope ps(e, "ddm_peak_kernel");
            hipLaunchKernelGGL(ddm_peak_kernel, dim3((unsigned)n_items), dim3(kThreads), 0, e->stream, d_items, K, T, first_chips,
                               step_chips, cfg->step_hz, d_map, d_res);
            SDR_HIP(hipGetLastError());
        }
    }
    SDR_HIP(hipMemcpyAsync(results, d_res, b_res, hipMemcpyDeviceToHost, e->stream));
    if (map) SDR_HIP(hipMemcpyAsync(map, d_map, (size_t)n_items * K * T * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    if (segment_sums) SDR_HIP(hipMemcpyAsync(segment_sums, d_z, b_z, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

}  // extern "C"
