// Fine carrier-frequency and bit-edge refinement behind an acquisition (sdr_acq_refine, include/sydr_amd.h): the step
// the textbook receiver has between its coarse search and its Costas loop, which the reference left out.
//
//   stage 1  refine_segments_kernel: one wave per segment (item, period m, segment s) wipes code and coarse carrier off
//            its samples of the ring with the E/P/L correlator's per-sample core (correlator.h correlate_epoch, one tap at
//            spacing 0.0: the prompt tap of EPL, hence its parity with the oracle) -> z[item][m][s].
//   stage 2  refine_search_kernel: one workgroup per item, a thread per fine-grid frequency: Z[m][k] = sum_s z * phasor,
//            the M sign hypotheses from prefix sums, the first maximum of P[h][k] in row-major order.
// Both on the engine's stream, nothing crosses the host in between; every sum has a fixed order (no atomics).
#include <algorithm>
#include <cmath>

#include "refine_segments.h"

namespace {

using namespace sdr;

constexpr int kSearchThreads = 256;

// better() (refine_segments.h): a NaN never wins a comparison, so a window that holds NaN / Inf samples (a float ring) keeps
// the initial record, which the last thread turns into power = power_no_edge = NaN, fine_hz = f0, fine_idx = (K-1)/2, bit_edge = 0.
__global__ __launch_bounds__(kSearchThreads) void refine_search_kernel(const RefineItemDev* __restrict__ items, int M, int S, int K,
                                                                       double step_hz, double fs, const double2* __restrict__ z,
                                                                       double* __restrict__ power /* nullable */,
                                                                       sdr_refine_result* __restrict__ results) {
    __shared__ double2 zs[kRefineMaxPeriods * kRefineMaxSegments];
    __shared__ double taus[kRefineMaxPeriods * kRefineMaxSegments];
    __shared__ double best_v[kSearchThreads], best0_v[kSearchThreads];
    __shared__ int best_i[kSearchThreads];
    const int tid = threadIdx.x, item = blockIdx.x;
    const RefineItemDev it = items[item];
    for (int q = tid; q < M * S; q += kSearchThreads) {
        const int m = q / S, s = q - m * S;
        int64_t a0, a, b;
        segment_bounds(it.N, S, m, s, a0, a, b);
        zs[q] = z[(size_t)item * M * S + q];
        taus[q] = (double)(a + b - 1) / 2.0 / fs;    // the segment's middle, seconds into the window
    }
    __syncthreads();

    const int half = (K - 1) / 2;
    double bv = -1.0, b0 = -1.0;
    int bi = 0;
    for (int k = tid; k < K; k += kSearchThreads) {
        const double w = -2.0 * M_PI * ((double)(k - half) * step_hz);
        double zr[kRefineMaxPeriods], zi[kRefineMaxPeriods];
        double tr = 0.0, ti = 0.0;
#pragma unroll
        for (int m = 0; m < kRefineMaxPeriods; ++m) {
            zr[m] = zi[m] = 0.0;
            if (m < M) {
                double sr = 0.0, si = 0.0;
                for (int s = 0; s < S; ++s) {
                    const double2 v = zs[m * S + s];
                    double sn, cs;
                    sincos_reduced(w * taus[m * S + s], &sn, &cs);
                    sr += v.x * cs - v.y * sn;
                    si += v.x * sn + v.y * cs;
                }
                zr[m] = sr, zi[m] = si;
                tr += sr, ti += si;
            }
        }
        // hypothesis h: periods m >= h enter with the opposite sign: sum_{m<h} Z - sum_{m>=h} Z = 2 * prefix_h - total
        double pr = 0.0, pi = 0.0;
#pragma unroll
        for (int h = 0; h < kRefineMaxPeriods; ++h) {
            if (h < M) {
                const double xr = h ? 2.0 * pr - tr : tr, xi = h ? 2.0 * pi - ti : ti;
                const double p = xr * xr + xi * xi;
                if (power) power[((size_t)item * M + h) * K + k] = p;
                if (better(p, h * K + k, bv, bi)) bv = p, bi = h * K + k;
                if (h == 0 && p > b0) b0 = p;
                pr += zr[h], pi += zi[h];
            }
        }
    }
    best_v[tid] = bv, best_i[tid] = bi, best0_v[tid] = b0;
    __syncthreads();
    for (int d = kSearchThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
            if (better(best_v[tid + d], best_i[tid + d], best_v[tid], best_i[tid])) best_v[tid] = best_v[tid + d], best_i[tid] = best_i[tid + d];
            if (best0_v[tid + d] > best0_v[tid]) best0_v[tid] = best0_v[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool found = best_v[0] >= 0.0;             // (false: every P was NaN)
        const int h = found ? best_i[0] / K : 0, k = found ? best_i[0] - h * K : half;
        sdr_refine_result r;
        r.fine_hz = it.f0 + (double)(k - half) * step_hz;
        r.power = found ? best_v[0] : NAN;
        r.power_no_edge = found && best0_v[0] >= 0.0 ? best0_v[0] : NAN;
        r.fine_idx = k;
        r.bit_edge = h;
        results[item] = r;
    }
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int sdr_acq_refine_bins(double span_hz, double step_hz) {
    if (!(step_hz > 0.0) || !(span_hz >= 0.0)) return 0;
    const double half = std::floor(span_hz / step_hz);
    if (!(half < 1e9)) return 0;
    return 2 * (int)half + 1;
}

int sdr_acq_refine(sdr_engine* e, const sdr_refine_item* items, int n_items, double fs, int n_periods, int n_segments,
                   double span_hz, double step_hz, sdr_refine_result* results, double* power, double* segment_sums) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if (!items || n_items <= 0 || n_items > 65535) return sdr_fail(SDR_ERR_INVALID, "no item to refine");
    if (!results) return sdr_fail(SDR_ERR_INVALID, "results is NULL");
    if (!(fs > 0.0) || !std::isfinite(fs)) return sdr_fail(SDR_ERR_INVALID, "bad sampling frequency");
    const int M = n_periods, S = n_segments;
    if (M < 1 || M > kRefineMaxPeriods)
        return sdr_fail(SDR_ERR_INVALID, "n_periods %d outside 1..%d (one data bit: at most one edge)", M, kRefineMaxPeriods);
    if (S < 1 || S > kRefineMaxSegments) return sdr_fail(SDR_ERR_INVALID, "n_segments %d outside 1..%d", S, kRefineMaxSegments);
    const int K = sdr_acq_refine_bins(span_hz, step_hz);
    if (K <= 0 || !std::isfinite(span_hz) || !std::isfinite(step_hz)) return sdr_fail(SDR_ERR_INVALID, "bad fine frequency grid");
    if (K > kRefineMaxBins) return sdr_fail(SDR_ERR_UNSUPPORTED, "fine grid of %d frequencies (at most %d)", K, kRefineMaxBins);

    // (the engine's own block, not a local: the list outlives every return below, whatever state its copy is in)
    e->refine_host.resize((size_t)n_items * sizeof(RefineItemDev));
    RefineItemDev* host = reinterpret_cast<RefineItemDev*>(e->refine_host.data());
    const RefineRing ring{e->iq_capacity, e->n_slots, e->code_len_host.data(), e->lut_stride};
    int max_words = 0;
    for (int i = 0; i < n_items; ++i) {
        const sdr_refine_item& it = items[i];
        char text[200];
        if (int rc = refine_admit_item(ring, i, it.code_slot, it.start_sample, it.carrier_hz, it.code_hz, fs, M, S, &host[i], text, sizeof text))
            return sdr_fail(rc, "%s", text);
        max_words = std::max(max_words, (int)host[i].lut_words);
    }

    // one workspace: [items][z: n*M*S complex][results][power: n*M*K, when asked for]
    const size_t b_items = round16((size_t)n_items * sizeof(RefineItemDev));
    const size_t b_z = (size_t)n_items * M * S * sizeof(double2);
    const size_t b_res = round16((size_t)n_items * sizeof(sdr_refine_result));
    const size_t b_pow = power ? (size_t)n_items * M * K * sizeof(double) : 0;
    if (int rc = sdr_devbuf_reserve(e, &e->refine_ws, b_items + b_z + b_res + b_pow)) return rc;
    char* ws = (char*)e->refine_ws.ptr;
    RefineItemDev* d_items = (RefineItemDev*)ws;
    double2* d_z = (double2*)(ws + b_items);
    sdr_refine_result* d_res = (sdr_refine_result*)(ws + b_items + b_z);
    double* d_pow = power ? (double*)(ws + b_items + b_z + b_res) : nullptr;

    if (int rc = sdr_iq_order_reader(e, &e->ctx0)) return rc;   // (behind the uploads queued on the engine's stream so far)
    SDR_HIP(hipMemcpyAsync(d_items, host, (size_t)n_items * sizeof(RefineItemDev), hipMemcpyHostToDevice, e->stream));
    {
        ProfScope whole(e, "call_refine");
        {
            ProfScope ps(e, "refine_segments");
            if (int rc = refine_launch_segments(e, d_items, n_items, M, S, max_words, fs, d_z)) return rc;
        }
        {
            ProfScope ps(e, "refine_search");
            hipLaunchKernelGGL(refine_search_kernel, dim3(n_items), dim3(kSearchThreads), 0, e->stream, d_items, M, S, K, step_hz, fs,
                               d_z, d_pow, d_res);
            SDR_HIP(hipGetLastError());
        }
    }
    SDR_HIP(hipMemcpyAsync(results, d_res, (size_t)n_items * sizeof(sdr_refine_result), hipMemcpyDeviceToHost, e->stream));
    if (power) SDR_HIP(hipMemcpyAsync(power, d_pow, b_pow, hipMemcpyDeviceToHost, e->stream));
    if (segment_sums) SDR_HIP(hipMemcpyAsync(segment_sums, d_z, b_z, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

}  // extern "C"
