// Secondary-code phase and fine carrier frequency behind an acquisition (sdr_acq_secondary, include/sydr_amd.h): the step
// behind the zero-padded search for signals whose sign may change at every code period.
//
//   stage 1  refine_segments_kernel (refine_segments.h, shared with sdr_acq_refine): z[item][m][s].
//   stage 2  secondary_search_kernel: a workgroup per (item, tile of kSecTile frequencies).  Phase A: Z[m][k] = sum_s z *
//            phasor of its tile into LDS.  Phase B: thread (h, k) walks the periods in ascending order under hypothesis h,
//            P[h][k]; the workgroup leaves its best (value, h*K + k, X) and its best value per h.
//   stage 3  secondary_pick_kernel: a workgroup per item reduces the tiles' records -- (value, then the lower index) is a total
//            order and a maximum has none, so the result does not depend on the tile size -- and fills the result.
// All on the engine's stream, nothing crosses the host in between; every sum has a fixed order (no atomics).
#include <algorithm>
#include <cmath>

#include "refine_segments.h"

namespace {

using namespace sdr;

constexpr int kSecThreads = 256;
// A tile of 16 frequencies: Z of 128 periods is 2 x 16 KB of LDS, beside 16 KB of segment times and the reduction's 7 KB
// inside the 64 KB a workgroup gets without asking (z itself is read from global memory: every 16 lanes one address).
// A row of Z is 16 doubles = 128 B with k fastest: phase A's wave writes four whole rows (512 contiguous bytes), phase B's
// reads 16 adjacent doubles, the same ones for its four hypotheses (a broadcast) -- no padding to gain anything from.
constexpr int kSecTile = 16;
constexpr int kSecRows = kSecThreads / kSecTile;   // periods (phase A) / hypotheses (phase B) in flight per round

struct SecBest {   // a tile's, then an item's best cell
    double v, xr, xi;
    int32_t idx, reserved;
};

__global__ __launch_bounds__(kSecThreads) void secondary_search_kernel(const RefineItemDev* __restrict__ items,
                                                                       const int8_t* __restrict__ sec, int Ls, int M, int S, int K,
                                                                       double step_hz, double fs, int mode,
                                                                       const double2* __restrict__ z, SecBest* __restrict__ part_best,
                                                                       double* __restrict__ part_h, double* __restrict__ power /* nullable */) {
    __shared__ double Zr[kSecMaxPeriods * kSecTile], Zi[kSecMaxPeriods * kSecTile];
    __shared__ double taus[kSecMaxProducts];
    __shared__ double red_v[kSecThreads], red_xr[kSecThreads], red_xi[kSecThreads];
    __shared__ int red_i[kSecThreads];
    __shared__ int8_t chips[kSecMaxLen];
    const int tid = threadIdx.x, tile = blockIdx.x, n_tiles = gridDim.x, item = blockIdx.y;
    const int kk = tid % kSecTile, row = tid / kSecTile;
    const int k = tile * kSecTile + kk;
    const RefineItemDev it = items[item];
    const double2* zi = z + (size_t)item * M * S;
    if (tid < Ls) chips[tid] = sec[(size_t)it.sec_row * Ls + tid];
    for (int q = tid; q < M * S; q += kSecThreads) {
        const int m = q / S, s = q - m * S;
        int64_t a0, a, b;
        segment_bounds(it.N, S, m, s, a0, a, b);
        taus[q] = (double)(a + b - 1) / 2.0 / fs;    // the segment's middle, seconds into the window
    }
    __syncthreads();

    // ---- phase A: the tile's Z[m][k], s ascending
    const int half = (K - 1) / 2;
    const double w = -2.0 * M_PI * ((double)(k - half) * step_hz);
    for (int m = row; m < M; m += kSecRows) {
        double sr = 0.0, si = 0.0;
        if (k < K)
            for (int s = 0; s < S; ++s) {
                const double2 v = zi[m * S + s];
                double sn, cs;
                sincos_reduced(w * taus[m * S + s], &sn, &cs);
                sr += v.x * cs - v.y * sn;
                si += v.x * sn + v.y * cs;
            }
        Zr[m * kSecTile + kk] = sr, Zi[m * kSecTile + kk] = si;
    }
    __syncthreads();

    // ---- phase B: hypothesis h at frequency k, m ascending; c = (h + m) mod Ls runs along
    double bv = -1.0, bxr = 0.0, bxi = 0.0;
    int bi = 0;
    for (int h0 = 0; h0 < Ls; h0 += kSecRows) {     // (the same count for every thread: the shuffles below need whole waves)
        const int h = h0 + row;
        const bool live = h < Ls && k < K;
        double p = -1.0;
        if (live) {
            int c = h;
            double gr = 0.0, gi = 0.0, groups = 0.0;
            for (int m = 0; m < M; ++m) {
                const double sg = (double)chips[c];
                gr += sg * Zr[m * kSecTile + kk], gi += sg * Zi[m * kSecTile + kk];
                if (++c == Ls) {
                    c = 0;
                    if (mode == SDR_SEC_DATA) groups += gr * gr + gi * gi, gr = gi = 0.0;   // a data symbol ends with the code
                }
            }
            p = gr * gr + gi * gi;
            if (mode == SDR_SEC_DATA) p = groups + p, gr = gi = 0.0;                        // (the partial group at the end)
            if (power) power[((size_t)item * Ls + h) * K + k] = p;
            if (better(p, h * K + k, bv, bi)) bv = p, bi = h * K + k, bxr = gr, bxi = gi;
        }
        // the best of hypothesis h inside the tile: its 16 frequencies are 16 adjacent lanes.  A NaN never wins.
        double hv = p > -1.0 ? p : -1.0;
        for (int d = kSecTile / 2; d > 0; d >>= 1) {
            const double o = __shfl_xor(hv, d);
            hv = o > hv ? o : hv;
        }
        if (kk == 0 && h < Ls) part_h[((size_t)item * n_tiles + tile) * Ls + h] = hv;
    }
    red_v[tid] = bv, red_i[tid] = bi, red_xr[tid] = bxr, red_xi[tid] = bxi;
    __syncthreads();
    for (int d = kSecThreads / 2; d > 0; d >>= 1) {
        if (tid < d && better(red_v[tid + d], red_i[tid + d], red_v[tid], red_i[tid]))
            red_v[tid] = red_v[tid + d], red_i[tid] = red_i[tid + d], red_xr[tid] = red_xr[tid + d], red_xi[tid] = red_xi[tid + d];
        __syncthreads();
    }
    if (tid == 0) part_best[(size_t)item * n_tiles + tile] = SecBest{red_v[0], red_xr[0], red_xi[0], red_i[0], 0};
}

__global__ __launch_bounds__(kSecThreads) void secondary_pick_kernel(const RefineItemDev* __restrict__ items, int Ls, int K, int n_tiles,
                                                                     double step_hz, const SecBest* __restrict__ part_best,
                                                                     const double* __restrict__ part_h,
                                                                     sdr_sec_result* __restrict__ results) {
    __shared__ double red_v[kSecThreads], red_xr[kSecThreads], red_xi[kSecThreads];
    __shared__ int red_i[kSecThreads];
    __shared__ double best_h[kSecMaxLen];
    const int tid = threadIdx.x, item = blockIdx.x;
    double bv = -1.0, bxr = 0.0, bxi = 0.0;
    int bi = 0;
    for (int t = tid; t < n_tiles; t += kSecThreads) {
        const SecBest r = part_best[(size_t)item * n_tiles + t];
        if (better(r.v, r.idx, bv, bi)) bv = r.v, bi = r.idx, bxr = r.xr, bxi = r.xi;
    }
    red_v[tid] = bv, red_i[tid] = bi, red_xr[tid] = bxr, red_xi[tid] = bxi;
    if (tid < Ls) {
        double hv = -1.0;
        for (int t = 0; t < n_tiles; ++t) {
            const double o = part_h[((size_t)item * n_tiles + t) * Ls + tid];
            hv = o > hv ? o : hv;
        }
        best_h[tid] = hv;
    }
    __syncthreads();
    for (int d = kSecThreads / 2; d > 0; d >>= 1) {
        if (tid < d && better(red_v[tid + d], red_i[tid + d], red_v[tid], red_i[tid]))
            red_v[tid] = red_v[tid + d], red_i[tid] = red_i[tid + d], red_xr[tid] = red_xr[tid + d], red_xi[tid] = red_xi[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        const int half = (K - 1) / 2;
        const bool found = red_v[0] >= 0.0;              // (false: every P was NaN)
        const int h = found ? red_i[0] / K : 0, k = found ? red_i[0] - h * K : half;
        double other = -1.0;
        for (int g = 0; g < Ls; ++g)
            if (g != h && best_h[g] > other) other = best_h[g];
        sdr_sec_result r;
        r.fine_hz = items[item].f0 + (double)(k - half) * step_hz;
        r.power = found ? red_v[0] : NAN;
        r.power_other = found && other >= 0.0 ? other : NAN;
        r.prompt_re = found ? red_xr[0] : 0.0;
        r.prompt_im = found ? red_xi[0] : 0.0;
        r.fine_idx = k;
        r.sec_phase = h;
        results[item] = r;
    }
}

size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int sdr_acq_secondary(sdr_engine* e, const sdr_sec_item* items, int n_items, const int8_t* sec_codes, int n_sec, int sec_len, double fs,
                      int n_periods, int n_segments, double span_hz, double step_hz, int mode, sdr_sec_result* results, double* power,
                      double* segment_sums) {
    if (int rc = sdr_set_device(e)) return rc;
    SecRequest r;
    r.ring = e->iq != nullptr, r.slots_allocated = e->codes != nullptr;
    r.g = RefineRing{e->iq_capacity, e->n_slots, e->code_len_host.data(), e->lut_stride};
    r.items = items, r.n_items = n_items, r.sec_codes = sec_codes, r.n_sec = n_sec, r.sec_len = sec_len;
    r.fs = fs, r.n_periods = n_periods, r.n_segments = n_segments, r.span_hz = span_hz, r.step_hz = step_hz;
    r.K = sdr_acq_refine_bins(span_hz, step_hz), r.mode = mode, r.results = results != nullptr;
    // the item list and the secondary rows as the device wants them, in the engine's own block (not a local: the list
    // outlives every return below, whatever state its copy is in)
    const size_t b_items = n_items > 0 && n_items <= 65535 ? round16((size_t)n_items * sizeof(RefineItemDev)) : 0;
    const size_t b_sec = b_items && n_sec > 0 && n_sec <= n_items && sec_len > 0 && sec_len <= kSecMaxLen ? round16((size_t)n_sec * sec_len) : 0;
    e->secondary_host.resize(b_items + b_sec);
    SecShape shape;
    if (int rc = secondary_request_check(r, &shape, b_items ? reinterpret_cast<RefineItemDev*>(e->secondary_host.data()) : nullptr))
        return sdr_fail(rc, "%s", shape.text);
    const int M = n_periods, S = n_segments, Ls = sec_len, K = r.K;
    std::copy(sec_codes, sec_codes + (size_t)n_sec * Ls, reinterpret_cast<int8_t*>(e->secondary_host.data() + b_items));

    // one workspace: [items][sec rows][z: n*M*S complex][partials: n*tiles best cells, n*tiles*Ls values][results][power: n*Ls*K, when asked for]
    const int n_tiles = (K + kSecTile - 1) / kSecTile;
    const size_t b_z = (size_t)n_items * M * S * sizeof(double2);
    const size_t b_best = (size_t)n_items * n_tiles * sizeof(SecBest);
    const size_t b_h = round16((size_t)n_items * n_tiles * Ls * sizeof(double));
    const size_t b_res = round16((size_t)n_items * sizeof(sdr_sec_result));
    const size_t b_pow = power ? (size_t)n_items * Ls * K * sizeof(double) : 0;
    if (int rc = sdr_devbuf_reserve(e, &e->secondary_ws, b_items + b_sec + b_z + b_best + b_h + b_res + b_pow)) return rc;
    char* ws = (char*)e->secondary_ws.ptr;
    RefineItemDev* d_items = (RefineItemDev*)ws;
    int8_t* d_sec = (int8_t*)(ws + b_items);
    double2* d_z = (double2*)(ws + b_items + b_sec);
    SecBest* d_best = (SecBest*)(ws + b_items + b_sec + b_z);
    double* d_h = (double*)(ws + b_items + b_sec + b_z + b_best);
    sdr_sec_result* d_res = (sdr_sec_result*)(ws + b_items + b_sec + b_z + b_best + b_h);
    double* d_pow = power ? (double*)(ws + b_items + b_sec + b_z + b_best + b_h + b_res) : nullptr;

    if (int rc = sdr_iq_order_reader(e, &e->ctx0)) return rc;   // (behind the uploads queued on the engine's stream so far)
    SDR_HIP(hipMemcpyAsync(ws, e->secondary_host.data(), b_items + b_sec, hipMemcpyHostToDevice, e->stream));
    {
        ProfScope whole(e, "call_secondary");
        {
            ProfScope ps(e, "secondary_segments");
            if (int rc = refine_launch_segments(e, d_items, n_items, M, S, shape.max_words, fs, d_z)) return rc;
        }
        {
            ProfScope ps(e, "secondary_search");
            hipLaunchKernelGGL(secondary_search_kernel, dim3(n_tiles, n_items), dim3(kSecThreads), 0, e->stream, d_items, d_sec, Ls, M, S,
                               K, step_hz, fs, mode, d_z, d_best, d_h, d_pow);
            SDR_HIP(hipGetLastError());
        }
        {
            ProfScope ps(e, "secondary_pick");
            hipLaunchKernelGGL(secondary_pick_kernel, dim3(n_items), dim3(kSecThreads), 0, e->stream, d_items, Ls, K, n_tiles, step_hz,
                               d_best, d_h, d_res);
            SDR_HIP(hipGetLastError());
        }
    }
    SDR_HIP(hipMemcpyAsync(results, d_res, (size_t)n_items * sizeof(sdr_sec_result), hipMemcpyDeviceToHost, e->stream));
    if (power) SDR_HIP(hipMemcpyAsync(power, d_pow, b_pow, hipMemcpyDeviceToHost, e->stream));
    if (segment_sums) SDR_HIP(hipMemcpyAsync(segment_sums, d_z, b_z, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

}  // extern "C"
