// The coherent search under secondary-code hypotheses (sdr_pcps_coherent, include/sydr_amd.h): what lies behind the transforms.
//
//   combine  coherent_combine_kernel: a workgroup per (unit, tile of 256 lags), a lane owns a lag.  For every fine frequency k
//            and every block of kCohHyp hypotheses the lane walks the M periods once: C_m of its lag (read from the chunk's
//            scratch, coalesced: 16 bytes per lane, the tile's M x 4 KB stay in the L2 between the walks), rotated by g(m,b,k)
//            from LDS, added with the overlay's sign into the block's kCohHyp accumulators -- hypothesis h + 1 reads at period
//            m the chip hypothesis h reads at m + 1, so a block of periods takes ONE window of 2 kCohHyp - 1 signs from LDS
//            and every sign is a register of the unrolled body.  The running maximum of P stays in a register; R = its root.
//   keep     coherent_keep_kernel: a workgroup per PRN of the chunk keeps the M correlations of the PRN's largest R so far.
//   pick     coherent_pick_kernel: a workgroup per PRN, a thread per (h, k), the table P[h][k] of the peak cell from the kept
//            column -- the same expressions in the same order as the combine, so that peak^2 == power bit for bit.
// The rotations g(m,b,k) are made once per workgroup and round of frequencies with sincos_reduced on the phase in cycles less
// its nearest whole number.  Every sum has a fixed order, nothing is added atomically.  docs/notes/coherent_search.md.
#include <cmath>

#include "pcps_codelets.h"
#include "pcps_coherent.h"
#include "sincos_reduced.h"

#pragma clang fp contract(off)

namespace {

using namespace sdr;

constexpr int kCohThreads = 256;
// Hypotheses per block: NH10 is one block, NH20 two.  A block holds 2 x 10 accumulators, 19 signs and 10 loaded correlations.
constexpr int kCohHyp = 10;
constexpr int kCohRot = 2048;            // rotations in LDS per round of frequencies: 32 KB, >= 16 frequencies of 128 periods
constexpr int kCohExt = kSecMaxLen + kSecMaxPeriods + 2 * kCohHyp;   // the overlay row, continued periodically
constexpr int kPeakParts = 64;           // == pcps::kPeakParts (pcps_plan.h): records argmax_part_kernel leaves per PRN
static_assert(kCohRot / kSecMaxPeriods >= 1, "a round holds one frequency at least");

__device__ __forceinline__ double coh_freq(const CohGeom& g, int b, int k) {
    const double bin = g.bin_start + (double)b * g.bin_delta;
    return (g.if_hz - bin) + (double)(k - (g.K - 1) / 2) * g.step_hz;
}
// g(m,b,k) = exp(-2j*pi*f*(m*N)/fs): the phase in cycles, less its nearest whole number
__device__ __forceinline__ double2 coh_rotation(double f, int m, int N, double fs) {
    const double t = (double)((long long)m * N) / fs;
    const double ph = f * t;
    const double fr = ph - rint(ph);
    double s, c;
    sincos_reduced((2.0 * M_PI) * fr, &s, &c);
    return make_double2(c, -s);
}
// the overlay row of a PRN continued periodically: sgn[i] = c[i mod Ls], wrp[i] = a data symbol ends behind chip i
__device__ __forceinline__ void coh_overlay(const CohGeom& g, int p, double* sgn, int* wrp) {
    const int8_t* row = g.sec + (size_t)g.sec_rows[p] * g.Ls;
    for (int i = threadIdx.x; i < g.Ls + g.M + 2 * kCohHyp; i += kCohThreads) {
        const int c = i % g.Ls;
        sgn[i] = (double)row[c];
        wrp[i] = c == g.Ls - 1;
    }
}

template <int MODE>
__global__ __launch_bounds__(kCohThreads) void coherent_combine_kernel(const CohGeom g, int prn0, int bin0, int bins, int units,
                                                                       const double2* __restrict__ C, double* __restrict__ map) {
    __shared__ double2 rot[kCohRot];
    __shared__ double sgn[kCohExt];
    __shared__ int wrp[kCohExt];
    const int tid = threadIdx.x, ul = blockIdx.y;
    const int pl = ul / bins, bl = ul - pl * bins, p = prn0 + pl, b = bin0 + bl;
    const int tau = blockIdx.x * kCohThreads + tid;
    const int M = g.M, Ls = g.Ls;
    coh_overlay(g, p, sgn, wrp);
    // (a lane beyond the last lag reads the last lag's and stores nothing)
    const double2* __restrict__ col = C + (size_t)ul * g.T + (tau < g.N ? tau : g.N - 1);
    const size_t pitch = (size_t)units * g.T;
    double best = 0.0;
    const int kc = kCohRot / M;
    for (int k0 = 0; k0 < g.K; k0 += kc) {
        const int kn = g.K - k0 < kc ? g.K - k0 : kc;
        __syncthreads();
        for (int q = tid; q < kn * M; q += kCohThreads) {
            const int kk = q / M, m = q - kk * M;
            rot[q] = coh_rotation(coh_freq(g, b, k0 + kk), m, g.N, g.fs);
        }
        __syncthreads();
        for (int kk = 0; kk < kn; ++kk) {
            const double2* rk = rot + kk * M;
            for (int h0 = 0; h0 < Ls; h0 += kCohHyp) {
                double ar[kCohHyp], ai[kCohHyp], grp[kCohHyp];
#pragma unroll
                for (int j = 0; j < kCohHyp; ++j) ar[j] = ai[j] = grp[j] = 0.0;
                for (int m0 = 0; m0 < M; m0 += kCohHyp) {
                    double w[2 * kCohHyp - 1];
                    int wf[2 * kCohHyp - 1];
                    double2 cv[kCohHyp];
#pragma unroll
                    for (int i = 0; i < kCohHyp; ++i) {
                        const int m = m0 + i < M ? m0 + i : M - 1;
                        cv[i] = col[(size_t)m * pitch];
                    }
#pragma unroll
                    for (int t = 0; t < 2 * kCohHyp - 1; ++t) {
                        w[t] = sgn[h0 + m0 + t];
                        wf[t] = MODE == SDR_SEC_DATA ? wrp[h0 + m0 + t] : 0;
                    }
#pragma unroll
                    for (int i = 0; i < kCohHyp; ++i) {
                        if (m0 + i < M) {
                            const double2 gg = rk[m0 + i];
                            const double zr = cv[i].x * gg.x - cv[i].y * gg.y;
                            const double zi = cv[i].x * gg.y + cv[i].y * gg.x;
#pragma unroll
                            for (int j = 0; j < kCohHyp; ++j) {
                                ar[j] = __builtin_fma(w[i + j], zr, ar[j]);
                                ai[j] = __builtin_fma(w[i + j], zi, ai[j]);
                                if (MODE == SDR_SEC_DATA && wf[i + j]) {     // a data symbol ends with the code
                                    grp[j] += ar[j] * ar[j] + ai[j] * ai[j];
                                    ar[j] = ai[j] = 0.0;
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < kCohHyp; ++j) {
                    double pw = ar[j] * ar[j] + ai[j] * ai[j];
                    if (MODE == SDR_SEC_DATA) pw = grp[j] + pw;             // (the partial group at the end)
                    if (h0 + j < Ls) best = pw > best ? pw : best;          // a NaN never wins
                }
            }
        }
    }
    if (tau < g.N) map[((size_t)p * g.nbins + b) * g.N + tau] = sqrt(best);
}

__global__ __launch_bounds__(kCohThreads) void coherent_keep_kernel(int N, int T, int M, int prn0, int bin0, int bins, int units,
                                                                    const double2* __restrict__ C, const Best* __restrict__ parts,
                                                                    Best* __restrict__ best, double2* __restrict__ keep) {
    __shared__ long long at;
    const int pl = blockIdx.x, p = prn0 + pl;
    if (threadIdx.x == 0) {
        Best cand = {-1.0, 0x7fffffffffffffffLL};
        for (int i = 0; i < kPeakParts; ++i) {
            const Best o = parts[(size_t)pl * kPeakParts + i];
            if (o.v > cand.v || (o.v == cand.v && o.i < cand.i)) cand = o;
        }
        const bool any = cand.v >= 0.0;
        const long long flat = any ? cand.i + (long long)bin0 * N : cand.i;       // in the PRN's whole map
        const Best cur = bin0 == 0 ? Best{-1.0, 0x7fffffffffffffffLL} : best[p];
        const bool take = any && (cand.v > cur.v || (cand.v == cur.v && flat < cur.i));
        if (take) best[p] = Best{cand.v, flat};
        else if (bin0 == 0) best[p] = cur;
        at = take ? cand.i : -1;
    }
    __syncthreads();
    if (at < 0) return;
    const int bl = (int)(at / N), tau = (int)(at - (long long)bl * N);
    for (int m = threadIdx.x; m < M; m += kCohThreads)
        keep[(size_t)p * M + m] = C[((size_t)m * units + (size_t)pl * bins + bl) * T + tau];
}

template <int MODE>
__global__ __launch_bounds__(kCohThreads) void coherent_pick_kernel(const CohGeom g, const double2* __restrict__ keep,
                                                                    const double* __restrict__ map,
                                                                    const long long* __restrict__ peak_bin,
                                                                    const long long* __restrict__ peak_code,
                                                                    const double* __restrict__ peak_ratio,
                                                                    sdr_coh_result* __restrict__ results, double* __restrict__ power) {
    __shared__ double2 rot[kCohRot];
    __shared__ double2 col[kSecMaxPeriods];
    __shared__ double sgn[kCohExt];
    __shared__ int wrp[kCohExt];
    __shared__ double red_v[kCohThreads], red_xr[kCohThreads], red_xi[kCohThreads];
    __shared__ int red_i[kCohThreads];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int M = g.M, Ls = g.Ls, K = g.K;
    const int b = (int)peak_bin[p];
    coh_overlay(g, p, sgn, wrp);
    for (int m = tid; m < M; m += kCohThreads) col[m] = keep[(size_t)p * M + m];
    double* pw_tab = power + (size_t)p * Ls * K;
    double bv = -1.0, bxr = 0.0, bxi = 0.0;
    int bi = 0;
    const int kc = kCohRot / M;
    // ---- pass 1: P[h][k], m ascending; the thread's cells are written, and read again below, by the thread alone
    for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = K - k0 < kc ? K - k0 : kc;
        __syncthreads();
        for (int q = tid; q < kn * M; q += kCohThreads) {
            const int kk = q / M, m = q - kk * M;
            rot[q] = coh_rotation(coh_freq(g, b, k0 + kk), m, g.N, g.fs);
        }
        __syncthreads();
        for (int q = tid; q < Ls * kn; q += kCohThreads) {
            const int h = q / kn, kk = q - h * kn;
            double ar = 0.0, ai = 0.0, grp = 0.0;
            for (int m = 0; m < M; ++m) {
                const double2 gg = rot[kk * M + m], cv = col[m];
                const double zr = cv.x * gg.x - cv.y * gg.y;
                const double zi = cv.x * gg.y + cv.y * gg.x;
                ar = __builtin_fma(sgn[h + m], zr, ar);
                ai = __builtin_fma(sgn[h + m], zi, ai);
                if (MODE == SDR_SEC_DATA && wrp[h + m]) {
                    grp += ar * ar + ai * ai;
                    ar = ai = 0.0;
                }
            }
            double pw = ar * ar + ai * ai;
            if (MODE == SDR_SEC_DATA) pw = grp + pw, ar = ai = 0.0;
            const int idx = h * K + k0 + kk;
            pw_tab[idx] = pw;
            if (pw > bv || (pw == bv && idx < bi)) bv = pw, bi = idx, bxr = ar, bxi = ai;
        }
    }
    red_v[tid] = bv, red_i[tid] = bi, red_xr[tid] = bxr, red_xi[tid] = bxi;
    __syncthreads();
    for (int d = kCohThreads / 2; d > 0; d >>= 1) {
        if (tid < d && (red_v[tid + d] > red_v[tid] || (red_v[tid + d] == red_v[tid] && red_i[tid + d] < red_i[tid])))
            red_v[tid] = red_v[tid + d], red_i[tid] = red_i[tid + d], red_xr[tid] = red_xr[tid + d], red_xi[tid] = red_xi[tid + d];
        __syncthreads();
    }
    const bool found = red_v[0] >= 0.0;              // (false: every P was NaN)
    const int half = (K - 1) / 2;
    const int hs = found ? red_i[0] / K : 0, ks = found ? red_i[0] - hs * K : half;
    const double top = red_v[0], xr = red_xr[0], xi = red_xi[0];
    __syncthreads();
    // ---- pass 2: the best cell of any other hypothesis
    double other = -1.0;
    for (int k0 = 0; k0 < K; k0 += kc) {
        const int kn = K - k0 < kc ? K - k0 : kc;
        for (int q = tid; q < Ls * kn; q += kCohThreads) {
            const int h = q / kn, kk = q - h * kn;
            const double o = pw_tab[h * K + k0 + kk];
            if (h != hs && o > other) other = o;
        }
    }
    red_v[tid] = other;
    __syncthreads();
    for (int d = kCohThreads / 2; d > 0; d >>= 1) {
        if (tid < d && red_v[tid + d] > red_v[tid]) red_v[tid] = red_v[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        other = red_v[0];
        const long long tau = peak_code[p];
        sdr_coh_result r;
        r.carrier_hz = coh_freq(g, b, ks);
        r.peak = map[((size_t)p * g.nbins + b) * g.N + tau];
        r.peak_ratio = peak_ratio[p];
        r.power = found ? top : NAN;
        r.power_other = found && other >= 0.0 ? other : NAN;
        r.prompt_re = found ? xr : 0.0;
        r.prompt_im = found ? xi : 0.0;
        r.peak_code = tau;
        r.peak_bin = b, r.fine_idx = ks, r.sec_phase = hs, r.reserved = 0;
        results[p] = r;
    }
}

}  // namespace

int sdr_coh_combine(sdr_engine* e, const CohGeom& g, const sdr::CohChunk& c, const void* C, double* map) {
    ProfScope ps(e, "coherent_combine");
    const dim3 grid((g.N + kCohThreads - 1) / kCohThreads, c.units());
    if (g.mode == SDR_SEC_DATA)
        hipLaunchKernelGGL(coherent_combine_kernel<SDR_SEC_DATA>, grid, dim3(kCohThreads), 0, e->stream, g, c.prn0, c.bin0, c.bins,
                           c.units(), (const double2*)C, map);
    else
        hipLaunchKernelGGL(coherent_combine_kernel<SDR_SEC_PILOT>, grid, dim3(kCohThreads), 0, e->stream, g, c.prn0, c.bin0, c.bins,
                           c.units(), (const double2*)C, map);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_coh_keep(sdr_engine* e, const CohGeom& g, const sdr::CohChunk& c, const void* C, const void* parts, void* best, void* keep) {
    hipLaunchKernelGGL(coherent_keep_kernel, dim3(c.prns), dim3(kCohThreads), 0, e->stream, g.N, g.T, g.M, c.prn0, c.bin0, c.bins,
                       c.units(), (const double2*)C, (const Best*)parts, (Best*)best, (double2*)keep);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_coh_pick(sdr_engine* e, const CohGeom& g, int n_prn, const void* keep, const double* map, const long long* peak_bin,
                 const long long* peak_code, const double* peak_ratio, sdr_coh_result* results, double* power) {
    ProfScope ps(e, "coherent_pick");
    if (g.mode == SDR_SEC_DATA)
        hipLaunchKernelGGL(coherent_pick_kernel<SDR_SEC_DATA>, dim3(n_prn), dim3(kCohThreads), 0, e->stream, g, (const double2*)keep, map,
                           peak_bin, peak_code, peak_ratio, results, power);
    else
        hipLaunchKernelGGL(coherent_pick_kernel<SDR_SEC_PILOT>, dim3(n_prn), dim3(kCohThreads), 0, e->stream, g, (const double2*)keep, map,
                           peak_bin, peak_code, peak_ratio, results, power);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}
