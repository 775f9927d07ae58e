// Deep acquisition (sdr_acq_deep, include/sydr_amd.h), the two kernels around its transforms:
//
//   fold        F[b][n] = sum_{c<C} x[s + c*N + n] * exp(-1j*(IF - bin_b)*phi[c*N + n])      one coherent block, every bin
//   shift-add   M[p][g][b][n] (+)= |R[p][b][(n + q[b]) mod N]|                                one block into its group
//
// The transform is linear, so the C mixed code periods of a coherent block are added BEFORE the forward transform: one
// forward transform per (bin, block) and one inverse per (PRN, bin, block) instead of C of each (pcps.hip run_map).
//
// Fold kernel.  A workgroup owns 256 consecutive n and a tile of kBinTile Doppler bins; a lane reads its C samples once
// (C strided, coalesced reads of the ring; held in registers as doubles) and walks the tile's bins, so the ring is read once
// per bin tile, not once per bin, and every store of F is a wave's 64 consecutive 16-byte values.  No LDS: nothing is shared
// between lanes.  The phasor of every (bin, c, n) is evaluated directly -- arg = (IF - bin_b) * (((c*N + n)*2)*pi/fs) in the
// statement's own operation order, through the library's sincos_reduced -- rather than composed as phasor(n) * phasor(c*N) or
// advanced from bin to bin: the kernel is then the first pass of sdr_pcps's forward transform (load_elem<LOAD_IQ_MIX>) with
// the sum moved in front, value for value, and its error is sincos_reduced's < 1 ulp with nothing accumulated over bins or
// periods.  The price is C sincos_reduced (~45 fp64 operations each) per (bin, n) where composition would pay one and C
// complex multiplications; the fold's arithmetic stays a fraction of what the n_prn inverse transforms behind it cost per
// (bin, n) (docs/notes/deep_acq.md has the count and the measured share).
#include "acq_deep.h"
#include "sincos_reduced.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kBinTile = 16;   // bins per workgroup: 256 B written per sample column against <= 16*C B read (cf64 ring)

// CT: the compiled-in bound of the period loop (the lane's samples stay in registers), C <= CT periods are live.
template <int FMT, int CT>
__global__ __launch_bounds__(kThreads) void deep_fold_kernel(const void* __restrict__ ring, int64_t capacity, int64_t first,
                                                             int N, int C, int nbins, double fs, double if_hz,
                                                             double bin_start, double bin_delta, double2* __restrict__ F) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    double2 x[CT];
    double pp[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        x[c] = make_double2(0.0, 0.0);
        pp[c] = 0.0;
        if (c < C) {
            const int64_t m = (int64_t)c * N + n;              // index into phasePoints: the carrier restarts with the block
            x[c] = sdr::ring_read<FMT>(ring, (first + m) % capacity);
            pp[c] = (double)(m * 2) * M_PI;                    // acquisition.py:33: ((m*2)*pi)/fs
            pp[c] = pp[c] / fs;
        }
    }
    const int b0 = blockIdx.y * kBinTile;
    const int b1 = b0 + kBinTile < nbins ? b0 + kBinTile : nbins;
    for (int b = b0; b < b1; ++b) {
        const double bin = bin_start + (double)b * bin_delta;
        const double freq = if_hz - bin;
        double2 acc = make_double2(0.0, 0.0);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (c < C) {
                double s, cs;
                sdr::sincos_reduced(freq * pp[c], &s, &cs);
                // (cs - 1j*s) * x, added in ascending c
                acc.x += cs * x[c].x + s * x[c].y;
                acc.y += cs * x[c].y - s * x[c].x;
            }
        }
        F[(size_t)b * N + n] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void deep_shift_acc_kernel(const double* __restrict__ mag, double* __restrict__ map,
                                                                  const int32_t* __restrict__ q, int nbins, int N, int groups,
                                                                  int g, int store) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const int row = blockIdx.y;                    // (PRN of the sweep, bin)
    const int p = row / nbins, b = row - p * nbins;
    int src = n + q[b];                            // 0 <= q[b] < N
    if (src >= N) src -= N;
    const double v = mag[(size_t)row * N + src];
    double* dst = map + (((size_t)p * groups + g) * nbins + b) * N + n;
    *dst = store ? 0.0 + v : *dst + v;
}

template <int FMT>
void launch_fold(sdr_engine* e, int64_t first, int N, int C, int nbins, double fs, double if_hz, double bin_start,
                 double bin_delta, double2* F) {
    const dim3 grid((N + kThreads - 1) / kThreads, (nbins + kBinTile - 1) / kBinTile);
#define SDR_DEEP_FOLD(CT)                                                                                              \
    hipLaunchKernelGGL((deep_fold_kernel<FMT, CT>), grid, dim3(kThreads), 0, e->stream, (const void*)e->iq, e->iq_capacity, \
                       first, N, C, nbins, fs, if_hz, bin_start, bin_delta, F)
    if (C <= 1) SDR_DEEP_FOLD(1);
    else if (C <= 2) SDR_DEEP_FOLD(2);
    else if (C <= 5) SDR_DEEP_FOLD(5);
    else if (C <= 10) SDR_DEEP_FOLD(10);
    else SDR_DEEP_FOLD(20);
#undef SDR_DEEP_FOLD
}

}  // namespace

int sdr_deep_fold(sdr_engine* e, int64_t first, int N, int coh, int nbins, double fs, double if_hz, double bin_start,
                  double bin_delta, void* F) {
    if (coh < 1 || coh > 20 || N < 1 || nbins < 1 || first < 0 || !F) return sdr_fail(SDR_ERR_INVALID, "bad fold request");
    ProfScope ps(e, "deep_fold");
    double2* f = (double2*)F;
    sdr::with_fmt(e->iq_fmt, [&](auto fmt) { launch_fold<decltype(fmt)::value>(e, first, N, coh, nbins, fs, if_hz, bin_start, bin_delta, f); });
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

int sdr_deep_shift_acc(sdr_engine* e, const double* mag, double* map, const int32_t* q, int n_prn, int nbins, int N, int groups,
                       int g, int store) {
    if (n_prn < 1 || (int64_t)n_prn * nbins > 65535 || g < 0 || g >= groups) return sdr_fail(SDR_ERR_INVALID, "bad shift request");
    ProfScope ps(e, "deep_shift_acc");
    hipLaunchKernelGGL(deep_shift_acc_kernel, dim3((N + kThreads - 1) / kThreads, n_prn * nbins), dim3(kThreads), 0, e->stream,
                       mag, map, q, nbins, N, groups, g, store);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

extern "C" int64_t sdr_acq_deep_shift(const sdr_deep_cfg* cfg, int bin, int64_t block) {
    if (!cfg || !(cfg->carrier_rf_hz > 0.0) || bin < 0 || block < 0) return 0;
    // the search's own grid and samples per code (acq_request.h)
    const double d = sdr::acq_bin(cfg->doppler_range, cfg->doppler_step, bin);
    const int64_t N = (int64_t)sdr::acq_samples_per_code(cfg->fs);
    const double t = (double)(block * (int64_t)cfg->coh * N);
    return (int64_t)std::nearbyint(d * t / cfg->carrier_rf_hz);
}
