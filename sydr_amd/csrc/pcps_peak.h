// The peak search of the acquisition maps (K6): the first maximum of a PRN's map by parts, TwoCorrelationPeakComparison's
// second peak and ratio, and the same from the per-wave records of the map-free sweeps.  Included by pcps.hip (every search
// that ends in these kernels) and serial_search.hip (the first maximum by parts).  The (value, index) record `Best` and the
// wave-wide maximum are pcps_codelets.h's, which pcps_fused.hip shares.
#pragma once

#include "pcps_codelets.h"
#include "pcps_plan.h"

namespace {

using pcps::kThreads;
using pcps::kPeakParts;
static_assert(sizeof(Best) == pcps::kBestBytes, "the planner sizes the record buffers with it");
// ([[maybe_unused]]: serial_search.hip launches argmax_part_kernel alone)

__device__ __forceinline__ Best better(Best a, Best b) {
    // larger value wins; on ties the smaller flat index (first occurrence, np.argmax)
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
    return a;
}
__device__ __forceinline__ Best block_best(Best mine, Best* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Best o;
        o.v = __shfl_down(mine.v, off, 64);
        o.i = __shfl_down(mine.i, off, 64);
        mine = better(mine, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = mine;
    __syncthreads();
    Best r = sh[0];
    for (int w = 1; w < kThreads / 64; ++w) r = better(r, sh[w]);
    __syncthreads();
    return r;
}


__global__ __launch_bounds__(kThreads) void argmax_part_kernel(const double* __restrict__ map, long long per_prn,
                                                               Best* __restrict__ parts) {
    __shared__ Best sh[kThreads / 64];
    const int prn = blockIdx.y, part = blockIdx.x;
    const double* m = map + (size_t)prn * per_prn;
    long long chunk = (per_prn + kPeakParts - 1) / kPeakParts;
    long long lo = (long long)part * chunk, hi = lo + chunk < per_prn ? lo + chunk : per_prn;
    Best mine = {-1.0, 0x7fffffffffffffffLL};
    for (long long i = lo + threadIdx.x; i < hi; i += kThreads) {
        Best c = {m[i], i};
        mine = better(mine, c);
    }
    Best r = block_best(mine, sh);
    if (threadIdx.x == 0) parts[(size_t)prn * kPeakParts + part] = r;
}

// TwoCorrelationPeakComparison (acquisition.py:78-115), including its quirks.
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void peak_finish_kernel(const double* __restrict__ map, int nbins, int N,
                                                               int spc, const Best* __restrict__ parts,
                                                               long long* __restrict__ out_bin,
                                                               long long* __restrict__ out_code,
                                                               double* __restrict__ out_ratio) {
    __shared__ Best sh[kThreads / 64];
    const int prn = blockIdx.x;
    Best mine = {-1.0, 0x7fffffffffffffffLL};
    if (threadIdx.x < kPeakParts) mine = parts[(size_t)prn * kPeakParts + threadIdx.x];
    Best top = block_best(mine, sh);
    const long long bin = top.i / N;
    const int code = (int)(top.i - bin * N);
    const double* row = map + ((size_t)prn * nbins + bin) * N;
    const int e0 = code - spc, e1 = code + spc;
    // allowed = [a0,a1) U [b0,b1)
    int a0 = 0, a1 = 0, b0 = 0, b1 = 0;
    if (e0 < 1) {
        b0 = e1;
        b1 = N - 1;
    } else if (e1 >= N) {
        a1 = e0;
    } else {
        a1 = e0;
        b0 = e1;
        b1 = N - 1;
    }
    Best second = {-1.0, 0x7fffffffffffffffLL};
    for (int i = threadIdx.x; i < N; i += kThreads) {
        bool ok = (i >= a0 && i < a1) || (i >= b0 && i < b1);
        if (ok) {
            Best c = {row[i], i};
            second = better(second, c);
        }
    }
    Best p2 = block_best(second, sh);
    if (threadIdx.x == 0) {
        out_bin[prn] = bin;
        out_code[prn] = code;
        out_ratio[prn] = p2.v >= 0.0 ? top.v / p2.v : nan("");
    }
}

// Map-free search, step 2: the first maximum of PRN p's (never materialised) map from the per-wave records of the
// inverse row kernel.  Writes the winning (bin, code) and keeps the record for the ratio.
[[maybe_unused]] __global__ __launch_bounds__(kThreads) void argmax_records_kernel(const Best* __restrict__ recs, int per_prn, int N,
                                                                  Best* __restrict__ tops,
                                                                  long long* __restrict__ out_bin,
                                                                  long long* __restrict__ out_code) {
    __shared__ Best sh[kThreads / 64];
    const int prn = blockIdx.x;
    Best mine = {-1.0, 0x7fffffffffffffffLL};
    for (int i = threadIdx.x; i < per_prn; i += kThreads) mine = better(mine, recs[(size_t)prn * per_prn + i]);
    Best top = block_best(mine, sh);
    if (threadIdx.x == 0) {
        if (top.v < 0.0) top.i = 0;      // (no record at all: never an index the second sweep would read a row with)
        tops[prn] = top;
        out_bin[prn] = top.i / N;
        out_code[prn] = top.i - (top.i / N) * N;
    }
}

// Map-free search, step 4: the second peak of PRN p from the per-wave records of the pass over its winning row
// (which ran the maximum over the allowed columns only), and the ratio.
// (dev_bin / dev_code: the first peaks as argmax_records_kernel left them in device memory, where the second sweep
// read its rows from; out_* may be page-locked host memory -- this is the call's last kernel and hands everything over)
[[maybe_unused]] __global__ __launch_bounds__(64) void ratio_kernel(const Best* __restrict__ seconds, int per_prn,
                                                   const Best* __restrict__ tops, const long long* __restrict__ dev_bin,
                                                   const long long* __restrict__ dev_code, long long* __restrict__ out_bin,
                                                   long long* __restrict__ out_code, double* __restrict__ out_ratio) {
    const int prn = blockIdx.x;
    Best mine = {-1.0, 0x7fffffffffffffffLL};
    for (int i = threadIdx.x; i < per_prn; i += 64) mine = better(mine, seconds[(size_t)prn * per_prn + i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Best o;
        o.v = __shfl_down(mine.v, off, 64);
        o.i = __shfl_down(mine.i, off, 64);
        mine = better(mine, o);
    }
    if (threadIdx.x == 0) {
        out_ratio[prn] = mine.v >= 0.0 ? tops[prn].v / mine.v : nan("");
        if (out_bin != dev_bin) {
            out_bin[prn] = dev_bin[prn];
            out_code[prn] = dev_code[prn];
        }
    }
}

}  // namespace
