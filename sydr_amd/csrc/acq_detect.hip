// Detection statistics on the resident maps of a deep search (sdr_acq_deep_detect, include/sydr_amd.h): the further peaks
// outside the zones of the earlier ones, and the count, the mean and the variance of the cells whose code column lies clear
// of every peak.  docs/notes/detect.md has the statement, the design and the cost.
//
// Every pass walks a PRN's map in parts of kDetectPartCells columns of ONE map row (detect_zone.h): grid = (row, part of
// the row, PRN).  The row's bin is then uniform in a workgroup, and so is the answer to "can a zone reach this part at
// all" -- for all but a few parts of a map it cannot, and their lanes test nothing per cell.  Where a zone does reach the
// part, a lane compares its column's circular distance with the window: no division per cell anywhere.  A lane owns
// kDetectPairs pairs of neighbouring columns; a pair is one 16-byte load where the row starts on a 16-byte boundary (N even,
// or an even row of an even-sized map) and two 8-byte loads where it does not, so which cells a lane adds, and in which
// order, never depends on the alignment -- nor on n_prn or the device: a PRN's figures are a function of its own map.
//
//   masked arg-max   part kernel: the best cell of a part outside the zones of peaks j < k; finish kernel: the best part
//                    (ties to the smaller linear index), written to device memory where pass k + 1 reads it
//   masked moments   part kernel: a part's sum and count (pass 0) or its sum of squared deviations from the rounded mean
//                    (pass 1); finish kernel: the parts added in ascending order by one workgroup, mean = sum / count and
//                    variance = squares / count made on the device -- no floating-point atomics, an integer count
#include "acq_deep.h"
#include "detect_zone.h"
#include "pcps_codelets.h"

#pragma clang fp contract(off)

namespace {

using namespace sdr;

constexpr int kThreads = kDetectThreads;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ Best better(Best a, Best b) {
    // larger value wins; on ties the smaller flat index (pcps_peak.h)
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
    for (int w = 1; w < kWaves; ++w) r = better(r, sh[w]);
    return r;
}
// The workgroup's sum in a fixed order: lanes pairwise at distances 32, 16, ... 1, then the waves ascending.
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < kWaves; ++w) r = r + sh[w];
    return r;
}
__device__ __forceinline__ long long block_count(long long v, long long* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    long long r = sh[0];
    for (int w = 1; w < kWaves; ++w) r += sh[w];
    return r;
}

// The code columns of the peaks whose zone can reach this workgroup's part (bit j of `mask`): uniform in the workgroup.
struct Zones {
    int code[kDetectMaxPeaks];
    unsigned mask;
};
__device__ __forceinline__ bool zone_hit(const Zones& z, int n, int N, int excl_code) {
    bool hit = false;
#pragma unroll
    for (int j = 0; j < kDetectMaxPeaks; ++j) hit |= ((z.mask >> j) & 1u) && detect_dist(n, z.code[j], N) <= excl_code;
    return hit;
}
// bins: test |b - b_j| <= excl_bins too (the zones of the peak search); otherwise whole code columns (the noise cells).
template <bool BINS>
__device__ __forceinline__ Zones part_zones(const DeepDetectPeak* __restrict__ peaks, int n_peaks, int b, int nbins, int c0,
                                            int c1, int N, int excl_code, int excl_bins) {
    Zones z;
    z.mask = 0;
#pragma unroll
    for (int j = 0; j < kDetectMaxPeaks; ++j) {
        z.code[j] = 0;
        if (j < n_peaks) {
            const DeepDetectPeak p = peaks[j];
            if (p.row >= 0) {
                z.code[j] = p.code;
                const bool near = !BINS || detect_bin_near(b, p.row % nbins, excl_bins);
                if (near && detect_run_touches(c0, c1, p.code, N, excl_code)) z.mask |= 1u << j;
            }
        }
    }
    return z;
}

// f(n, M[row][n]) for this lane's columns of [c0, c1), ascending.
template <class F>
__device__ __forceinline__ void lane_cells(const double* __restrict__ row, bool aligned, int c0, int c1, F&& f) {
#pragma unroll
    for (int i = 0; i < kDetectPairs; ++i) {
        const int n = detect_pair_column(c0, i, threadIdx.x);
        if (n + 1 < c1) {
            double a, b;
            if (aligned) {
                const double2 v = *reinterpret_cast<const double2*>(row + n);
                a = v.x, b = v.y;
            } else {
                a = row[n], b = row[n + 1];
            }
            f(n, a);
            f(n + 1, b);
        } else if (n < c1) {
            f(n, row[n]);
        }
    }
}

struct PartPlace {
    const double* row;   // the map row of this workgroup
    bool aligned;        // ... starts on a 16-byte boundary
    int r, c0, c1;
    size_t slot;         // where the part's result goes: [PRN][row][part of the row]
};
__device__ __forceinline__ PartPlace part_place(const double* __restrict__ map, int rows, int N) {
    PartPlace p;
    const int prn = blockIdx.z;
    p.r = blockIdx.x;
    p.c0 = blockIdx.y * kDetectPartCells;
    p.c1 = p.c0 + kDetectPartCells < N ? p.c0 + kDetectPartCells : N;
    const size_t first = ((size_t)prn * rows + p.r) * N;
    p.row = map + first;
    p.aligned = (first & 1) == 0;       // (the map itself is a device allocation: 256-byte aligned)
    p.slot = ((size_t)prn * rows + p.r) * gridDim.y + blockIdx.y;
    return p;
}

__global__ __launch_bounds__(64) void detect_seed_kernel(int n_prn, const long long* __restrict__ row0,
                                                         const long long* __restrict__ code0, const double* __restrict__ value0,
                                                         DeepDetectPeak* __restrict__ peaks) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_prn) return;
    DeepDetectPeak o;
    o.row = (int32_t)row0[p];
    o.code = (int32_t)code0[p];
    o.value = value0[p];
    peaks[(size_t)p * kDetectMaxPeaks] = o;
}

__global__ __launch_bounds__(kThreads) void detect_argmax_part_kernel(const double* __restrict__ map, int rows, int nbins, int N,
                                                                      int k, int excl_code, int excl_bins,
                                                                      const DeepDetectPeak* __restrict__ peaks,
                                                                      Best* __restrict__ parts) {
    __shared__ Best sh[kWaves];
    const PartPlace pl = part_place(map, rows, N);
    const Zones z = part_zones<true>(peaks + (size_t)blockIdx.z * kDetectMaxPeaks, k, pl.r % nbins, nbins, pl.c0, pl.c1, N,
                                     excl_code, excl_bins);
    const long long base = (long long)pl.r * N;
    Best mine = {-1.0, 0x7fffffffffffffffLL};
    if (z.mask == 0) {
        lane_cells(pl.row, pl.aligned, pl.c0, pl.c1, [&](int n, double v) {
            const Best c = {v, base + n};
            mine = better(mine, c);
        });
    } else {
        lane_cells(pl.row, pl.aligned, pl.c0, pl.c1, [&](int n, double v) {
            const Best c = {v, base + n};
            if (!zone_hit(z, n, N, excl_code)) mine = better(mine, c);
        });
    }
    const Best r = block_best(mine, sh);
    if (threadIdx.x == 0) parts[pl.slot] = r;
}

__global__ __launch_bounds__(kThreads) void detect_argmax_finish_kernel(const Best* __restrict__ parts, long long n_parts, int N,
                                                                        int k, DeepDetectPeak* __restrict__ peaks) {
    __shared__ Best sh[kWaves];
    const int prn = blockIdx.x;
    Best mine = {-1.0, 0x7fffffffffffffffLL};
    for (long long i = threadIdx.x; i < n_parts; i += kThreads) mine = better(mine, parts[(size_t)prn * n_parts + i]);
    const Best top = block_best(mine, sh);
    if (threadIdx.x == 0) {
        DeepDetectPeak o;
        if (top.v < 0.0) {           // (every cell lay in a zone: the map's values are >= 0)
            o.row = -1, o.code = 0, o.value = 0.0;
        } else {
            o.row = (int32_t)(top.i / N);
            o.code = (int32_t)(top.i - (long long)o.row * N);
            o.value = top.v;
        }
        peaks[(size_t)prn * kDetectMaxPeaks + k] = o;
    }
}

// PASS 0: the part's sum and count of noise cells; PASS 1: its sum of (M - mean)^2 with the mean pass 0's finish left.
template <int PASS>
__global__ __launch_bounds__(kThreads) void detect_moment_part_kernel(const double* __restrict__ map, int rows, int nbins, int N,
                                                                      int n_peaks, int excl_code,
                                                                      const DeepDetectPeak* __restrict__ peaks,
                                                                      const sdr_detect_noise* __restrict__ noise,
                                                                      double* __restrict__ psum, int32_t* __restrict__ pcount) {
    __shared__ double sh[kWaves];
    __shared__ long long shc[kWaves];
    const PartPlace pl = part_place(map, rows, N);
    const Zones z = part_zones<false>(peaks + (size_t)blockIdx.z * kDetectMaxPeaks, n_peaks, 0, nbins, pl.c0, pl.c1, N,
                                      excl_code, 0);
    const double mean = PASS ? noise[blockIdx.z].mean : 0.0;
    double acc = 0.0;
    long long cnt = 0;
    auto add = [&](double v) {
        if (PASS) {
            const double d = v - mean;
            acc = acc + d * d;
        } else {
            acc = acc + v;
            ++cnt;
        }
    };
    if (z.mask == 0) {
        lane_cells(pl.row, pl.aligned, pl.c0, pl.c1, [&](int, double v) { add(v); });
    } else {
        lane_cells(pl.row, pl.aligned, pl.c0, pl.c1, [&](int n, double v) {
            if (!zone_hit(z, n, N, excl_code)) add(v);
        });
    }
    const double s = block_sum(acc, sh);
    if (PASS) {
        if (threadIdx.x == 0) psum[pl.slot] = s;
    } else {
        const long long c = block_count(cnt, shc);
        if (threadIdx.x == 0) {
            psum[pl.slot] = s;
            pcount[pl.slot] = (int32_t)c;
        }
    }
}

// The parts of a PRN added in ascending order: lane t adds its run of ceil(n_parts / 256) consecutive parts, the runs are
// added as block_sum adds -- an order that depends on n_parts alone.
template <int PASS>
__global__ __launch_bounds__(kThreads) void detect_moment_finish_kernel(const double* __restrict__ psum,
                                                                        const int32_t* __restrict__ pcount, long long n_parts,
                                                                        sdr_detect_noise* __restrict__ noise) {
    __shared__ double sh[kWaves];
    __shared__ long long shc[kWaves];
    const int prn = blockIdx.x;
    const long long run = (n_parts + kThreads - 1) / kThreads;
    const long long lo = threadIdx.x * run, hi = lo + run < n_parts ? lo + run : n_parts;
    double acc = 0.0;
    long long cnt = 0;
    for (long long i = lo; i < hi; ++i) {
        acc = acc + psum[(size_t)prn * n_parts + i];
        if (!PASS) cnt += pcount[(size_t)prn * n_parts + i];
    }
    const double s = block_sum(acc, sh);
    if (PASS) {
        if (threadIdx.x == 0) noise[prn].variance = s / (double)noise[prn].n_cells;
    } else {
        const long long c = block_count(cnt, shc);
        if (threadIdx.x == 0) {
            noise[prn].n_cells = c;
            noise[prn].mean = s / (double)c;
            noise[prn].variance = 0.0;
        }
    }
}

constexpr size_t align16(size_t b) { return (b + 15) / 16 * 16; }

}  // namespace

size_t sdr_deep_detect_bytes(int n_prn, int rows, int N) {
    const size_t n_parts = (size_t)n_prn * rows * detect_row_parts(N);
    return align16((size_t)n_prn * kDetectMaxPeaks * sizeof(DeepDetectPeak)) + align16((size_t)n_prn * sizeof(sdr_detect_noise)) +
           n_parts * sizeof(Best);      // (a pass's partials: a Best, or a double and an int32, per part)
}

DeepDetectWs sdr_deep_detect_ws(void* buf, int n_prn) {
    DeepDetectWs ws;
    char* p = (char*)buf;
    ws.peaks = (DeepDetectPeak*)p;
    p += align16((size_t)n_prn * kDetectMaxPeaks * sizeof(DeepDetectPeak));
    ws.noise = (sdr_detect_noise*)p;
    p += align16((size_t)n_prn * sizeof(sdr_detect_noise));
    ws.parts = p;
    return ws;
}

int sdr_deep_detect(sdr_engine* e, const double* map, int n_prn, int rows, int nbins, int N, const sdr_detect_cfg* det,
                    const long long* row0, const long long* code0, const double* value0, const DeepDetectWs& ws) {
    if (!det || n_prn < 1 || n_prn > 65535 || rows < 1 || nbins < 1 || rows % nbins || N < 2 || det->n_peaks < 1 ||
        det->n_peaks > kDetectMaxPeaks || det->excl_code < 0 || det->excl_bins < 0 ||
        !detect_windows_fit(det->n_peaks, det->excl_code, N))
        return sdr_fail(SDR_ERR_INVALID, "bad detection request");
    const int row_parts = detect_row_parts(N);
    if (row_parts > 65535) return sdr_fail(SDR_ERR_UNSUPPORTED, "map rows too long");
    const long long n_parts = (long long)rows * row_parts;
    const dim3 grid(rows, row_parts, n_prn), block(kThreads);
    {
        ProfScope ps(e, "deep_detect_peaks");
        hipLaunchKernelGGL(detect_seed_kernel, dim3((n_prn + 63) / 64), dim3(64), 0, e->stream, n_prn, row0, code0, value0, ws.peaks);
        for (int k = 1; k < det->n_peaks; ++k) {
            hipLaunchKernelGGL(detect_argmax_part_kernel, grid, block, 0, e->stream, map, rows, nbins, N, k, det->excl_code,
                               det->excl_bins, (const DeepDetectPeak*)ws.peaks, (Best*)ws.parts);
            hipLaunchKernelGGL(detect_argmax_finish_kernel, dim3(n_prn), block, 0, e->stream, (const Best*)ws.parts, n_parts, N, k,
                               ws.peaks);
        }
        SDR_HIP(hipGetLastError());
    }
    {
        ProfScope ps(e, "deep_detect_noise");
        double* psum = (double*)ws.parts;
        int32_t* pcount = (int32_t*)(psum + (size_t)n_prn * n_parts);
        hipLaunchKernelGGL(detect_moment_part_kernel<0>, grid, block, 0, e->stream, map, rows, nbins, N, det->n_peaks, det->excl_code,
                           (const DeepDetectPeak*)ws.peaks, (const sdr_detect_noise*)ws.noise, psum, pcount);
        hipLaunchKernelGGL(detect_moment_finish_kernel<0>, dim3(n_prn), block, 0, e->stream, (const double*)psum,
                           (const int32_t*)pcount, n_parts, ws.noise);
        hipLaunchKernelGGL(detect_moment_part_kernel<1>, grid, block, 0, e->stream, map, rows, nbins, N, det->n_peaks, det->excl_code,
                           (const DeepDetectPeak*)ws.peaks, (const sdr_detect_noise*)ws.noise, psum, pcount);
        hipLaunchKernelGGL(detect_moment_finish_kernel<1>, dim3(n_prn), block, 0, e->stream, (const double*)psum,
                           (const int32_t*)pcount, n_parts, ws.noise);
        SDR_HIP(hipGetLastError());
    }
    return SDR_OK;
}
