// What the ring holds, looked at where it lies (sdr_iq_probe, include/sydr_amd.h): level statistics, a histogram per
// component and a Welch power spectral density of a window of the ring, in one call that reads the ring and writes nothing
// into it.
//
// probe_moments_int_kernel<FMT, HIST> / probe_moments_float_kernel<FMT>  grid-stride over the 16-byte granules of the window
//   (probe_window.h: one or two pieces, a ragged head and tail masked sample by sample), one plain dwordx4 load per granule
//   and lane.
//   Integer rings: every sum is an exact integer.  A lane adds into 32-bit registers and moves them into 64-bit ones every
//   kFlush granules (the bound is derived at kFlush); lanes are added across the wave and the workgroup, then ONE set of
//   64-bit integer atomics per workgroup -- integer adds commute, so the result does not depend on who arrives first.
//   The histogram is kHistCopies interleaved tables in LDS, a lane adding into copy (lane & 15): a 1- or 2-bit recording has
//   two or four distinct values per component, and with one table all 64 lanes of a wave would queue on the same two to
//   four counters; here 16 lanes that see the same value hit 16 different banks and only lanes l, l + 16, l + 32, l + 48
//   share a counter.  The copies are added per bin and flushed with one 64-bit atomic per non-empty bin and workgroup.
//   Float rings: a sample with a NaN / Inf component is counted and left out; fp64 partial sums per lane in stride order,
//   added across the wave by a fixed butterfly and across the waves in wave order; one row per workgroup goes to a slab
//   with plain stores and probe_moments_finish_kernel adds the rows (at most 512, staged in LDS) in workgroup order.  No
//   float atomics.
// probe_psd_kernel<FMT>  Welch: workgroup g transforms segments g, g + G, g + 2G, ... in LDS (nfft complex fp64: 64 KB at
//   4096), samples widened and multiplied by the periodic Hann window on the way in; an in-place radix-2
//   decimation-in-frequency transform (twiddles from an fp64 table made on the host once per nfft and kept on the engine)
//   leaves the spectrum in bit-reversed order, |X|^2 is added per LDS position in registers, segment after segment, and
//   the partial row is written un-reversed.  probe_psd_reduce_kernel adds the rows in workgroup order and divides by
//   S * fs * sum w^2 last.  Neighbouring segments share half their samples; they are loaded again (not measured against
//   keeping them).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "correlator.h"
#include "fft_lds.h"
#include "probe_window.h"

namespace {

using namespace sdr;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kHistBins = 256;
constexpr int kHistCopies = 16;
constexpr size_t kHistLds = (size_t)2 * kHistBins * kHistCopies * sizeof(unsigned);   // 32 KB
constexpr size_t kScratchLds = (size_t)kWaves * 16 * sizeof(double);                  // the waves' sums
// Granules a lane takes between two moves of its 32-bit sums into the 64-bit ones.  What 32 bits would bear:
//   ci8 : 8 samples a granule, |x| <= 2^7: in 1024 granules |sum x| <= 2^13 * 2^7 = 2^20, sum x^2 and |sum I*Q| <= 2^13 * 2^14
//         = 2^27 < 2^31.
//   ci16: 4 samples a granule, |x| <= 2^15: in 1024 granules |sum x| <= 2^12 * 2^15 = 2^27 < 2^31.  x^2 and |I*Q| reach 2^30:
//         TWO of them are 2^31, so those go into 64-bit registers from the first sample on.
// The move is five 64-bit adds against ~20 instructions for each of a granule's samples, so it is made every 4 granules
// already (1 % of the loop): a lane of the grids launched here sees 4 .. 16 granules of a second at 25 MHz and would never
// reach 1024 -- the move has to run in the tests and in every large window, not first in a window of gigabytes.
// Counters: a lane's rail count and an LDS histogram counter are at most the components of one kind in the window,
// <= 2^31 < 2^32 (unsigned); everything that crosses lanes is 64-bit.
constexpr int kFlush = 4;
static_assert(kFlush <= 1024, "see the bound above");
constexpr int kBias = 32768;   // minimum and maximum travel through unsigned atomicMax: x + kBias + 1 and kBias - x (0 = none yet)

struct ProbeDev {   // zeroed in front of the moments launch
    long long sum[2], sq[2], iq, rail[2], nonfinite;
    unsigned umax[2], uneg[2];
    int psd_bad, pad[3];
    double fsum[2], fsq[2], fiq, fmin[2], fmax[2];   // float rings: written by probe_moments_finish_kernel
};
constexpr size_t kDevBytes = 256;
static_assert(sizeof(ProbeDev) <= kDevBytes, "the result block has 256 bytes of the workspace");
constexpr int kSlabCols = 16;   // doubles per workgroup row: sum[2], sq[2], iq, min[2], max[2]

template <int FMT>
struct IntFmt;
template <>
struct IntFmt<SDR_FMT_CI8> {
    static constexpr int kSpg = ring_granule_samples(SDR_FMT_CI8), kLo = -128, kHi = 127;
    typedef int wide;
    static __device__ __forceinline__ void get(const uint4& v, int j, int& xi, int& xq) {
        const unsigned w = (j >> 1) == 0 ? v.x : (j >> 1) == 1 ? v.y : (j >> 1) == 2 ? v.z : v.w;
        const unsigned h = (j & 1) ? w >> 16 : w;
        xi = (int)(h & 0xffu) - ring_fill_byte(SDR_FMT_CI8);   // (the ring's bytes are u = x + 128)
        xq = (int)((h >> 8) & 0xffu) - ring_fill_byte(SDR_FMT_CI8);
    }
    static __device__ __forceinline__ int bin(int x, int) { return x + 128; }   // the stored byte IS the bin
};
template <>
struct IntFmt<SDR_FMT_CI16> {
    static constexpr int kSpg = ring_granule_samples(SDR_FMT_CI16), kLo = -32768, kHi = 32767;
    typedef long long wide;
    static __device__ __forceinline__ void get(const uint4& v, int j, int& xi, int& xq) {
        const int w = (int)(j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w);
        xi = (int)(short)(w & 0xffff);
        xq = w >> 16;
    }
    static __device__ __forceinline__ int bin(int x, int shift) {
        const int b = (x >> shift) + 128;
        return b < 0 ? 0 : b > 255 ? 255 : b;
    }
};

__device__ __forceinline__ long long wave_add(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double wave_add(double v) {   // a fixed butterfly: the same bits every time
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ bool finite64(double x) { return (__double2hiint(x) & 0x7ff00000) != 0x7ff00000; }

template <int FMT, bool HIST>
__global__ __launch_bounds__(kThreads) void probe_moments_int_kernel(const uint4* __restrict__ ring, ProbeWindow W, int hist_shift,
                                                                      ProbeDev* __restrict__ dev,
                                                                      unsigned long long* __restrict__ hist) {
    typedef IntFmt<FMT> F;
    typedef typename F::wide wide;
    extern __shared__ __attribute__((aligned(16))) char probe_lds[];
    long long* scratch = reinterpret_cast<long long*>(probe_lds);
    unsigned* table = reinterpret_cast<unsigned*>(probe_lds + kScratchLds);   // [component][bin][copy]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (HIST) {
        for (int q = tid; q < 2 * kHistBins * kHistCopies; q += kThreads) table[q] = 0u;
        __syncthreads();
    }
    const int copy = lane & (kHistCopies - 1);

    int s[2] = {0, 0};
    wide q[2] = {0, 0}, p = 0;
    long long S[2] = {0, 0}, Q[2] = {0, 0}, P = 0;
    unsigned rail[2] = {0u, 0u};
    int mn[2] = {F::kHi, F::kHi}, mx[2] = {F::kLo, F::kLo};
    auto take = [&](int xi, int xq) {
        s[0] += xi, s[1] += xq;
        q[0] += (wide)(xi * xi), q[1] += (wide)(xq * xq);
        p += (wide)(xi * xq);
        mn[0] = min(mn[0], xi), mx[0] = max(mx[0], xi);
        mn[1] = min(mn[1], xq), mx[1] = max(mx[1], xq);
        rail[0] += (unsigned)(xi == F::kLo || xi == F::kHi);
        rail[1] += (unsigned)(xq == F::kLo || xq == F::kHi);
        if (HIST) {
            atomicAdd(&table[F::bin(xi, hist_shift) * kHistCopies + copy], 1u);
            atomicAdd(&table[(kHistBins + F::bin(xq, hist_shift)) * kHistCopies + copy], 1u);
        }
    };
    auto flush = [&]() {
        S[0] += s[0], S[1] += s[1], Q[0] += q[0], Q[1] += q[1], P += p;
        s[0] = s[1] = 0, q[0] = q[1] = 0, p = 0;
    };

    const int64_t stride = (int64_t)gridDim.x * kThreads;
    int since = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < W.total; i += stride) {
        int64_t lo, hi;
        const int64_t g = probe_granule(W, i, F::kSpg, &lo, &hi);
        const uint4 v = ring[g];
        if (hi - lo == F::kSpg) {
#pragma unroll
            for (int j = 0; j < F::kSpg; ++j) {
                int xi, xq;
                F::get(v, j, xi, xq);
                take(xi, xq);
            }
        } else {   // the ragged head or tail of a piece
            const int64_t s0 = g * F::kSpg;
#pragma unroll
            for (int j = 0; j < F::kSpg; ++j) {
                int xi, xq;
                F::get(v, j, xi, xq);
                if (s0 + j >= lo && s0 + j < hi) take(xi, xq);
            }
        }
        if (++since == kFlush) {
            flush();
            since = 0;
        }
    }
    flush();

    // lanes -> wave -> workgroup -> one set of atomics
    long long sums[7] = {S[0], S[1], Q[0], Q[1], P, (long long)rail[0], (long long)rail[1]};
#pragma unroll
    for (int k = 0; k < 7; ++k) sums[k] = wave_add(sums[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            mn[c] = min(mn[c], __shfl_xor(mn[c], d));
            mx[c] = max(mx[c], __shfl_xor(mx[c], d));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) scratch[wave * 16 + k] = sums[k];
#pragma unroll
        for (int c = 0; c < 2; ++c) scratch[wave * 16 + 8 + c] = mn[c], scratch[wave * 16 + 10 + c] = mx[c];
    }
    __syncthreads();
    if (tid < 7) {
        long long t = 0;
        for (int w = 0; w < kWaves; ++w) t += scratch[w * 16 + tid];
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(tid < 2 ? &dev->sum[tid] : tid < 4 ? &dev->sq[tid - 2]
                                                                              : tid == 4 ? &dev->iq : &dev->rail[tid - 5]);
        atomicAdd(dst, (unsigned long long)t);   // (two's complement: the signed sum)
    } else if (tid >= 8 && tid < 12) {
        const bool is_min = tid < 10;
        const int c = tid & 1;
        long long t = scratch[tid];
        for (int w = 1; w < kWaves; ++w) t = is_min ? min(t, scratch[w * 16 + tid]) : max(t, scratch[w * 16 + tid]);
        if (is_min)
            atomicMax(&dev->uneg[c], (unsigned)(kBias - (int)t));
        else
            atomicMax(&dev->umax[c], (unsigned)((int)t + kBias + 1));
    }
    if (HIST) {   // (the table is complete: the barrier above is behind every lane's last add)
        for (int b = tid; b < 2 * kHistBins; b += kThreads) {
            unsigned long long t = 0;
#pragma unroll
            for (int k = 0; k < kHistCopies; ++k) t += table[b * kHistCopies + ((k + tid) & (kHistCopies - 1))];
            if (t) atomicAdd(&hist[b], t);
        }
    }
}

template <int FMT>
__global__ __launch_bounds__(kThreads) void probe_moments_float_kernel(const uint4* __restrict__ ring, ProbeWindow W,
                                                                        ProbeDev* __restrict__ dev, double* __restrict__ slab) {
    constexpr int kSpg = ring_granule_samples(FMT);
    extern __shared__ __attribute__((aligned(16))) char probe_lds[];
    double* scratch = reinterpret_cast<double*>(probe_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_huge_val();
    double s[2] = {0.0, 0.0}, q[2] = {0.0, 0.0}, p = 0.0, mn[2] = {inf, inf}, mx[2] = {-inf, -inf};
    long long bad = 0;
    auto take = [&](double xi, double xq) {
        if (finite64(xi) && finite64(xq)) {
            s[0] += xi, s[1] += xq;
            q[0] += xi * xi, q[1] += xq * xq;
            p += xi * xq;
            mn[0] = fmin(mn[0], xi), mx[0] = fmax(mx[0], xi);
            mn[1] = fmin(mn[1], xq), mx[1] = fmax(mx[1], xq);
        } else {
            ++bad;
        }
    };
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + tid; i < W.total; i += stride) {
        int64_t lo, hi;
        const int64_t g = probe_granule(W, i, kSpg, &lo, &hi);
        const uint4 v = ring[g];
        if (FMT == SDR_FMT_CF32) {
            const int64_t s0 = g * 2;
            if (s0 >= lo) take((double)__uint_as_float(v.x), (double)__uint_as_float(v.y));
            if (s0 + 1 < hi) take((double)__uint_as_float(v.z), (double)__uint_as_float(v.w));
        } else {
            take(__hiloint2double((int)v.y, (int)v.x), __hiloint2double((int)v.w, (int)v.z));
        }
    }
    double vals[5] = {s[0], s[1], q[0], q[1], p};
#pragma unroll
    for (int k = 0; k < 5; ++k) vals[k] = wave_add(vals[k]);
    bad = wave_add(bad);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            mn[c] = fmin(mn[c], __shfl_xor(mn[c], d));
            mx[c] = fmax(mx[c], __shfl_xor(mx[c], d));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) scratch[wave * 16 + k] = vals[k];
#pragma unroll
        for (int c = 0; c < 2; ++c) scratch[wave * 16 + 5 + c] = mn[c], scratch[wave * 16 + 7 + c] = mx[c];
        if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(&dev->nonfinite), (unsigned long long)bad);
    }
    __syncthreads();
    if (tid < 9) {
        double t = scratch[tid];
        for (int w = 1; w < kWaves; ++w) {
            const double o = scratch[w * 16 + tid];
            t = tid < 5 ? t + o : tid < 7 ? fmin(t, o) : fmax(t, o);
        }
        slab[(size_t)blockIdx.x * kSlabCols + tid] = t;
    }
}

// The workgroups' rows, added in workgroup order: all lanes bring the rows into LDS (a lane that fetched row after row from
// HBM itself would wait out one memory latency per row), then one lane per column adds them in ascending order.
constexpr int kMaxFloatRows = 512;
constexpr int kFinishCols = 9;
__global__ __launch_bounds__(kThreads) void probe_moments_finish_kernel(const double* __restrict__ slab, int rows, ProbeDev* __restrict__ dev) {
    __shared__ double staged[kMaxFloatRows * kFinishCols];
    for (int q = threadIdx.x; q < rows * kFinishCols; q += kThreads) staged[q] = slab[(size_t)(q / kFinishCols) * kSlabCols + q % kFinishCols];
    __syncthreads();
    const int c = threadIdx.x;
    if (c >= kFinishCols) return;
    double t = staged[c];
    for (int r = 1; r < rows; ++r) {
        const double o = staged[r * kFinishCols + c];
        t = c < 5 ? t + o : c < 7 ? fmin(t, o) : fmax(t, o);
    }
    double* dst = c < 2 ? &dev->fsum[c] : c < 4 ? &dev->fsq[c - 2] : c == 4 ? &dev->fiq : c < 7 ? &dev->fmin[c - 5] : &dev->fmax[c - 7];
    *dst = t;
}

constexpr int kMaxNfft = kFftLdsMax, kMinNfft = kFftLdsMin;
constexpr int kPsdRegs = kMaxNfft / kThreads;   // LDS positions of a lane: tid + 256 * r

template <int FMT>
__global__ __launch_bounds__(kThreads) void probe_psd_kernel(const void* __restrict__ ring, int64_t capacity, int64_t base, int64_t n_seg,
                                                             int nfft, int log2n, const double2* __restrict__ tw,
                                                             const double* __restrict__ win, double* __restrict__ rows,
                                                             ProbeDev* __restrict__ dev) {
    extern __shared__ __attribute__((aligned(16))) char probe_lds[];
    double2* x = reinterpret_cast<double2*>(probe_lds);
    const int tid = threadIdx.x;
    double acc[kPsdRegs];
#pragma unroll
    for (int r = 0; r < kPsdRegs; ++r) acc[r] = 0.0;
    bool bad = false;
    for (int64_t s = blockIdx.x; s < n_seg; s += gridDim.x) {
        for (int j = tid; j < nfft; j += kThreads) {
            const double2 v = ring_read<FMT>(ring, probe_segment_sample(base, capacity, s, nfft, j));
            bad |= !(finite64(v.x) && finite64(v.y));
            const double w = win[j];
            x[j] = make_double2(w * v.x, w * v.y);
        }
        __syncthreads();
        fft_lds_forward<kThreads>(x, nfft, tw, tid);   // X[k] ends at position bitrev(k)
#pragma unroll
        for (int r = 0; r < kPsdRegs; ++r) {
            const int j = tid + kThreads * r;
            if (j < nfft) {
                const double2 v = x[j];
                acc[r] += __builtin_fma(v.x, v.x, v.y * v.y);
            }
        }
        __syncthreads();   // (the next segment overwrites x)
    }
#pragma unroll
    for (int r = 0; r < kPsdRegs; ++r) {
        const int j = tid + kThreads * r;
        if (j < nfft) rows[(size_t)blockIdx.x * nfft + (__brev((unsigned)j) >> (32 - log2n))] = acc[r];
    }
    if (bad) atomicOr(&dev->psd_bad, 1);
}

// The workgroups' rows in workgroup order, the scale last; NaN everywhere when a used segment held a non-finite sample.
__global__ __launch_bounds__(kThreads) void probe_psd_reduce_kernel(const double* __restrict__ rows, int n_rows, int nfft, double den,
                                                                    const ProbeDev* __restrict__ dev, double* __restrict__ psd) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= nfft) return;
    double t = rows[k];
#pragma unroll 8
    for (int r = 1; r < n_rows; ++r) t += rows[(size_t)r * nfft + k];   // (ascending; the loads do not wait for the adds)
    psd[k] = dev->psd_bad ? __builtin_nan("") : t / den;
}

// exp(-2j*pi*k/nfft), k < nfft / 2, then the periodic Hann window; made once per nfft, kept on the engine
int probe_tables(sdr_engine* e, int nfft) {
    if (e->probe_tab_nfft == nfft && e->probe_tab.ptr) return SDR_OK;
    e->probe_tab_nfft = 0;
    const size_t b_tw = (size_t)(nfft / 2) * sizeof(double2), b_win = (size_t)nfft * sizeof(double);
    if (int rc = sdr_devbuf_reserve(e, &e->probe_tab, b_tw + b_win)) return rc;
    std::vector<double> host(nfft + nfft);
    const double sumw2 = fft_lds_fill_tables(nfft, host.data());
    SDR_HIP(hipStreamSynchronize(e->stream));
    SDR_HIP(hipMemcpy(e->probe_tab.ptr, host.data(), b_tw + b_win, hipMemcpyHostToDevice));
    e->probe_sumw2 = sumw2;
    e->probe_tab_nfft = nfft;
    return SDR_OK;
}

}  // namespace

extern "C" {

int sdr_iq_probe(sdr_engine* e, int64_t start_sample, int64_t n_samples, int hist_shift, int nfft, double fs, sdr_probe_result* res,
                 int64_t* hist, double* psd) {
    if (int rc = sdr_set_device(e)) return rc;   // (a resident tick server leaves, a parked slab goes into the ring)
    if (!res) return sdr_fail(SDR_ERR_INVALID, "no result block for the probe");
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    const int fmt = e->iq_fmt;
    const bool integer = fmt == SDR_FMT_CI8 || fmt == SDR_FMT_CI16;
    if (n_samples < 1) return sdr_fail(SDR_ERR_INVALID, "a window of %lld samples", (long long)n_samples);
    if (hist_shift < 0) return sdr_fail(SDR_ERR_INVALID, "negative hist_shift %d", hist_shift);
    if (integer && hist_shift > (fmt == SDR_FMT_CI8 ? 0 : 8))
        return sdr_fail(SDR_ERR_INVALID, "hist_shift %d: a %s ring takes 0..%d", hist_shift, fmt == SDR_FMT_CI8 ? "ci8" : "ci16",
                        fmt == SDR_FMT_CI8 ? 0 : 8);
    int log2n = 0;
    if (psd) {
        if (nfft < kMinNfft || nfft > kMaxNfft || (nfft & (nfft - 1)))
            return sdr_fail(SDR_ERR_INVALID, "nfft %d is not a power of two in %d..%d", nfft, kMinNfft, kMaxNfft);
        if (!(fs > 0.0) || !std::isfinite(fs)) return sdr_fail(SDR_ERR_INVALID, "bad sampling frequency");
        if (n_samples < nfft) return sdr_fail(SDR_ERR_INVALID, "a window of %lld samples holds no segment of %d", (long long)n_samples, nfft);
        while ((1 << log2n) < nfft) ++log2n;
    }
    if (hist && !integer) return sdr_fail(SDR_ERR_UNSUPPORTED, "no histogram of a float ring");
    if (n_samples > ((int64_t)1 << 31)) return sdr_fail(SDR_ERR_UNSUPPORTED, "a window of %lld samples (at most 2^31)", (long long)n_samples);
    if (start_sample < 0) return sdr_fail(SDR_ERR_RANGE, "negative start_sample");
    if (n_samples > e->iq_capacity)
        return sdr_fail(SDR_ERR_RANGE, "a window of %lld samples, ring holds %lld", (long long)n_samples, (long long)e->iq_capacity);

    const int64_t base = start_sample % e->iq_capacity;
    const int spg = sdr::ring_granule_samples(fmt);
    const ProbeWindow W = probe_window(base, n_samples, e->iq_capacity, spg);
    // (with a histogram fewer, longer-lived workgroups: each flushes up to 512 bins)
    const int64_t want = (W.total + kThreads * 4 - 1) / (kThreads * 4);
    // (float rings: at most kMaxFloatRows rows for probe_moments_finish_kernel to add)
    const int64_t most = integer ? (int64_t)std::max(e->n_cus, 1) * (hist ? 2 : 4) : std::min<int64_t>(2LL * std::max(e->n_cus, 1), kMaxFloatRows);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, most));
    const int64_t n_seg = psd ? probe_segments(n_samples, nfft) : 0;
    const int psd_grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_seg, 2LL * std::max(e->n_cus, 1)));

    if (psd)
        if (int rc = probe_tables(e, nfft)) return rc;
    // one workspace: [result block][histogram][moment rows][spectrum rows][spectrum]
    const size_t b_hist = (size_t)2 * kHistBins * sizeof(unsigned long long);
    const size_t b_slab = integer ? 0 : (size_t)grid * kSlabCols * sizeof(double);
    const size_t b_rows = psd ? (size_t)psd_grid * nfft * sizeof(double) : 0;
    const size_t b_psd = psd ? (size_t)nfft * sizeof(double) : 0;
    if (int rc = sdr_devbuf_reserve(e, &e->probe_ws, kDevBytes + b_hist + b_slab + b_rows + b_psd)) return rc;
    char* ws = (char*)e->probe_ws.ptr;
    ProbeDev* d_dev = (ProbeDev*)ws;
    unsigned long long* d_hist = (unsigned long long*)(ws + kDevBytes);
    double* d_slab = (double*)(ws + kDevBytes + b_hist);
    double* d_rows = (double*)(ws + kDevBytes + b_hist + b_slab);
    double* d_psd = (double*)(ws + kDevBytes + b_hist + b_slab + b_rows);
    e->probe_host.resize(kDevBytes + b_hist);

    if (int rc = sdr_iq_order_reader(e, &e->ctx0)) return rc;   // (behind the uploads queued on the engine's stream so far)
    const uint4* ring16 = (const uint4*)e->iq;
    {
        ProfScope whole(e, "call_iq_probe");
        {
            ProfScope ps(e, "probe_moments_kernel");
            SDR_HIP(hipMemsetAsync(ws, 0, kDevBytes + (hist ? b_hist : 0), e->stream));
            if (integer) {
                const void* kernel =
                    fmt == SDR_FMT_CI8
                        ? (hist ? (const void*)probe_moments_int_kernel<SDR_FMT_CI8, true> : (const void*)probe_moments_int_kernel<SDR_FMT_CI8, false>)
                        : (hist ? (const void*)probe_moments_int_kernel<SDR_FMT_CI16, true> : (const void*)probe_moments_int_kernel<SDR_FMT_CI16, false>);
                ProbeWindow w = W;
                void* args[] = {&ring16, &w, &hist_shift, &d_dev, &d_hist};
                SDR_HIP(hipLaunchKernel(kernel, dim3((unsigned)grid), dim3(kThreads), args, kScratchLds + (hist ? kHistLds : 0), e->stream));
            } else {
                const void* kernel = fmt == SDR_FMT_CF32 ? (const void*)probe_moments_float_kernel<SDR_FMT_CF32>
                                                         : (const void*)probe_moments_float_kernel<SDR_FMT_CF64>;
                ProbeWindow w = W;
                void* args[] = {&ring16, &w, &d_dev, &d_slab};
                SDR_HIP(hipLaunchKernel(kernel, dim3((unsigned)grid), dim3(kThreads), args, kScratchLds, e->stream));
                hipLaunchKernelGGL(probe_moments_finish_kernel, dim3(1), dim3(kThreads), 0, e->stream, (const double*)d_slab, grid, d_dev);
                SDR_HIP(hipGetLastError());
            }
        }
        if (psd) {
            ProfScope ps(e, "probe_psd_kernel");
            const void* kernel = sdr::with_fmt(fmt, [](auto f) { return (const void*)probe_psd_kernel<decltype(f)::value>; });
            const void* ring = e->iq;
            int64_t capacity = e->iq_capacity, b = base, ns = n_seg;
            const double2* tw = (const double2*)e->probe_tab.ptr;
            const double* win = (const double*)((const char*)e->probe_tab.ptr + (size_t)(nfft / 2) * sizeof(double2));
            void* args[] = {&ring, &capacity, &b, &ns, &nfft, &log2n, &tw, &win, &d_rows, &d_dev};
            SDR_HIP(hipLaunchKernel(kernel, dim3((unsigned)psd_grid), dim3(kThreads), args, (size_t)nfft * sizeof(double2), e->stream));
            const double den = ((double)n_seg * fs) * e->probe_sumw2;
            hipLaunchKernelGGL(probe_psd_reduce_kernel, dim3((unsigned)((nfft + kThreads - 1) / kThreads)), dim3(kThreads), 0, e->stream,
                               (const double*)d_rows, psd_grid, nfft, den, (const ProbeDev*)d_dev, d_psd);
            SDR_HIP(hipGetLastError());
        }
    }
    SDR_HIP(hipMemcpyAsync(e->probe_host.data(), ws, kDevBytes + (hist ? b_hist : 0), hipMemcpyDeviceToHost, e->stream));
    if (psd) SDR_HIP(hipMemcpyAsync(psd, d_psd, b_psd, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));

    ProbeDev dev;
    memcpy(&dev, e->probe_host.data(), sizeof(dev));
    sdr_probe_result r;
    memset(&r, 0, sizeof(r));
    r.n_samples = n_samples;
    r.n_segments = n_seg;
    if (integer) {
        for (int c = 0; c < 2; ++c) {
            r.n_rail[c] = dev.rail[c];
            r.min[c] = (double)(kBias - (int)dev.uneg[c]);
            r.max[c] = (double)((int)dev.umax[c] - 1 - kBias);
            r.sum[c] = (double)dev.sum[c];   // (one rounding, to nearest even)
            r.sum_sq[c] = (double)dev.sq[c];
        }
        r.sum_iq = (double)dev.iq;
    } else {
        r.n_nonfinite = dev.nonfinite;
        const bool none = dev.nonfinite >= n_samples;
        for (int c = 0; c < 2; ++c) {
            r.min[c] = none ? std::numeric_limits<double>::quiet_NaN() : dev.fmin[c];
            r.max[c] = none ? std::numeric_limits<double>::quiet_NaN() : dev.fmax[c];
            r.sum[c] = dev.fsum[c];
            r.sum_sq[c] = dev.fsq[c];
        }
        r.sum_iq = dev.fiq;
    }
    *res = r;
    if (hist) memcpy(hist, e->probe_host.data() + kDevBytes, b_hist);
    return SDR_OK;
}

}  // extern "C"
