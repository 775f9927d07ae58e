// Pulse blanking and narrow-band excision between the down-converter's fp64 output and the ring's format
// (sdr_ddc_mitigate, include/sydr_amd.h).  What the ring must hold is stated in sydr_amd/signal/mitigate.py; which values a
// push needs, which segments it transforms, which of them it counts and where its outputs land is mit_plan.h.
//
// With a mitigator attached the converter kernel (ddc.hip) writes its outputs as cf64 behind the kept state in a linear work
// buffer W = [the last K values of v][this push's v].  Behind it on the engine's stream:
// mit_blank_kernel    a workgroup per tile of kMitBlankTile u: the triggers of the tile and of its hold / lead halo into LDS
//   (p = re*re + im*im with explicitly rounded products and sum), an exclusive prefix count over them, so that "any trigger
//   within hold behind .. lead ahead" is one difference of two counts; u = 0 or v goes to a second buffer U.
// mit_excise_kernel   a workgroup per segment, N complex fp64 in LDS: windowed on the way in, the probe's
//   decimation-in-frequency pass (fft_lds.h), the gate applied where the bins lie -- bit-reversed, the limit read at the
//   reversed index --, a decimation-in-time inverse straight back to natural order, times 1 / N, into the segment buffer B.
//   A segment is a function of its N inputs alone: whichever push recomputes it finds the same bits.
// mit_combine_kernel  y = one sample of each of the two segments an output lies in (or u without the excisor), the ring's
//   format, the store at (ring_offset + i) mod capacity; zero for the stream's first L outputs.
// The state for the next push -- W's last K values -- is copied into the OTHER of two work buffers, which the next push then
// extends: no kernel reads what another workgroup of the same launch writes.  Counters are 64-bit integer atomics (they
// commute); a push counts only the u it delivers and the segments that finish in it (mit_plan.h), so every one is counted
// once however the stream was cut.
#include "mitigate.h"

#include <cmath>
#include <new>
#include <vector>

#include "fft_lds.h"
#include "mit_plan.h"

namespace sdr {

struct Mitigator {
    int N = 0, log2n = 0, lead = 0, hold = 0;
    bool blank = false;
    double level2 = 0.0;
    int64_t K = 0;
    void* tab = nullptr;            // device: [N / 2] twiddles, [N] window, [N] limits (excisor only)
    unsigned long long* counters = nullptr;   // device: triggers, blanked, then bins[N]
    DevBuf work[2];                 // W; work[cur] holds the state in its first K samples
    int cur = 0;
    DevBuf u, seg;                  // U (blanker only), B
};

namespace {

constexpr int kCounterHead = 2;

__device__ __forceinline__ int wave_add_int(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

constexpr int kBlankSpan = kMitBlankTile + 2 * kMitMaxReach;   // triggers a workgroup looks at, at most

__global__ __launch_bounds__(kMitThreads) void mit_blank_kernel(const double2* __restrict__ W, double2* __restrict__ U, MitPlan p,
                                                                double level2, unsigned long long* __restrict__ counters) {
    __shared__ int pre[kBlankSpan + 1];      // triggers, then pre[x] = triggers among the span's first x
    __shared__ int part[kMitThreads];
    __shared__ int tally[2];
    const int tid = threadIdx.x;
    const int64_t x0 = (int64_t)blockIdx.x * kMitBlankTile;
    const int64_t left = p.n_u - x0;
    const int count = (int)(left < kMitBlankTile ? left : kMitBlankTile);
    const int reach = p.hold + p.lead, span = count + reach;          // W[x0 .. x0 + span): x0 + span <= n_u + reach = K + k
    if (tid < 2) tally[tid] = 0;
    for (int i = tid; i <= span; i += kMitThreads) {
        int t = 0;
        if (i < span) {
            const double2 v = W[x0 + i];
            t = __dadd_rn(__dmul_rn(v.x, v.x), __dmul_rn(v.y, v.y)) > level2;
        }
        pre[i] = t;
    }
    __syncthreads();
    // exclusive prefix over span + 1 entries: a run of consecutive entries per lane, the lanes' sums scanned in LDS
    const int run = (span + kMitThreads) / kMitThreads;               // ceil((span + 1) / threads)
    const int c0 = tid * run < span + 1 ? tid * run : span + 1, c1 = c0 + run < span + 1 ? c0 + run : span + 1;
    int sum = 0;
    for (int i = c0; i < c1; ++i) sum += pre[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kMitThreads; d <<= 1) {
        const int other = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += other;
        __syncthreads();
    }
    int running = part[tid] - sum;
    for (int i = c0; i < c1; ++i) {
        const int t = pre[i];
        pre[i] = running;
        running += t;
    }
    __syncthreads();
    int n_trig = 0, n_blank = 0;
    for (int o = tid; o < count; o += kMitThreads) {
        const bool b = pre[o + reach + 1] - pre[o] > 0;
        const int64_t j = p.j_lo + x0 + o;
        const double2 v = W[x0 + o + p.hold];
        U[x0 + o] = b ? make_double2(0.0, 0.0) : v;
        if (j >= p.cnt_lo && j < p.cnt_hi) {
            n_trig += pre[o + p.hold + 1] - pre[o + p.hold];
            n_blank += (int)b;
        }
    }
    n_trig = wave_add_int(n_trig), n_blank = wave_add_int(n_blank);
    if ((tid & 63) == 0) {
        if (n_trig) atomicAdd(&tally[0], n_trig);
        if (n_blank) atomicAdd(&tally[1], n_blank);
    }
    __syncthreads();
    if (tid < 2 && tally[tid]) atomicAdd(&counters[tid], (unsigned long long)tally[tid]);
}

__global__ __launch_bounds__(kMitThreads) void mit_excise_kernel(const double2* __restrict__ U, double2* __restrict__ B, MitPlan p, int log2n,
                                                                 const double2* __restrict__ tw, const double* __restrict__ win,
                                                                 const double* __restrict__ limit, unsigned long long* __restrict__ bins) {
    extern __shared__ __attribute__((aligned(16))) char mit_lds[];
    double2* x = reinterpret_cast<double2*>(mit_lds);
    const int tid = threadIdx.x, N = p.N;
    const int64_t sl = blockIdx.x, s = p.s_lo + sl;
    const double2* u = U + mit_segment_u(p, sl);        // inside U: mit_plan_check
    for (int j = tid; j < N; j += kMitThreads) {
        const double2 v = u[j];
        const double w = win[j];
        x[j] = make_double2(w * v.x, w * v.y);
    }
    __syncthreads();
    fft_lds_forward<kMitThreads>(x, N, tw, tid);
    const bool counted = s >= p.fin_lo && s < p.fin_hi;
    for (int i = tid; i < N; i += kMitThreads) {
        const int k = (int)(__brev((unsigned)i) >> (32 - log2n));
        const double2 a = x[i];
        if (__dadd_rn(__dmul_rn(a.x, a.x), __dmul_rn(a.y, a.y)) > limit[k]) {
            x[i] = make_double2(0.0, 0.0);
            if (counted) atomicAdd(&bins[k], 1ull);
        }
    }
    __syncthreads();
    fft_lds_inverse<kMitThreads>(x, N, tw, tid);
    const double scale = 1.0 / (double)N;               // (a power of two: exact)
    double2* out = B + sl * N;
    for (int j = tid; j < N; j += kMitThreads) {
        const double2 a = x[j];
        out[j] = make_double2(a.x * scale, a.y * scale);
    }
}

// src: B with the excisor, U without.
__global__ __launch_bounds__(kMitThreads) void mit_combine_kernel(const double2* __restrict__ src, void* __restrict__ ring, int out_fmt, MitPlan p,
                                                                  int64_t ring_offset, int64_t capacity) {
    const int64_t i = (int64_t)blockIdx.x * kMitThreads + threadIdx.x;
    if (i >= p.k) return;
    const int64_t m = mit_output_m(p, i);
    double yr = 0.0, yi = 0.0;
    if (m >= 0) {
        if (p.N) {
            int64_t a, b;
            mit_output_terms(p, m, &a, &b);
            const double2 va = src[a], vb = src[b];
            yr = va.x + vb.x, yi = va.y + vb.y;
        } else {
            const double2 v = src[mit_output_u(p, m)];
            yr = v.x, yi = v.y;
        }
    }
    const int64_t pos = ring_offset + i;
    ring_write(ring, out_fmt, pos >= capacity ? pos - capacity : pos, yr, yi);
}

// b grows to `bytes`, its first `keep` bytes kept (the state when a push is longer than any before it).
int grow_keeping(sdr_engine* e, DevBuf* b, size_t bytes, size_t keep) {
    if (bytes <= b->bytes && b->ptr) return SDR_OK;
    void* fresh = nullptr;
    hipError_t err = hipMalloc(&fresh, bytes);
    if (err != hipSuccess) return sdr_fail(SDR_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    if (b->ptr) {
        if (keep) err = hipMemcpyAsync(fresh, b->ptr, keep, hipMemcpyDeviceToDevice, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);   // (kernels queued earlier may still read the old block)
        if (err != hipSuccess) {
            (void)hipFree(fresh);
            return sdr_fail(SDR_ERR_HIP, "growing the mitigator's work buffer: %s", hipGetErrorString(err));
        }
        (void)hipFree(b->ptr);
    }
    b->ptr = fresh, b->bytes = bytes;
    return SDR_OK;
}

size_t counter_bytes(const Mitigator* m) { return (size_t)(kCounterHead + m->N) * sizeof(unsigned long long); }

}  // namespace

int mit_create(sdr_engine* e, const sdr_mit_cfg* cfg, Mitigator** out) {
    *out = nullptr;
    const int N = cfg->nfft;
    if (N != 0 && (N < kFftLdsMin || N > kFftLdsMax || (N & (N - 1))))
        return sdr_fail(SDR_ERR_INVALID, "nfft %d is neither 0 nor a power of two in %d..%d", N, kFftLdsMin, kFftLdsMax);
    if (cfg->blank_lead < 0 || cfg->blank_lead > kMitMaxReach || cfg->blank_hold < 0 || cfg->blank_hold > kMitMaxReach)
        return sdr_fail(SDR_ERR_INVALID, "blank_lead %d / blank_hold %d outside 0..%d", cfg->blank_lead, cfg->blank_hold, kMitMaxReach);
    if (cfg->flags) return sdr_fail(SDR_ERR_INVALID, "unknown flags 0x%x", cfg->flags);
    if (!(cfg->blank_level >= 0.0)) return sdr_fail(SDR_ERR_INVALID, "blank_level is negative or not a number");
    if (N && !cfg->limit) return sdr_fail(SDR_ERR_INVALID, "limit is NULL");
    for (int k = 0; k < N; ++k)
        if (!(cfg->limit[k] >= 0.0)) return sdr_fail(SDR_ERR_INVALID, "limit %d is negative or not a number", k);
    if (!N && cfg->blank_level == 0.0) return sdr_fail(SDR_ERR_INVALID, "neither a blanker nor an excisor");
    Mitigator* m = new (std::nothrow) Mitigator();
    if (!m) return sdr_fail(SDR_ERR_NOMEM, "host allocation failed");
    m->N = N, m->blank = cfg->blank_level > 0.0;
    m->lead = m->blank ? cfg->blank_lead : 0, m->hold = m->blank ? cfg->blank_hold : 0;   // (they are the blanker's)
    m->level2 = cfg->blank_level * cfg->blank_level;
    while ((1 << m->log2n) < N) ++m->log2n;
    m->K = mit_state_length(N, m->lead, m->hold);
    const size_t state_bytes = (size_t)(m->K > 0 ? m->K : 1) * sizeof(double2);
    hipError_t err = hipMalloc((void**)&m->counters, counter_bytes(m));
    if (err == hipSuccess) err = hipMemsetAsync(m->counters, 0, counter_bytes(m), e->stream);
    for (int b = 0; b < 2 && err == hipSuccess; ++b) {
        err = hipMalloc(&m->work[b].ptr, state_bytes);
        if (err == hipSuccess) m->work[b].bytes = state_bytes;
    }
    if (err == hipSuccess) err = hipMemsetAsync(m->work[0].ptr, 0, state_bytes, e->stream);
    std::vector<double> host;
    if (N && err == hipSuccess) {
        host.resize((size_t)3 * N);
        fft_lds_fill_tables(N, host.data());
        for (int k = 0; k < N; ++k) host[(size_t)2 * N + k] = cfg->limit[k];
        err = hipMalloc(&m->tab, host.size() * sizeof(double));
        if (err == hipSuccess) err = hipMemcpyAsync(m->tab, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, e->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);     // (`host` and cfg->limit are free again)
    if (err != hipSuccess) {
        mit_destroy(nullptr, m);
        return sdr_fail(SDR_ERR_HIP, "sdr_ddc_mitigate: %s", hipGetErrorString(err));
    }
    *out = m;
    return SDR_OK;
}

void mit_destroy(sdr_engine* e, Mitigator* m) {
    if (!m) return;
    if (e) (void)hipStreamSynchronize(e->stream);     // (a queued push may still use the buffers)
    void* blocks[] = {m->tab, m->counters, m->work[0].ptr, m->work[1].ptr, m->u.ptr, m->seg.ptr};
    for (void* b : blocks)
        if (b) (void)hipFree(b);
    delete m;
}

int mit_reset(sdr_engine* e, Mitigator* m) {
    if (m->K > 0) SDR_HIP(hipMemsetAsync(m->work[m->cur].ptr, 0, (size_t)m->K * sizeof(double2), e->stream));
    SDR_HIP(hipMemsetAsync(m->counters, 0, counter_bytes(m), e->stream));
    return SDR_OK;
}

int64_t mit_delay_of(const Mitigator* m) { return mit_delay(m->N, m->lead); }

int mit_push_begin(sdr_engine* e, Mitigator* m, int64_t n, int64_t k, void** dst, int64_t* offset, int64_t* capacity) {
    const MitPlan p = mit_plan(n, k, m->N, m->lead, m->hold);
    if (int rc = grow_keeping(e, &m->work[m->cur], (size_t)(p.K + k) * sizeof(double2), (size_t)p.K * sizeof(double2))) return rc;
    if (m->blank)
        if (int rc = sdr_devbuf_reserve(e, &m->u, (size_t)p.n_u * sizeof(double2))) return rc;
    if (m->N)
        if (int rc = sdr_devbuf_reserve(e, &m->seg, (size_t)p.n_seg * m->N * sizeof(double2))) return rc;
    *dst = m->work[m->cur].ptr;
    *offset = p.K;
    *capacity = p.K + k;
    return SDR_OK;
}

int mit_push_finish(sdr_engine* e, Mitigator* m, int64_t n, int64_t k, int64_t ring_offset) {
    const MitPlan p = mit_plan(n, k, m->N, m->lead, m->hold);
    const double2* W = (const double2*)m->work[m->cur].ptr;
    const double2* U = W;                               // (no blanker: hold = lead = 0, U[x] = W[x])
    if (m->blank) {
        ProfScope ps(e, "mit_blank_kernel");
        hipLaunchKernelGGL(mit_blank_kernel, dim3((unsigned)((p.n_u + kMitBlankTile - 1) / kMitBlankTile)), dim3(kMitThreads), 0, e->stream, W,
                           (double2*)m->u.ptr, p, m->level2, m->counters);
        U = (const double2*)m->u.ptr;
    }
    const double2* src = U;
    if (m->N) {
        ProfScope ps(e, "mit_excise_kernel");
        const double2* tw = (const double2*)m->tab;
        const double* win = (const double*)m->tab + m->N;
        hipLaunchKernelGGL(mit_excise_kernel, dim3((unsigned)p.n_seg), dim3(kMitThreads), (size_t)m->N * sizeof(double2), e->stream, U,
                           (double2*)m->seg.ptr, p, m->log2n, tw, win, win + m->N, m->counters + kCounterHead);
        src = (const double2*)m->seg.ptr;
    }
    {
        ProfScope ps(e, "mit_combine_kernel");
        hipLaunchKernelGGL(mit_combine_kernel, dim3((unsigned)((k + kMitThreads - 1) / kMitThreads)), dim3(kMitThreads), 0, e->stream, src, e->iq,
                           e->iq_fmt, p, ring_offset, e->iq_capacity);
    }
    SDR_HIP(hipGetLastError());
    if (p.K > 0) {
        // the state of the next push, into the other buffer (which that push then extends)
        SDR_HIP(hipMemcpyAsync(m->work[m->cur ^ 1].ptr, W + k, (size_t)p.K * sizeof(double2), hipMemcpyDeviceToDevice, e->stream));
        m->cur ^= 1;
    }
    return SDR_OK;
}

int mit_stats(sdr_engine* e, Mitigator* m, int64_t n, sdr_mit_stats* out, int64_t* bins) {
    std::vector<unsigned long long> host((size_t)kCounterHead + m->N);
    SDR_HIP(hipMemcpyAsync(host.data(), m->counters, counter_bytes(m), hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    out->n_outputs = n;
    out->n_triggers = (int64_t)host[0];
    out->n_blanked = (int64_t)host[1];
    out->n_segments = mit_segments_finished(n, m->N, m->lead);
    int64_t total = 0;
    for (int k = 0; k < m->N; ++k) {
        total += (int64_t)host[(size_t)kCounterHead + k];
        if (bins) bins[k] = (int64_t)host[(size_t)kCounterHead + k];
    }
    out->n_bins_excised = total;
    return SDR_OK;
}

}  // namespace sdr
