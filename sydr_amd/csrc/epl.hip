// K1: batched carrier wipe-off + multi-tap PRN correlate-accumulate.
//
// One 64-lane WAVE = one channel-epoch = one call of the reference's EPL (sydr/dsp/tracking.py:92-116); a workgroup
// is one wave (or four waves -- four epochs of one channel -- when the staged replica is 16 KB and more).  IQ is
// streamed from the HBM ring with 16-byte loads, the PRN replica sits in LDS as the high words of +-1.0, accumulators
// are fp64 and are reduced inside the wave with DPP moves + v_readlane in a fixed order (so results do not depend on
// how channels are sharded over GPUs).  Three correlator cores, chosen per launch from the items' code steps:
//   chip-aligned (correlator_chip.h) : ci8, 16-26 samples per chip -- a lane owns a whole chip of the prompt tap; with the
//                                      block length (24/25 samples) and the outer taps' switch position (12/13) compiled
//                                      in when every epoch of the launch has them; 32-52 samples per chip through the
//                                      half-chip view of the replicas (every chip twice, doubled NCO parameters)
//   boundary     (correlator.h)      : a lane owns 16 (8) consecutive samples, < 1 chip; running sums in an LDS strip
//   per-sample   (correlator.h)      : exact chip index per sample and tap; low rates, epochs that wrap the ring
//
// Arithmetic that selects a chip is the reference's, operation for operation (np.linspace + np.ceil),
// in IEEE fp64 with contraction off:
//     shift = rem_code + spacing            stop = code_step*n + shift
//     step  = (stop - shift) / n            idx_i = ceil(i*step + shift)
// The carrier replica exp(1j*(-(f*2.0*pi*(i/fs)) + rem)) is evaluated once per lane in fp64 (exact range reduction +
// minimax sincos) and advanced by precomputed fp64 rotations inside a block and from block to block, which agrees
// with the reference to ~1e-15 relative on the accumulators (the bar is 1e-6).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>

#include "correlator.h"
#include "correlator_chip.h"
#include "correlator_chip2.h"
#include "epl_items.h"

#ifdef SDR_TRACE_WG
// Debug build only (tools/wg_trace.py): per-workgroup start/end clock and hardware id.
__device__ unsigned long long g_wg_trace[3 * 65536];
extern "C" __attribute__((visibility("default"))) int sdr_debug_read_trace(unsigned long long* dst, int n) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wg_trace), (size_t)n * 3 * sizeof(unsigned long long));
}
#endif

#include "epl_kernel.h"

namespace {

using namespace sdr;

// Half-chip view of the staged replicas: every chip twice.  A code of 32-52 samples per chip (GPS L1 C/A at 50 MHz)
// presented as a code of twice the chips at twice the rate has 16-26 samples per (half-)chip and runs on the
// chip-aligned correlator.  Exact: the kernel is handed 2*rem_code, 2*code_step and 2*spacing -- scaling by two
// commutes with every fp64 rounding of the reference's index expression, so its half-chip index is ceil(2y) for the
// reference's own y, and ceil(ceil(2y) / 2) = ceil(y) is the chip:  lut2[h + PAD] = lut[((h + 1) >> 1) + PAD].
__global__ __launch_bounds__(256) void double_lut_kernel(const uint32_t* __restrict__ luts, int stride, uint32_t* __restrict__ luts2,
                                                         int stride2) {
    const int slot = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= stride2) return;
    int src = ((j - SDR_LUT_PAD + 1) >> 1) + SDR_LUT_PAD;
    src = src < stride - 1 ? src : stride - 1;
    luts2[(size_t)slot * stride2 + j] = luts[(size_t)slot * stride + src];
}

int ensure_doubled_luts(sdr_engine* e, hipStream_t stream) {
    if (e->luts2 && e->luts2_generation == e->code_generation && e->luts2_stamp == e->code_stamp_counter) return SDR_OK;
    if (!e->luts2 || e->luts2_generation != e->code_generation) {
        if (e->luts2) SDR_HIP(hipFree(e->luts2));
        e->luts2 = nullptr;
        e->lut2_stride = (2 * e->lut_stride + 3) & ~3;
        if (hipMalloc(&e->luts2, (size_t)e->n_slots * e->lut2_stride * sizeof(uint32_t)) != hipSuccess)
            return sdr_fail(SDR_ERR_NOMEM, "hipMalloc for the half-chip replica tables failed");
    }
    // (on the stream the staging kernels use -- they are ordered before this -- and complete before any batch stream reads it)
    hipLaunchKernelGGL(double_lut_kernel, dim3((e->lut2_stride + 255) / 256, e->n_slots), dim3(256), 0, e->stream, e->luts,
                       e->lut_stride, e->luts2, e->lut2_stride);
    SDR_HIP(hipGetLastError());
    if (stream != e->stream) SDR_HIP(hipStreamSynchronize(e->stream));
    e->luts2_generation = e->code_generation;
    e->luts2_stamp = e->code_stamp_counter;
    return SDR_OK;
}

#ifndef SDR_EPL2_WAVES
#define SDR_EPL2_WAVES 3   // (a cap of 128 registers for four waves per SIMD spills into scratch: 0.296 instead of 0.192 ms per 32 000 epochs)
#endif
// Several chips per lane (correlator_chip2.h): one wave per item, three taps, ci8 ring; the item's setup comes from the plan.
// Dynamic LDS: [8 zero words][lut: lut_words uint32].
template <int... P>
__global__ __launch_bounds__(kWaveThreads, (sizeof...(P) > 4 ? 2 : SDR_EPL2_WAVES)) void epl2_kernel(const void* __restrict__ ring, const void* __restrict__ ring_flipped,
                                                            int64_t capacity, const sdr_epl_item* __restrict__ items, int n_items,
                                                            const uint32_t* __restrict__ luts, int lut_words, int lut_stride,
                                                            const double* __restrict__ spacing, double fs, double* __restrict__ out,
                                                            const ChipNSetup<P...>* __restrict__ setups, int xcd_run) {
    extern __shared__ double smem[];
    uint32_t* zero_words = reinterpret_cast<uint32_t*>(smem);
    uint32_t* lut = zero_words + 8;
    const int lane = threadIdx.x;
    const int item = __builtin_amdgcn_readfirstlane((int)xcd_order(blockIdx.x, gridDim.x, (unsigned)xcd_run));   // (xcd_order.h: runs of consecutive items per XCD)
    const sdr_epl_item it = items[item];
    EpochParams ep;
    ep.start_sample = it.start_sample;
    ep.n = it.n_samples;
    ep.carrier_hz = it.carrier_hz;
    ep.rem_carrier = it.rem_carrier;
    ep.rem_code = it.rem_code;
    ep.code_step = it.code_step;
    const ChipNSetup<P...>& S = setups[item];
    stage_lut<kWaveThreads>(lut, luts + (size_t)it.code_slot * lut_stride, lut_words, lane);
    if (lane < 8) zero_words[lane] = 0u;
    __syncthreads();  // replica staged
    double accr[3], acci[3];
    const bool done = S.base >= 0 && correlate_epoch_chipn<P...>(ring, ring_flipped, ep, S, lut, zero_words, lane, accr, acci);
    if (!done) {     // an epoch the scheme does not cover: per sample
        const double dphi = carrier_step(it.carrier_hz, fs);
        EpochConsts<3> K2;
        compute_constants<3>(K2, ep, spacing, dphi, kWaveThreads);
        correlate_epoch<SDR_FMT_CI8, 3>(ring, capacity, ep, dphi, K2, lut, lane, kWaveThreads, lane, accr, acci);
    }
    int slot;
    const double total = reduce_taps_scatter<3>(accr, acci, lane, slot);
    if (lane < 8) out[(size_t)item * 6 + slot] = total;
}

// One chunk of NT taps of a list: the kernel its variant word decodes to (epl_variant.h), launched through its address --
// every epl_kernel has the same arguments.
template <int FMT, int NT>
int launch_one(sdr_engine* e, hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs,
               int tap0, int n_taps_total, int lut_words, int wide, int group_stride, bool doubled, double* d_out,
               const void* d_setups, int xcd_run) {
    // long replicas: four waves (four epochs of one channel) per workgroup around one staged table
    const int wpw = (lut_words >= kLongLutWords && group_stride > 0) ? 4 : 1;
    // (the straight-line kernels read the plan's per-item setups: without them the run-time-position kernel serves the list)
    const EplForm f = decode(wide, FMT, NT, wpw, d_setups != nullptr);
    // (the chip-aligned cores are compiled for a ci8 ring alone, and chosen for one alone: the other formats name the 16-sample
    // boundary kernel where ci8 names a chip-aligned one)
    constexpr int kW = FMT == SDR_FMT_CI8 ? kChipMax : 16;
    constexpr int kOdd = NT == 3 || NT == 5 ? 1 : 0;          // (the compile-time tap geometries exist for these)
    const void* kernel = nullptr;
    if (f.row) {
#define SDR_ROW(N, KM, KS, KI) \
    if (NT == N && f.km == KM && f.ks == KS && f.ki == KI) kernel = (const void*)epl_kernel<FMT, N, kW, KM, 1, KS, KI>;
        SDR_EPL_ROWS_HEADLINE(SDR_ROW)
#undef SDR_ROW
        if (!kernel) kernel = sdr_epl_straight_kernel(NT, f.km, f.ks, f.ki);
    } else if (f.km2) {                  // 15.x or 16.x samples per chip, epoch by epoch
        if constexpr (FMT == SDR_FMT_CI8 && NT == 3) kernel = (const void*)epl_kernel<FMT, NT, kChipMax, 15, 1, 0, 0, 16>;
    } else if (f.w == kChipMax) {        // chip-aligned, tap positions at run time; 24: every epoch with 24 or 25 samples per chip
        if (wpw == 4)                    // (... and its form with taps whole (half-)chips apart: configs 4-5)
            kernel = f.ki   ? (const void*)epl_kernel<FMT, NT, kW, 24, 4, 0, kOdd>
                     : f.km ? (const void*)epl_kernel<FMT, NT, kW, 24, 4>
                            : (const void*)epl_kernel<FMT, NT, kW, 0, 4>;
        else
            kernel = f.km ? (const void*)epl_kernel<FMT, NT, kW, 24> : (const void*)epl_kernel<FMT, NT, kW>;
    } else if (wpw == 4) {
        kernel = f.w == 16  ? (const void*)epl_kernel<FMT, NT, 16, 0, 4>
                 : f.w == 8 ? (const void*)epl_kernel<FMT, NT, 8, 0, 4>
                            : (const void*)epl_kernel<FMT, NT, 0, 0, 4>;
    } else {
        kernel = f.w == 16 ? (const void*)epl_kernel<FMT, NT, 16> : f.w == 8 ? (const void*)epl_kernel<FMT, NT, 8> : (const void*)epl_kernel<FMT, NT, 0>;
    }
    if (!kernel) return sdr_fail(SDR_ERR_STATE, "no E/P/L kernel is compiled for variant %d with %d taps", wide, NT);
    const int threads = kWaveThreads * wpw;
    const size_t scratch = f.w == kChipMax ? (size_t)threads * chip_strip_slots<NT>() + wpw * kChipRotSlots
                                           : (f.w ? (size_t)threads * kPrefixSlots : 0);
    size_t shmem = (size_t)(wpw * 2 * NT) * sizeof(double) + (size_t)((lut_words + 3) & ~3) * sizeof(uint32_t) +
                   scratch * sizeof(double2);
    int stride = wpw > 1 ? group_stride : 1;
    const int grid = wpw > 1 ? (int)(((int64_t)n_items + (int64_t)wpw * stride - 1) / ((int64_t)wpw * stride)) * stride : n_items;
    const void* ring = e->iq;
    const void* flipped = (const void*)e->iq;
    int64_t cap = e->iq_capacity;
    int lut_stride = doubled ? e->lut2_stride : e->lut_stride;
    const uint32_t* luts = doubled ? e->luts2 : e->luts;
    void* args[] = {&ring, &flipped, &cap, &d_items, &n_items, &stride, &luts, &lut_words, &lut_stride, &d_spacing, &fs, &tap0,
                    &n_taps_total, &d_out, &d_setups, &xcd_run};
    if (shmem > 64u * 1024u)  // beyond the default dynamic-LDS grant (long multi-period replicas)
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    (void)hipLaunchKernel(kernel, dim3(grid), dim3(threads), args, shmem, stream);
    return SDR_OK;
}

template <int FMT>
int launch_fmt(sdr_engine* e, hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs,
               int n_taps, int lut_words, int wide, int group_stride, bool doubled, double* d_out, const void* d_setups, int xcd_run) {
    // Taps are served in register-resident chunks of 5/3/2/1.
    for (int t0 = 0; t0 < n_taps;) {
        const int left = n_taps - t0, nt = left >= 5 ? 5 : (left >= 3 ? 3 : left);
        auto chunk = [&](auto launch) { return launch(e, stream, d_items, n_items, d_spacing, fs, t0, n_taps, lut_words, wide, group_stride, doubled, d_out, d_setups, xcd_run); };
        const int rc = nt == 5 ? chunk(launch_one<FMT, 5>) : nt == 3 ? chunk(launch_one<FMT, 3>) : nt == 2 ? chunk(launch_one<FMT, 2>) : chunk(launch_one<FMT, 1>);
        if (rc) return rc;
        t0 += nt;
    }
    return SDR_OK;
}

}  // namespace

struct sdr_epl_plan {
    sdr_epl_item* d_items = nullptr;
    double* d_out = nullptr;
    double* d_spacing = nullptr;
    char* d_setups = nullptr;   // straight-line kernels: one ChipSetup<n_taps> / ChipNSetup per item (correlator_chip.h, correlator_chip2.h)
    size_t setup_bytes = 0;     // sizeof(ChipSetup<n_taps>), 0: none
    size_t bytes_items = 0, bytes_out = 0, bytes_spacing = 0, bytes_setups = 0;   // what the four allocations hold (plan_give)
    int n_items = 0;
    int n_taps = 0;
    int lut_words = 0;
    int wide = 0;  // 16 / 8: every item has 16 (8) * code_step < 1, the boundary variant with that group width applies
    int group_stride = 0;  // C > 0: items[i] and items[i + C] use the same code slot for every i (epoch-major lists of C channels)
    bool borrowed = false;  // device buffers are the engine's workspaces (sdr_epl_batch): not freed with the plan
    bool doubled = false;  // the plan runs on the half-chip view: its device items / spacings carry 2*rem_code, 2*code_step, 2*spacing
    double fs = 0.0;
    int64_t code_generation = 0;  // of the engine's code tables the plan was validated against
    int64_t ring_capacity = 0;    // and of the ring
    // one event per stream a range of the plan was launched on, re-recorded behind every launch: fetch waits for
    // exactly these instead of the whole device
    std::vector<std::pair<hipStream_t, hipEvent_t>> ran_on;
    // a long list's setups are made on the engine's plan_stream after creation has returned: recorded behind them, waited
    // for on the device by every launch and fetch and by the host in destroy (nullptr: the setups were done when creation returned)
    hipEvent_t ready = nullptr;
    // work of the plan may be pending on the engine's own stream: a creation that ended on an error path or did all its work
    // there, a range run on stream id 0.  Destroy then waits for that stream as well.
    bool engine_stream_work = true;
};

// The per-epoch setups of the straight-line kernels (ChipSetup / ChipNSetup: tap constants, epoch geometry, ring position,
// carrier rotations), made when a plan is created: one THREAD per item -- what every wave of an epoch would otherwise
// repeat in all of its 64 lanes -- with the same functions the run-time-position kernels call per wave.  1.92 M items
// (60 s x 32 channels) take ~0.22 ms of one launch on an idle device (DESIGN.md's kernel table).
template <int NT, int KM, int KS, int KI>
__global__ __launch_bounds__(64) void chip_setup_kernel(const sdr_epl_item* __restrict__ items, int n_items,
                                                        const double* __restrict__ spacing, double fs, int64_t capacity,
                                                        sdr::ChipSetup<NT>* __restrict__ out) {
    // One wave per 64 items.  A thread's setup is 784 / 864 bytes (three / five taps): stored where it belongs by the thread
    // itself, a wave's store instruction touches 64 places that far apart (1.4 ms for a 60 s x 32 channel plan, when a setup
    // had 480 bytes); through LDS the wave writes its 64 setups -- contiguous in memory -- sixteen bytes per lane, a kilobyte
    // per instruction (round 6).
    constexpr int kWords = (int)(sizeof(sdr::ChipSetup<NT>) / 16);
    static_assert(sizeof(sdr::ChipSetup<NT>) % 16 == 0, "setups are copied out in 16-byte granules");
    __shared__ uint4 stage[64 * kWords];
    const int i0 = blockIdx.x * 64, i = i0 + threadIdx.x;
    if (i < n_items) {
        const sdr_epl_item it = items[i];
        double sp[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) sp[t] = spacing[t];
        sdr::ChipSetup<NT> S;
        sdr::chip_setup<NT, KM, KS, KI>(it.n_samples, it.start_sample, capacity, it.carrier_hz, it.rem_code, it.code_step, sp, fs,
                                    kWaveThreads, S);
        // (granule w of every lane side by side: lane-major slots would put 64 lanes 30 granules apart on the same banks)
        const uint4* const src = reinterpret_cast<const uint4*>(&S);
#pragma unroll
        for (int w = 0; w < kWords; ++w) stage[w * 64 + threadIdx.x] = src[w];
    }
    __syncthreads();
    const int n_here = n_items - i0 < 64 ? n_items - i0 : 64;
    uint4* const dst = reinterpret_cast<uint4*>(out + i0);
    for (int g = threadIdx.x; g < n_here * kWords; g += 64) {
        const int item = g / kWords, w = g - item * kWords;
        dst[g] = stage[w * 64 + item];
    }
}
// ... *missed counts the items the several-chips-per-lane scheme does not cover (their setups say so, and the kernel
// redoes them per sample).
template <int... P>
__global__ __launch_bounds__(256) void chipn_setup_kernel(const sdr_epl_item* __restrict__ items, int n_items,
                                                          const double* __restrict__ spacing, double fs, int64_t capacity,
                                                          sdr::ChipNSetup<P...>* __restrict__ out, int* __restrict__ missed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const sdr_epl_item it = items[i];
    const double sp[3] = {spacing[0], spacing[1], spacing[2]};
    sdr::ChipNSetup<P...> S;
    if (!sdr::chipn_setup<P...>(it.n_samples, it.start_sample, capacity, it.carrier_hz, it.rem_code, it.code_step, sp, fs, S))
        atomicAdd(missed, 1);
    out[i] = S;
}

// What plan creation needs of a straight-line form with per-item setups -- a row of SDR_EPL_ROWS_* (epl_variant.h) with KS or
// KI: the size of its ChipSetup<NT>, the setups of a short list on the host (sdr_epl_batch, one call per EPL(): the same
// function, ~2 us per item, instead of a launch), those of a long one in one launch.
struct RowSetups {
    size_t bytes;
    void (*on_host)(const sdr_epl_item* items, int n_items, const double* spacing, double fs, int64_t capacity, void* out);
    void (*on_device)(hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs, int64_t capacity,
                      void* d_out);
};
template <int NT, int KM, int KS, int KI>
struct RowSetupsOf {
    static void on_host(const sdr_epl_item* items, int n_items, const double* spacing, double fs, int64_t capacity, void* out) {
        sdr::ChipSetup<NT>* const S = static_cast<sdr::ChipSetup<NT>*>(out);
        for (int i = 0; i < n_items; ++i) {
            const sdr_epl_item& it = items[i];
            sdr::chip_setup<NT, KM, KS, KI>(it.n_samples, it.start_sample, capacity, it.carrier_hz, it.rem_code, it.code_step, spacing, fs,
                                            kWaveThreads, S[i]);
        }
    }
    static void on_device(hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs, int64_t capacity,
                          void* d_out) {
        hipLaunchKernelGGL((chip_setup_kernel<NT, KM, KS, KI>), dim3((unsigned)((n_items + 63) / 64)), dim3(64), 0, stream, d_items, n_items,
                           d_spacing, fs, capacity, static_cast<sdr::ChipSetup<NT>*>(d_out));      // (a wave per 64 items)
    }
    static const RowSetups* get() {
        if constexpr (KS != 0 || KI != 0) {
            static const RowSetups ops = {sizeof(sdr::ChipSetup<NT>), &on_host, &on_device};
            return &ops;
        } else {
            return nullptr;      // (the block length alone: tap positions at run time)
        }
    }
};
static const RowSetups* row_setups(const EplForm& f) {
#define SDR_ROW(NT, KM, KS, KI) \
    if (f.nt == NT && f.km == KM && f.ks == KS && f.ki == KI) return RowSetupsOf<NT, KM, KS, KI>::get();
    SDR_EPL_ROWS_HEADLINE(SDR_ROW)
    SDR_EPL_ROWS_STRAIGHT(SDR_ROW)
#undef SDR_ROW
    return nullptr;
}

// The same of a several-chips-per-lane shape (SDR_EPL_CHIPN_SHAPES), and the launch of its kernel.  on_host returns, on_device
// leaves in *d_missed, the number of items the scheme does not cover.
struct ShapeOps {
    size_t bytes;
    int (*on_host)(const sdr_epl_item* items, int n_items, const double* spacing, double fs, int64_t capacity, void* out);
    void (*on_device)(hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs, int64_t capacity,
                      void* d_out, int* d_missed);
    void (*launch)(hipStream_t stream, size_t shmem, const void* ring, int64_t capacity, const sdr_epl_item* d_items, int n_items,
                   const uint32_t* luts, int lut_words, int lut_stride, const double* d_spacing, double fs, double* d_out,
                   const void* d_setups, int xcd_run);
};
template <int... P>
struct ShapeOpsOf {
    using Setup = sdr::ChipNSetup<P...>;
    static int on_host(const sdr_epl_item* items, int n_items, const double* spacing, double fs, int64_t capacity, void* out) {
        int missed = 0;
        for (int i = 0; i < n_items; ++i) {
            const sdr_epl_item& it = items[i];
            missed += sdr::chipn_setup<P...>(it.n_samples, it.start_sample, capacity, it.carrier_hz, it.rem_code, it.code_step, spacing, fs,
                                             static_cast<Setup*>(out)[i]) ? 0 : 1;
        }
        return missed;
    }
    static void on_device(hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs, int64_t capacity,
                          void* d_out, int* d_missed) {
        hipLaunchKernelGGL((chipn_setup_kernel<P...>), dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, stream, d_items, n_items,
                           d_spacing, fs, capacity, static_cast<Setup*>(d_out), d_missed);
    }
    static void launch(hipStream_t stream, size_t shmem, const void* ring, int64_t capacity, const sdr_epl_item* d_items, int n_items,
                       const uint32_t* luts, int lut_words, int lut_stride, const double* d_spacing, double fs, double* d_out,
                       const void* d_setups, int xcd_run) {
        hipLaunchKernelGGL((epl2_kernel<P...>), dim3(n_items), dim3(kWaveThreads), shmem, stream, ring, ring, capacity, d_items, n_items, luts,
                           lut_words, lut_stride, d_spacing, fs, d_out, static_cast<const Setup*>(d_setups), xcd_run);
    }
    static const ShapeOps* get() {
        static const ShapeOps ops = {sizeof(Setup), &on_host, &on_device, &launch};
        return &ops;
    }
};
static const ShapeOps* chipn_shape(int shape) {
    switch (shape) {
#define SDR_SHAPE(S, ...) \
    case S: return ShapeOpsOf<__VA_ARGS__>::get();
        SDR_EPL_CHIPN_SHAPES(SDR_SHAPE)
#undef SDR_SHAPE
        default: return nullptr;
    }
}

// ---- validation of a list: no item may index outside the ring or the staged replica, and what the list as a whole
// allows (the kernel variant) follows from every item.  One function per item for both sides: the host walks short lists
// (one call per EPL(): latency), one THREAD per item checks long ones behind their upload (1.92 M items of a 60 s x 32
// channel plan took the host 20-30 ms of the 34 ms a plan cost; the launch takes ~0.1 ms).
__device__ __forceinline__ unsigned long long dbits(double x) { return (unsigned long long)__double_as_longlong(x); }

// Two rule sets at once (the list as it is and its half-chip view): one upload, one launch, one read-back.  A thread walks
// the list with the grid's stride and keeps its own statistics; a wave reduces them and adds them to the list's with ONE set
// of atomics -- at 1.92 M items a set per 64 items was 420 k atomics on seven addresses, 2.2 ms of a 4.5 ms plan (round 6).
//
// One rule set per workgroup (blockIdx.y), not both per thread: a plan is made while the segment before it is correlated, by a
// launch that keeps three waves of 152 registers on every SIMD.  56 registers are what those leave of a SIMD's 512; with the 80
// a thread took for both rule sets, no wave of this kernel could be placed before that launch had drained, and the check of a
// segment's 160 000 items ended with it, 0.92 ms after it began; with 54 (-Rpass-analysis=kernel-resource-usage) it takes
// 0.087 ms beside that launch (kernel traces: profiles/epl_plan_stream_ab_same_box.txt; docs/notes/K1.md, "A plan beside a
// running launch").  The items are read twice, out of the L2 the second time.
__global__ __launch_bounds__(256) void validate_items_kernel(const sdr_epl_item* __restrict__ items, int n_items, ItemRules r1,
                                                             ItemRules r2, const int32_t* __restrict__ code_len,
                                                             ItemStats* __restrict__ out) {
    const int stride = (int)(gridDim.x * 256);
    const int v = blockIdx.y;
    const ItemRules& r = v ? r2 : r1;
    // (a lane without an item, or with a bad one, carries the neutral element of every reduction: all 64 lanes take part)
    int ml = 0, mlo = 0x7fffffff, mhi = 0, a12 = 1, fb = 0x7fffffff;
    unsigned long long mx = 0ull, mn = ~0ull;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_items; i += stride) {
        const sdr_epl_item it = items[i];
        int maxlen = 0, m_chip = 0;
        double step = 0.0, lo, hi;
        bool split = true;
        const int bad = check_item(it, r, code_len, maxlen, step, m_chip, split, lo, hi);
        if (bad) {
            fb = min(fb, i);
        } else {
            ml = max(ml, maxlen);
            const unsigned long long sb = dbits(step);
            mx = sb > mx ? sb : mx;
            mn = sb < mn ? sb : mn;
            mlo = min(mlo, m_chip);
            mhi = max(mhi, m_chip);
            a12 &= split ? 1 : 0;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ml = max(ml, __shfl_xor(ml, off, 64));
        const unsigned long long ox = __shfl_xor(mx, off, 64), on = __shfl_xor(mn, off, 64);
        mx = ox > mx ? ox : mx;
        mn = on < mn ? on : mn;
        mlo = min(mlo, __shfl_xor(mlo, off, 64));
        mhi = max(mhi, __shfl_xor(mhi, off, 64));
        a12 &= __shfl_xor(a12, off, 64);
        fb = min(fb, __shfl_xor(fb, off, 64));
    }
    // the block's four waves through LDS, then one set of atomics per block
    __shared__ int sh_i[4][5];
    __shared__ unsigned long long sh_u[4][2];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh_i[wave][0] = ml, sh_i[wave][1] = mlo, sh_i[wave][2] = mhi, sh_i[wave][3] = a12, sh_i[wave][4] = fb;
        sh_u[wave][0] = mx, sh_u[wave][1] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int b_ml = 0, b_lo = 0x7fffffff, b_hi = 0, b_a12 = 1, b_fb = 0x7fffffff;
        unsigned long long b_mx = 0ull, b_mn = ~0ull;
        for (int w = 0; w < 4; ++w) {
            b_ml = max(b_ml, sh_i[w][0]);
            b_lo = min(b_lo, sh_i[w][1]);
            b_hi = max(b_hi, sh_i[w][2]);
            b_a12 &= sh_i[w][3];
            b_fb = min(b_fb, sh_i[w][4]);
            b_mx = sh_u[w][0] > b_mx ? sh_u[w][0] : b_mx;
            b_mn = sh_u[w][1] < b_mn ? sh_u[w][1] : b_mn;
        }
        ItemStats* o = out + v;
        atomicMax(&o->maxlen, b_ml);
        atomicMax(&o->max_step_bits, b_mx);
        atomicMin(&o->min_step_bits, b_mn);
        atomicMin(&o->m_lo, b_lo);
        atomicMax(&o->m_hi, b_hi);
        if (!b_a12) atomicAnd(&o->all_split, 0);
        if (b_fb != 0x7fffffff) atomicMin(&o->first_bad, b_fb);
    }
}

static ItemRules item_rules(const sdr_engine* e, const double* spacing, int n_taps, double scale) {
    ItemRules r = {};
    r.n_slots = e->n_slots;
    r.lut_stride = e->lut_stride;
    r.n_taps = n_taps;
    r.iq_capacity = e->iq_capacity;
    r.scale = scale;
    r.smin = r.smax = spacing[0];
    for (int t = 1; t < n_taps; ++t) {
        r.smin = spacing[t] < r.smin ? spacing[t] : r.smin;
        r.smax = spacing[t] > r.smax ? spacing[t] : r.smax;
    }
    r.s_anchor = scale * spacing[n_taps < 5 ? n_taps / 2 : 2];   // centre tap of the first chunk of taps the kernels serve together
    r.sp0 = spacing[0];
    r.sp2 = n_taps >= 3 ? spacing[2] : 0.0;
    r.want_s12 = n_taps == 3;   // both outer taps switch chips 12.x samples into the anchor's block (KS = 12 kernel)
    return r;
}

static int item_error(const sdr_engine* e, const sdr_epl_item& it, int index, int code, double lo, double hi) {
    switch (code) {
        case ITEM_SLOT: return sdr_fail(SDR_ERR_INVALID, "item %d: code slot %d is not staged", index, it.code_slot);
        case ITEM_SAMPLES: return sdr_fail(SDR_ERR_RANGE, "item %d: n_samples %d outside (0, ring capacity]", index, it.n_samples);
        case ITEM_START: return sdr_fail(SDR_ERR_RANGE, "item %d: negative start_sample", index);
        case ITEM_NCO: return sdr_fail(SDR_ERR_INVALID, "item %d: non-finite or non-positive NCO parameter", index);
        default:
            return sdr_fail(SDR_ERR_RANGE,
                            "item %d: code phase range [%g, %g] leaves the staged replica [-%d, %d] "
                            "(stage more code periods with sdr_code_slots_ex)", index, lo, hi, SDR_LUT_PAD,
                            e->lut_stride - SDR_LUT_PAD - 2);
    }
}

// The kernel variant a list of these statistics gets (epl_variant.h: choose_variant).
// m_lo / m_hi: the list's range of whole samples per chip; all_split: ItemStats::all_split.
static int variant_of(const sdr_engine* e, const ItemRules& r, const double* spacing, double max_step, double min_step, int m_lo, int m_hi,
                      bool all_split) {
    VariantInputs v = {};
    v.n_taps = r.n_taps, v.scale = r.scale, v.s_anchor = r.s_anchor, v.spacing = spacing;
    v.max_step = max_step, v.min_step = min_step, v.m_lo = m_lo, v.m_hi = m_hi, v.all_split = all_split;
    v.iq_fmt = e->iq_fmt, v.lut_stride = e->lut_stride, v.no_chip = e->epl_no_chip, v.no_split = e->epl_no_split;
    return choose_variant(v);
}

// Host walk (short lists; and the one bad item of a long list, for its message: index0 = its place in the list).
static int validate_items(sdr_engine* e, const sdr_epl_item* items, int n_items, const double* spacing,
                          int n_taps, double scale, int* lut_words, int* wide, int index0 = 0) {
    const ItemRules r = item_rules(e, spacing, n_taps, scale);
    int maxlen = 0;
    double max_step = 0.0, min_step = 1e300;
    int m_lo = 0x7fffffff, m_hi = 0;
    bool all_split = r.want_s12;
    for (int i = 0; i < n_items; ++i) {
        int ml = 0;
        double step = 0.0, lo = 0.0, hi = 0.0;
        int m_chip = 0;
        bool split = true;
        if (const int bad = check_item(items[i], r, e->code_len_host.data(), ml, step, m_chip, split, lo, hi))
            return item_error(e, items[i], index0 + i, bad, lo, hi);
        m_lo = m_chip < m_lo ? m_chip : m_lo;
        m_hi = m_chip > m_hi ? m_chip : m_hi;
        all_split = all_split && split;
        if (step > max_step) max_step = step;
        if (step < min_step) min_step = step;
        if (ml > maxlen) maxlen = ml;
    }
    if (lut_words) *lut_words = maxlen + SDR_LUT_PAD + 2;
    *wide = variant_of(e, r, spacing, max_step, min_step, m_lo, m_hi, all_split);
    return SDR_OK;
}

// Page-locked scratch of a long list's plan (StreamCtx::pinned of the engine's stream): the two ItemStats, then the tap
// spacings.  Every copy that reads it is queued in front of a synchronisation of the engine's stream inside the plan's
// creation (the statistics'; for the half-chip view's doubled spacings the one that ends the creation): once a creation has
// returned nothing reads the scratch, so the next plan -- or any other call that stages through ctx0.pinned -- may write it,
// whether or not the plan's setups are still being made.
constexpr size_t kPlanPinnedBytes = 2 * sizeof(ItemStats) + SDR_MAX_TAPS * sizeof(double);

// The same for a list that is already on the device (long lists: behind their upload).  ok2: the half-chip view's rules
// were met as well (wide2 then holds its answer).  The spacings go to d_spacing on the way: behind the statistics' copy, in
// front of the wait for it.
static int validate_items_dev(sdr_engine* e, const sdr_epl_item* d_items, const sdr_epl_item* h_items, int n_items,
                              const double* spacing, int n_taps, double* d_spacing, int* lut_words, int* wide, bool* ok2,
                              int* wide2) {
    const ItemRules r1 = item_rules(e, spacing, n_taps, 1.0), r2 = item_rules(e, spacing, n_taps, 2.0);
    if (int rc = sdr_devbuf_reserve(e, &e->ws_stats, 2 * sizeof(ItemStats))) return rc;
    if (int rc = sdr_pinned_reserve(e, &e->ctx0, kPlanPinnedBytes)) return rc;
    ItemStats* host = static_cast<ItemStats*>(e->ctx0.pinned);
    for (int v = 0; v < 2; ++v) {
        host[v] = ItemStats{0x7fffffff, 0, 0, 0ull, ~0ull, 0x7fffffff, 0, (v ? r2 : r1).want_s12 ? 1 : 0};
    }
    SDR_HIP(hipMemcpyAsync(e->ws_stats.ptr, host, 2 * sizeof(ItemStats), hipMemcpyHostToDevice, e->stream));
    const unsigned check_blocks = (unsigned)((n_items + 255) / 256) < 2048u ? (unsigned)((n_items + 255) / 256) : 2048u;      // (eight per CU)
    hipLaunchKernelGGL(validate_items_kernel, dim3(check_blocks, 2), dim3(256), 0, e->stream, d_items, n_items, r1, r2,
                       (const int32_t*)e->code_len, static_cast<ItemStats*>(e->ws_stats.ptr));
    SDR_HIP(hipGetLastError());
    SDR_HIP(hipMemcpyAsync(host, e->ws_stats.ptr, 2 * sizeof(ItemStats), hipMemcpyDeviceToHost, e->stream));
    double* const stage = reinterpret_cast<double*>(static_cast<char*>(e->ctx0.pinned) + 2 * sizeof(ItemStats));
    std::memcpy(stage, spacing, n_taps * sizeof(double));
    SDR_HIP(hipMemcpyAsync(d_spacing, stage, n_taps * sizeof(double), hipMemcpyHostToDevice, e->stream));
    // The one wait of a long list's creation.  In front of it on this stream: the copy of the caller's items (truly
    // asynchronous out of page-locked memory: the caller has its array back when this returns), the check, the statistics
    // and the spacings -- everything the setups read is in device memory from here on.
    SDR_HIP(hipStreamSynchronize(e->stream));
    auto as_double = [](unsigned long long b) { double d; std::memcpy(&d, &b, sizeof(d)); return d; };
    if (host[0].first_bad != 0x7fffffff) {
        const int i = host[0].first_bad;
        sdr_epl_item it;
        if (h_items) it = h_items[i];
        else SDR_HIP(hipMemcpy(&it, d_items + i, sizeof(it), hipMemcpyDeviceToHost));
        int wd;
        const int rc = validate_items(e, &it, 1, spacing, n_taps, 1.0, nullptr, &wd, i);   // (the message, from the host's own walk of that item)
        return rc ? rc : sdr_fail(SDR_ERR_INVALID, "item %d: rejected by the device check", i);
    }
    *lut_words = host[0].maxlen + SDR_LUT_PAD + 2;
    *wide = variant_of(e, r1, spacing, as_double(host[0].max_step_bits), as_double(host[0].min_step_bits), host[0].m_lo, host[0].m_hi,
                       host[0].all_split != 0);
    *ok2 = host[1].first_bad == 0x7fffffff;
    if (*ok2)
        *wide2 = variant_of(e, r2, spacing, as_double(host[1].max_step_bits), as_double(host[1].min_step_bits), host[1].m_lo, host[1].m_hi,
                            host[1].all_split != 0);
    return SDR_OK;
}

// (half-chip view of a list on the device: 2 * rem_code, 2 * code_step)
__global__ __launch_bounds__(256) void double_items_kernel(sdr_epl_item* __restrict__ items, int n_items) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    items[i].rem_code *= 2.0;
    items[i].code_step *= 2.0;
}

// Device memory for a plan: a buffer a destroyed plan left in the engine's pool if one fits (not more than twice the size:
// a 60 s plan's 0.9 GB of setups never serve a one-second plan), else a fresh allocation.  plan_give: back into the pool --
// eight buffers at most, the smallest makes room -- instead of hipFree, which waits for every stream of the device.
static hipError_t plan_take(sdr_engine* e, void** out, size_t bytes, size_t* got) {
    int best = -1;
    for (int i = 0; i < (int)e->plan_pool.size(); ++i) {
        const size_t b = e->plan_pool[(size_t)i].bytes;
        if (b >= bytes && b <= 2 * bytes + 4096 && (best < 0 || b < e->plan_pool[(size_t)best].bytes)) best = i;
    }
    if (best >= 0) {
        *out = e->plan_pool[(size_t)best].ptr;
        *got = e->plan_pool[(size_t)best].bytes;
        e->plan_pool.erase(e->plan_pool.begin() + best);
        return hipSuccess;
    }
    *got = bytes;
    return hipMalloc(out, bytes);
}

static void plan_give(sdr_engine* e, void* ptr, size_t bytes) {
    if (!ptr) return;
    if (!e || bytes == 0) {
        (void)hipFree(ptr);
        return;
    }
    e->plan_pool.push_back(DevBuf{ptr, bytes});
    if (e->plan_pool.size() > 8) {
        size_t small = 0;
        for (size_t i = 1; i < e->plan_pool.size(); ++i)
            if (e->plan_pool[i].bytes < e->plan_pool[small].bytes) small = i;
        (void)hipFree(e->plan_pool[small].ptr);
        e->plan_pool.erase(e->plan_pool.begin() + (long)small);
    }
}

extern "C" {

static int plan_create_impl(sdr_engine* e, const sdr_epl_item* items, const sdr_epl_item* d_src, int n_items, const double* spacing,
                            int n_taps, double fs, bool use_workspaces, sdr_epl_plan** out);

int sdr_epl_plan_create(sdr_engine* e, const sdr_epl_item* items, int n_items, const double* spacing,
                        int n_taps, double fs, sdr_epl_plan** out) {
    if (!items) return sdr_fail(SDR_ERR_INVALID, "no items");
    return plan_create_impl(e, items, nullptr, n_items, spacing, n_taps, fs, false, out);
}

int sdr_epl_plan_create_dev(sdr_engine* e, const sdr_epl_item* items_dev, int n_items, const double* spacing,
                            int n_taps, double fs, sdr_epl_plan** out) {
    if (!items_dev) return sdr_fail(SDR_ERR_INVALID, "no items");
    return plan_create_impl(e, nullptr, items_dev, n_items, spacing, n_taps, fs, false, out);
}

// items: the list in host memory, or d_src: the list in device memory (copied: the plan owns its items either way).
// use_workspaces: the one-shot sdr_epl_batch (the function-level drop-in calls it once per EPL()) keeps its three device
// buffers in the engine between calls instead of allocating and freeing them every time.
static int plan_create_impl(sdr_engine* e, const sdr_epl_item* items, const sdr_epl_item* d_src, int n_items, const double* spacing,
                            int n_taps, double fs, bool use_workspaces, sdr_epl_plan** out) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!out) return sdr_fail(SDR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if ((!items && !d_src) || n_items <= 0) return sdr_fail(SDR_ERR_INVALID, "no items");
    if (!spacing || n_taps < 1 || n_taps > SDR_MAX_TAPS)
        return sdr_fail(SDR_ERR_INVALID, "n_taps %d outside 1..%d", n_taps, SDR_MAX_TAPS);
    if (!(fs > 0.0)) return sdr_fail(SDR_ERR_INVALID, "fs must be positive");
    int lut_words = 0;
    int wide = 0;
    const bool timing = getenv("SDR_PLAN_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    // a short list is checked by the host before anything is allocated (one call per EPL(): latency); a long one by one
    // thread per item behind its upload
    const bool long_list = d_src != nullptr || n_items >= 4096;
    // a list that misses the chip-aligned correlator only because a chip holds too many samples (32-52: GPS L1 C/A at
    // 50 MHz) runs on the half-chip view of its replicas
    bool doubled = false;
    auto half_chip_view_allowed = [&] {
        return !variant_chip_aligned(wide) && e->iq_fmt == SDR_FMT_CI8 && !e->epl_no_chip && !e->epl_no_double;
    };
    auto consider_half_chip_view = [&](bool ok2, int wide2) -> int {
        if (half_chip_view_allowed() && ok2 && variant_chip_aligned(wide2)) {
            if (int rc = ensure_doubled_luts(e, e->stream)) return rc;
            doubled = true;
            wide = wide2;
            lut_words = 2 * lut_words < e->lut2_stride ? 2 * lut_words : e->lut2_stride;
        }
        return SDR_OK;
    };
    if (!long_list) {
        if (int rc = validate_items(e, items, n_items, spacing, n_taps, 1.0, &lut_words, &wide)) return rc;
        int wide2 = 0;
        bool ok2 = false;
        if (half_chip_view_allowed()) ok2 = validate_items(e, items, n_items, spacing, n_taps, 2.0, nullptr, &wide2) == SDR_OK;
        if (int rc = consider_half_chip_view(ok2, wide2)) return rc;
    }
    const double t_valid = now();

    sdr_epl_plan* p = new (std::nothrow) sdr_epl_plan();
    if (!p) return sdr_fail(SDR_ERR_NOMEM, "host allocation failed");
    p->n_items = n_items;
    p->n_taps = n_taps;
    p->fs = fs;
    p->code_generation = e->code_generation;
    p->ring_capacity = e->iq_capacity;
    hipError_t err = hipSuccess;
    if (use_workspaces) {
        int rc = sdr_devbuf_reserve(e, &e->ws_items, (size_t)n_items * sizeof(sdr_epl_item));
        if (!rc) rc = sdr_devbuf_reserve(e, &e->ws_out, (size_t)n_items * 2 * n_taps * sizeof(double));
        if (!rc) rc = sdr_devbuf_reserve(e, &e->ws_spacing, SDR_MAX_TAPS * sizeof(double));
        if (rc) {
            delete p;
            return rc;
        }
        p->borrowed = true;
        p->d_items = (sdr_epl_item*)e->ws_items.ptr;
        p->d_out = (double*)e->ws_out.ptr;
        p->d_spacing = (double*)e->ws_spacing.ptr;
    } else {
        err = plan_take(e, (void**)&p->d_items, (size_t)n_items * sizeof(sdr_epl_item), &p->bytes_items);
        if (err == hipSuccess) err = plan_take(e, (void**)&p->d_out, (size_t)n_items * 2 * n_taps * sizeof(double), &p->bytes_out);
        if (err == hipSuccess) err = plan_take(e, (void**)&p->d_spacing, SDR_MAX_TAPS * sizeof(double), &p->bytes_spacing);
    }
    const double t_alloc = now();
    if (err == hipSuccess)
        err = hipMemcpyAsync(p->d_items, d_src ? d_src : items, (size_t)n_items * sizeof(sdr_epl_item),
                             d_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess && long_list) {
        int wide2 = 0;
        bool ok2 = false;
        int rc = validate_items_dev(e, p->d_items, items, n_items, spacing, n_taps, p->d_spacing, &lut_words, &wide, &ok2, &wide2);
        if (!rc) rc = consider_half_chip_view(ok2, wide2);
        if (rc) {
            sdr_epl_plan_destroy(e, p);
            return rc;
        }
    }
    const double t_checked = now();
    p->lut_words = lut_words;
    p->wide = wide;
    p->doubled = doubled;
    // the period of the code-slot pattern, if the list has one (what lets four epochs of a channel share a staged table)
    std::vector<sdr_epl_item> fetched;          // (a device list of long replicas: its slots are read back for this)
    if (err == hipSuccess && lut_words >= kLongLutWords) {
        const sdr_epl_item* h = items;
        if (!h) {
            fetched.resize(n_items);
            err = hipMemcpy(fetched.data(), p->d_items, (size_t)n_items * sizeof(sdr_epl_item), hipMemcpyDeviceToHost);
            h = fetched.data();
        }
        if (err == hipSuccess) {
            int c = 1;
            while (c < n_items && h[c].code_slot != h[0].code_slot) ++c;
            bool periodic = c < n_items || n_items == 1;
            for (int i = 0; periodic && i + c < n_items; ++i) periodic = h[i].code_slot == h[i + c].code_slot;
            p->group_stride = periodic ? c : 0;
        }
    }
    std::vector<sdr_epl_item> items2;   // short lists on the half-chip view: the host's copy with 2 * rem_code, 2 * code_step (for its setups)
    std::vector<char> host_setups;      // short lists: the setups are made on the host (kept until the final synchronisation)
    double spacing2[SDR_MAX_TAPS];
    if (doubled) {
        if (items && !long_list) {
            items2.assign(items, items + n_items);
            for (sdr_epl_item& it : items2) it.rem_code *= 2.0, it.code_step *= 2.0;
        }
        for (int t = 0; t < n_taps; ++t) spacing2[t] = 2.0 * spacing[t];
        if (err == hipSuccess) {
            hipLaunchKernelGGL(double_items_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, e->stream, p->d_items, n_items);
            err = hipGetLastError();
        }
    }
    if (err == hipSuccess && !(long_list && !doubled)) {     // (a long list's own spacings went over with its check)
        // (the doubled spacings of a long list go through the page-locked scratch its statistics came back to -- validate_items_dev
        // reserved it; the final synchronisation below is what the copy's source waits for -- not out of pageable memory)
        const double* src = doubled ? spacing2 : spacing;
        if (long_list) {
            double* const stage = reinterpret_cast<double*>(static_cast<char*>(e->ctx0.pinned) + 2 * sizeof(ItemStats));
            std::memcpy(stage, src, n_taps * sizeof(double));
            src = stage;
        }
        err = hipMemcpyAsync(p->d_spacing, src, n_taps * sizeof(double), hipMemcpyHostToDevice, e->stream);
    }
    // ---- the per-item setups of the straight-line kernels: one launch, one thread per item (items and spacings are on the device)
    auto reserve_setups = [&](size_t bytes_per_item) {
        p->setup_bytes = bytes_per_item;
        const size_t bytes = bytes_per_item * (size_t)n_items;
        if (use_workspaces) {
            if (sdr_devbuf_reserve(e, &e->ws_setups, bytes + 64) != SDR_OK) err = hipErrorOutOfMemory;
            else p->d_setups = (char*)e->ws_setups.ptr;
        } else {
            err = plan_take(e, (void**)&p->d_setups, bytes + 64, &p->bytes_setups);     // (+ the counter of items a scheme does not cover)
        }
    };
    // (setups exist for lists of three or five taps, served as one chunk; `true`: whether a plan of this word is to hold them)
    const EplForm form = decode(wide, e->iq_fmt, n_taps, 1, true);
    if (err == hipSuccess && form.setups) {
        const RowSetups* const row = row_setups(form);
        if (!row) err = hipErrorInvalidValue;     // (a word whose tuple is no row of the lists)
        else reserve_setups(row->bytes);
        if (err == hipSuccess && !long_list) {
            host_setups.resize(p->setup_bytes * (size_t)n_items);
            row->on_host(doubled ? items2.data() : items, n_items, doubled ? spacing2 : spacing, fs, e->iq_capacity, host_setups.data());
            err = hipMemcpyAsync(p->d_setups, host_setups.data(), host_setups.size(), hipMemcpyHostToDevice, e->stream);
        } else if (err == hipSuccess) {
            // A long list with buffers of its own, run as it is: the setups are queued on the engine's plan_stream and the
            // creation returns without waiting for them.  Beside the launch of the segment before, chip_setup_kernel (196
            // registers) gets a SIMD only where that launch drains; a caller that waits for it can queue the next launch only
            // then, and on the engine's own stream the plan after this one would have its item copy and check stuck behind it.
            // What the kernel reads is complete: the items and the spacings were waited for with the statistics.  What it
            // writes is this plan's alone until `ready`, which every reader waits for (run, fetch, destroy).
            // (Not so: the half-chip view, whose double_items_kernel and doubled spacings are queued on the engine's stream;
            // sdr_epl_batch's shared workspaces.  Those keep the engine's stream and the wait that ends the creation.)
            hipStream_t on = e->stream;
            if (!doubled && !use_workspaces) {
                if (!e->plan_stream) err = hipStreamCreateWithFlags(&e->plan_stream, hipStreamNonBlocking);
                if (err == hipSuccess) err = hipEventCreateWithFlags(&p->ready, hipEventDisableTiming);
                if (err == hipSuccess) on = e->plan_stream;
            }
            if (err == hipSuccess) {
                row->on_device(on, p->d_items, n_items, p->d_spacing, fs, e->iq_capacity, p->d_setups);
                err = hipGetLastError();
            }
            if (err == hipSuccess && p->ready) err = hipEventRecord(p->ready, e->plan_stream);
        }
    }
    // three taps half a chip apart and chips of 9.5 .. 10 or 11.5 .. 12 samples (the reference's shipped 10 MHz; 12 MHz): two
    // chips per lane, if (nearly) every item fits the scheme.  (At 24 .. 24.5 samples per chip -- boundaries <12, 24, 36, 48> --
    // the same kernel was measured against the one-chip form: 5 % fewer instructions per sample, 60 % more per epoch, at the
    // register cap: 0.335 instead of 0.316 ms per 32 000 epochs; three chips per lane at 10 MHz -- <4, 9, 14, 19, 24, 29> --
    // spill 27 registers at three waves per SIMD: 0.44 instead of 0.57 of the roof.  Neither is instantiated.)
    // ... and chips of 3.75 .. 4 samples (the reference's 4 MHz, BASELINE configs[0]): FOUR chips per lane, where the list
    // would otherwise go per sample (round 6)
    if (err == hipSuccess && e->iq_fmt == SDR_FMT_CI8 && n_taps == 3 && !doubled && !e->epl_no_chip2 && (form.w == 8 || form.w == 0) &&
        lut_words < kLongLutWords) {          // (long multi-period replicas keep the four-epochs-per-workgroup kernels)
        sdr_epl_item first = {};
        if (items) first = items[0];
        else err = hipMemcpy(&first, p->d_items, sizeof(first), hipMemcpyDeviceToHost);
        const double two_chips = err == hipSuccess ? std::floor(2.0 / first.code_step) : 0.0;   // samples in two chips (any positive step got here)
        const double four_chips = err == hipSuccess ? std::floor(4.0 / first.code_step) : 0.0;
        const bool half_apart = spacing[0] == -0.5 && spacing[1] == 0.0 && spacing[2] == 0.5;
        const int shape = form.w == 8 ? (two_chips == 19.0 ? 1 : (two_chips == 23.0 ? 2 : 0)) : (four_chips == 15.0 && half_apart ? 3 : 0);
        if (const ShapeOps* const ops = chipn_shape(shape)) {
            reserve_setups(ops->bytes);
            int* d_missed = p->d_setups ? reinterpret_cast<int*>(p->d_setups + p->setup_bytes * (size_t)n_items) : nullptr;
            int missed = n_items;
            if (err == hipSuccess && !long_list) {
                // a short list (sdr_epl_batch: one call per EPL()): on the host, instead of a launch and a round trip for the
                // count -- the call is latency, not throughput
                host_setups.resize(p->setup_bytes * (size_t)n_items);
                missed = ops->on_host(items, n_items, spacing, fs, e->iq_capacity, host_setups.data());
                if (missed <= n_items / 64)      // (host_setups lives until the synchronisation that ends the plan's creation)
                    err = hipMemcpyAsync(p->d_setups, host_setups.data(), host_setups.size(), hipMemcpyHostToDevice, e->stream);
            } else if (err == hipSuccess) {
                err = hipMemsetAsync(d_missed, 0, sizeof(int), e->stream);
                if (err == hipSuccess) {
                    ops->on_device(e->stream, p->d_items, n_items, p->d_spacing, fs, e->iq_capacity, p->d_setups, d_missed);
                    err = hipGetLastError();
                }
                if (err == hipSuccess) err = hipMemcpyAsync(&missed, d_missed, sizeof(int), hipMemcpyDeviceToHost, e->stream);
                if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
            }
            if (err == hipSuccess && missed <= n_items / 64) {
                p->wide = wide = variant_with_shape(wide, shape);
            } else if (err == hipSuccess) {                 // too many strays: the boundary variant serves the list
                if (!use_workspaces && p->d_setups) plan_give(e, p->d_setups, p->bytes_setups);
                p->d_setups = nullptr;
                p->setup_bytes = 0;
            }
        }
    }
    // (ahead: nothing of this plan is left on the engine's stream -- its last wait there was the statistics' -- and `ready` has
    // been recorded behind the setups)
    const bool ahead = err == hipSuccess && p->ready != nullptr;
    const double t_queued = now();
    if (err == hipSuccess && !ahead) err = hipStreamSynchronize(e->stream);
    if (ahead && e->epl_plan_wait) err = hipEventSynchronize(p->ready);       // "epl_plan_wait": as a creation was before
    if (err == hipSuccess && ahead) p->engine_stream_work = false;
    if (timing) {    // (last field, ahead: from the call's begin until `ready` was recorded -- the call queues, it does not wait)
        const bool queued_only = ahead && !e->epl_plan_wait;
        fprintf(stderr, "plan_create %d items: validate %.3f ms, alloc %.3f, copy+check %.3f, queue setups %.3f, %s %.3f\n", n_items,
                t_valid - t_begin, t_alloc - t_valid, t_checked - t_alloc, t_queued - t_checked,
                queued_only ? "ready recorded at" : "sync", queued_only ? t_queued - t_begin : now() - t_queued);
    }
    if (err != hipSuccess) {
        if (p->ready) (void)sdr_sync_plans(e);      // (`ready` may not have been recorded behind setups that were queued)
        sdr_epl_plan_destroy(e, p);
        return sdr_fail(err == hipErrorOutOfMemory ? SDR_ERR_NOMEM : SDR_ERR_HIP, "plan setup failed: %s",
                        hipGetErrorString(err));
    }
    *out = p;
    return SDR_OK;
}

int sdr_epl_plan_run_range(sdr_engine* e, sdr_epl_plan* p, int64_t first, int64_t count) {
    return sdr_epl_plan_run_range_on(e, p, first, count, 0);
}

int sdr_epl_plan_run_range_on(sdr_engine* e, sdr_epl_plan* p, int64_t first, int64_t count, int stream_id) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!p) return sdr_fail(SDR_ERR_INVALID, "plan is NULL");
    StreamCtx* ctx = sdr_stream_ctx(e, stream_id);
    if (!ctx) return sdr_fail(SDR_ERR_INVALID, "stream id %d does not exist", stream_id);
    // A plan is validated against the code tables and the ring as they were at sdr_epl_plan_create; after
    // sdr_code_slots(_ex) / sdr_iq_alloc its slot indices, LUT length and ring bounds mean something else.
    if (p->code_generation != e->code_generation || p->ring_capacity != e->iq_capacity ||
        p->lut_words > (p->doubled ? 2 * e->lut_stride + 3 : e->lut_stride))
        return sdr_fail(SDR_ERR_STATE, "plan is stale: the code slots or the IQ ring were re-allocated after it was created");
    if (first < 0 || count <= 0 || first + count > p->n_items)
        return sdr_fail(SDR_ERR_RANGE, "item range [%lld, %lld) outside the plan's %d items", (long long)first,
                        (long long)(first + count), p->n_items);
    if (p->doubled)
        if (int rc = ensure_doubled_luts(e, ctx->stream)) return rc;   // (a slot may have been re-staged since the plan was made)
    // (the straight-line kernels build their doubles from sign-flipped bytes: a ci8 ring holds them that way -- ring_format.h kCi8Flip)
    if (int rc = sdr_iq_order_reader(e, ctx)) return rc;      // (behind the uploads queued on the engine's stream so far)
    const sdr_epl_item* items = p->d_items + first;
    double* out = p->d_out + (size_t)first * 2 * p->n_taps;
    const int n = (int)count;
    const void* setups = p->d_setups ? p->d_setups + (size_t)first * p->setup_bytes : nullptr;
    // (the order in which the range's own workgroups, 0 .. count - 1, take its items: xcd_order.h; read when the plan runs)
    const int xcd_run = e->epl_xcd_run;
    // behind the plan's setups, on the device: the host may be a whole launch ahead of them.  (On every stream, the engine's
    // own included -- the setups are on none of them; in front of the ProfScope: "epl_kernel" times the launch, not the wait.)
    if (p->ready) SDR_HIP(hipStreamWaitEvent(ctx->stream, p->ready, 0));
    if (ctx->stream == e->stream) p->engine_stream_work = true;      // (destroy has the engine's stream to wait for)
    {
        hipStream_t st = ctx->stream;
        ProfScope ps(e, "epl_kernel", st);
        // (several chips per lane: a kernel of its own, three taps in one launch)
        if (const ShapeOps* const ops = chipn_shape(decode(p->wide, e->iq_fmt, 3, 1, setups != nullptr).shape)) {
            const size_t shmem = 8 * sizeof(uint32_t) + (size_t)((p->lut_words + 3) & ~3) * sizeof(uint32_t);
            ops->launch(st, shmem, e->iq, e->iq_capacity, items, n, e->luts, p->lut_words, e->lut_stride, p->d_spacing, p->fs, out, setups, xcd_run);
        } else {
            const int rc = with_fmt(e->iq_fmt, [&](auto fmt) {
                return launch_fmt<decltype(fmt)::value>(e, st, items, n, p->d_spacing, p->fs, p->n_taps, p->lut_words, p->wide, p->group_stride,
                                                        p->doubled, out, setups, xcd_run);
            });
            if (rc) return rc;
        }
    }
    SDR_HIP(hipGetLastError());
    if (ctx->stream != e->stream) {   // (fetch copies on e->stream, which is ordered behind its own launches anyway)
        hipEvent_t ev = nullptr;
        for (auto& se : p->ran_on)
            if (se.first == ctx->stream) ev = se.second;
        if (!ev) {
            SDR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            p->ran_on.emplace_back(ctx->stream, ev);
        }
        SDR_HIP(hipEventRecord(ev, ctx->stream));
    }
    return SDR_OK;
}

int sdr_epl_plan_variant(const sdr_epl_plan* p) { return p ? p->wide + (p->doubled ? 65536 : 0) : -1; }

int sdr_epl_plan_run(sdr_engine* e, sdr_epl_plan* p) {
    if (!p) return sdr_fail(SDR_ERR_INVALID, "plan is NULL");
    return sdr_epl_plan_run_range(e, p, 0, p->n_items);
}

int sdr_epl_plan_fetch(sdr_engine* e, sdr_epl_plan* p, double* out) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!p || !out) return sdr_fail(SDR_ERR_INVALID, "NULL plan or output");
    for (auto& se : p->ran_on) SDR_HIP(hipStreamWaitEvent(e->stream, se.second, 0));   // the streams its ranges ran on, no others
    // (every launch waited for `ready` itself, so ran_on and the engine's own order cover the setups; a plan that never ran
    // has its copy behind them all the same)
    if (p->ready) SDR_HIP(hipStreamWaitEvent(e->stream, p->ready, 0));
    SDR_HIP(hipMemcpyAsync(out, p->d_out, (size_t)p->n_items * 2 * p->n_taps * sizeof(double),
                           hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

void sdr_epl_plan_destroy(sdr_engine* e, sdr_epl_plan* p) {
    if (!p) return;
    // Waits for THIS plan's work, not for the engine's stream as such: in a segmented pass the next plan's item copy and check
    // are queued there, and a destroy that waited for them would put the host back behind the running launch.
    if (e) (void)hipSetDevice(e->device);
    if (p->ready) {
        (void)hipEventSynchronize(p->ready);
        (void)hipEventDestroy(p->ready);
    }
    for (auto& se : p->ran_on) {
        (void)hipEventSynchronize(se.second);
        (void)hipEventDestroy(se.second);
    }
    if (e && p->engine_stream_work) (void)hipStreamSynchronize(e->stream);
    // The four buffers are free to serve the next plan.  d_items, d_spacing: written by copies that the creation waited for
    // with the statistics (or, a creation that kept to the engine's stream or failed half-way, by work on that stream: waited
    // for just above); read by the setups (`ready`) and the launches.  d_setups: written by the setups (`ready`, or the
    // engine's stream), read by the launches.  d_out: written by the launches -- on other streams `ran_on`, on stream id 0 the
    // engine's stream, waited for above -- and read by fetch, which waits for its own copy.
    if (!p->borrowed) {
        plan_give(e, p->d_items, p->bytes_items);
        plan_give(e, p->d_out, p->bytes_out);
        plan_give(e, p->d_spacing, p->bytes_spacing);
        plan_give(e, p->d_setups, p->bytes_setups);
    }
    delete p;
}

int sdr_epl_batch(sdr_engine* e, const sdr_epl_item* items, int n_items, const double* spacing, int n_taps,
                  double fs, double* out) {
    if (!out) return sdr_fail(SDR_ERR_INVALID, "out is NULL");
    sdr_epl_plan* p = nullptr;
    if (int rc = plan_create_impl(e, items, nullptr, n_items, spacing, n_taps, fs, true, &p)) return rc;
    int rc = sdr_epl_plan_run(e, p);
    if (!rc) rc = sdr_epl_plan_fetch(e, p, out);
    sdr_epl_plan_destroy(e, p);
    return rc;
}

}  // extern "C"
