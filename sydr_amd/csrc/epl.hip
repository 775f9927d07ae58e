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
//
// Here: the kernels and their launches (sdr_epl_plan_run*).  How a plan is made, fetched and destroyed: epl_plan.hip.
#include "correlator.h"
#include "correlator_chip.h"
#include "correlator_chip2.h"
#include "epl_plan_state.h"

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

}  // namespace

int sdr_epl_ensure_doubled_luts(sdr_engine* e, hipStream_t stream) {
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

namespace {

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

// The launch of a several-chips-per-lane shape's kernel (SDR_EPL_CHIPN_SHAPES): three taps in one launch.  false: `shape` is none.
bool launch_shape(int shape, sdr_engine* e, hipStream_t stream, const sdr_epl_plan* p, const sdr_epl_item* d_items, int n_items, double* d_out,
                  const void* d_setups, int xcd_run) {
    const size_t shmem = 8 * sizeof(uint32_t) + (size_t)((p->lut_words + 3) & ~3) * sizeof(uint32_t);
    switch (shape) {
#define SDR_SHAPE(S, ...)                                                                                                                      \
    case S:                                                                                                                                    \
        hipLaunchKernelGGL((epl2_kernel<__VA_ARGS__>), dim3(n_items), dim3(kWaveThreads), shmem, stream, e->iq, e->iq, e->iq_capacity, d_items, \
                           n_items, e->luts, p->lut_words, e->lut_stride, p->d_spacing, p->fs, d_out,                                           \
                           static_cast<const ChipNSetup<__VA_ARGS__>*>(d_setups), xcd_run);                                                     \
        return true;
        SDR_EPL_CHIPN_SHAPES(SDR_SHAPE)
#undef SDR_SHAPE
        default: return false;
    }
}

}  // namespace

extern "C" {

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
        if (int rc = sdr_epl_ensure_doubled_luts(e, ctx->stream)) return rc;   // (a slot may have been re-staged since the plan was made)
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
        // (several chips per lane: a kernel of its own)
        if (!launch_shape(decode(p->wide, e->iq_fmt, 3, 1, setups != nullptr).shape, e, st, p, items, n, out, setups, xcd_run)) {
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

int sdr_epl_plan_run(sdr_engine* e, sdr_epl_plan* p) {
    if (!p) return sdr_fail(SDR_ERR_INVALID, "plan is NULL");
    return sdr_epl_plan_run_range(e, p, 0, p->n_items);
}

}  // extern "C"
