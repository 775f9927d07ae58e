// Making, fetching and destroying an E/P/L plan (running one: epl.hip).  What a plan is gets decided by epl_plan.h -- host
// arithmetic, tested without a GPU; this file does the device work those decisions ask for, as a sequence of stages
// (plan_create_impl) with one error exit.
//
// What a creation queues, and what the host waits for, by route (PlanRoute; E: the engine's stream, P: its plan_stream):
//   short list (host memory, fewer than kLongList items)
//       host: the walk of the list (a second one by the half-chip view's rules where that view is allowed), the allocations,
//             the setups where the word asks for any
//       E:    [the doubled replica tables, where the view is taken and they are stale] items; [view: double_items_kernel];
//             spacings (the view's doubled ones out of the creation's own array); [the copy of the setups]; WAIT
//   long list (kLongList items and more, or in device memory: copied device to device)
//       E:    items; statistics in; validate_items_kernel; statistics out; spacings (out of the scratch); WAIT -- the one wait
//             of such a creation: the caller has its array back, and everything the setups read is in device memory
//       then  a word without setups: a WAIT of E, with nothing on it
//             row setups, buffers of its own -- P: chip_setup_kernel; `ready`.  No wait: the creation returns ("epl_plan_wait":
//             waits for `ready`), and every launch, fetch and destroy waits for `ready` itself
//             row setups in sdr_epl_batch's workspaces -- E: chip_setup_kernel; WAIT
//   long list on the half-chip view: as above up to the first WAIT (the plain spacings travel with the check all the same), then
//       E:    [the doubled replica tables]; double_items_kernel; the doubled spacings (out of the scratch); chip_setup_kernel; WAIT
//   long list with a shape: as above up to the first WAIT, then
//       host: a list in device memory has its first item read back (a blocking copy)
//       E:    the counter of strays zeroed; chipn_setup_kernel; the counter out; WAIT (the count decides the word); WAIT
//   long replicas (lut_words >= kLongLutWords): a list in device memory is read back whole, behind its check, for group_stride
//   sdr_epl_batch: the short or the long route by the list's length, in the engine's workspaces -- never P, always the final
//       WAIT -- then run, fetch (which waits) and destroy
//
// The page-locked scratch (StreamCtx::pinned of the engine's stream; layout: epl_plan.h) is written by a long list's creation
// alone, and every copy that reads it is queued in front of a wait of the engine's stream inside that creation (the
// statistics'; for the half-chip view's doubled spacings the one that ends the creation): once a creation has returned nothing
// reads the scratch, so the next plan -- or any other call that stages through ctx0.pinned -- may write it, whether or not the
// plan's setups are still being made.  The same holds for the host copies a short list's creation queues from (Creation).
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>

#include "correlator_chip2.h"
#include "epl_plan.h"
#include "epl_plan_state.h"

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
                                    sdr::kWaveThreads, S);
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

// What plan creation needs of a form with per-item setups -- a row of SDR_EPL_ROWS_* (epl_variant.h) with KS or KI, or a
// several-chips-per-lane shape (SDR_EPL_CHIPN_SHAPES): the size of one setup, the setups of a short list on the host
// (sdr_epl_batch, one call per EPL(): the same function, ~2 us per item, instead of a launch and -- a shape -- a round trip for
// the count), those of a long one in one launch.  on_host returns, on_device leaves in *d_missed (a shape; a row has no
// counter: nullptr), the number of items the scheme does not cover: 0 for a row.
struct SetupOps {
    size_t bytes;
    int (*on_host)(const sdr_epl_item* items, int n_items, const double* spacing, double fs, int64_t capacity, void* out);
    void (*on_device)(hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs, int64_t capacity,
                      void* d_out, int* d_missed);
};
template <int NT, int KM, int KS, int KI>
struct RowSetupsOf {
    static int on_host(const sdr_epl_item* items, int n_items, const double* spacing, double fs, int64_t capacity, void* out) {
        sdr::ChipSetup<NT>* const S = static_cast<sdr::ChipSetup<NT>*>(out);
        for (int i = 0; i < n_items; ++i) {
            const sdr_epl_item& it = items[i];
            sdr::chip_setup<NT, KM, KS, KI>(it.n_samples, it.start_sample, capacity, it.carrier_hz, it.rem_code, it.code_step, spacing, fs,
                                            sdr::kWaveThreads, S[i]);
        }
        return 0;
    }
    static void on_device(hipStream_t stream, const sdr_epl_item* d_items, int n_items, const double* d_spacing, double fs, int64_t capacity,
                          void* d_out, int*) {
        hipLaunchKernelGGL((chip_setup_kernel<NT, KM, KS, KI>), dim3((unsigned)((n_items + 63) / 64)), dim3(64), 0, stream, d_items, n_items,
                           d_spacing, fs, capacity, static_cast<sdr::ChipSetup<NT>*>(d_out));      // (a wave per 64 items)
    }
    static const SetupOps* get() {
        if constexpr (KS != 0 || KI != 0) {
            static const SetupOps ops = {sizeof(sdr::ChipSetup<NT>), &on_host, &on_device};
            return &ops;
        } else {
            return nullptr;      // (the block length alone: tap positions at run time)
        }
    }
};
static const SetupOps* row_setups(const EplForm& f) {
#define SDR_ROW(NT, KM, KS, KI) \
    if (f.nt == NT && f.km == KM && f.ks == KS && f.ki == KI) return RowSetupsOf<NT, KM, KS, KI>::get();
    SDR_EPL_ROWS_HEADLINE(SDR_ROW)
    SDR_EPL_ROWS_STRAIGHT(SDR_ROW)
#undef SDR_ROW
    return nullptr;
}
template <int... P>
struct ShapeSetupsOf {
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
    static const SetupOps* get() {
        static const SetupOps ops = {sizeof(Setup), &on_host, &on_device};
        return &ops;
    }
};
static const SetupOps* shape_setups(int shape) {
    switch (shape) {
#define SDR_SHAPE(S, ...) \
    case S: return ShapeSetupsOf<__VA_ARGS__>::get();
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
// (The fold is epl_plan.h's item_stats_merge, spelled in registers: the shape below is what fits beside a running launch.)
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

// ---- creation.  What its stages share.  items: the list in host memory, or d_src: the list in device memory (copied: the plan
// owns its items either way).  use_workspaces: the one-shot sdr_epl_batch (the function-level drop-in calls it once per EPL())
// keeps its device buffers in the engine between calls instead of allocating and freeing them every time.
struct Creation {
    sdr_engine* e;
    const sdr_epl_item *items, *d_src;
    int n_items;
    const double* spacing;
    int n_taps;
    double fs;
    bool use_workspaces;
    PlanSwitches sw;
    sdr_epl_plan* p = nullptr;
    int lut_words = 0, wide = 0;      // the list's verdict (ListVerdict), on the half-chip view (`doubled`) that view's
    bool doubled = false;
    int shape = 0;                    // the several-chips-per-lane shape the list asks for,
    const SetupOps* ops = nullptr;    // ... its setups, or those of the word's row (nullptr: the list has none)
    PlanRoute route = {};
    // what queued copies of a short list read: alive until the wait that ends the creation
    std::vector<sdr_epl_item> items2;   // the half-chip view: the host's copy with 2 * rem_code, 2 * code_step (for its setups)
    std::vector<char> host_setups;
    double spacing2[SDR_MAX_TAPS];      // the half-chip view: 2 * spacing
    double t_begin, t_valid, t_alloc, t_checked;   // "SDR_PLAN_TIMING"
};

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// A stage's failed runtime call ends the creation with this.
static int plan_fail(hipError_t err) {
    return sdr_fail(err == hipErrorOutOfMemory ? SDR_ERR_NOMEM : SDR_ERR_HIP, "plan setup failed: %s", hipGetErrorString(err));
}
#define PLAN_HIP(call) do { if (const hipError_t err_ = (call)) return plan_fail(err_); } while (0)

static ItemRules rules_of(const Creation& c, double scale) {
    return item_rules(c.e->n_slots, c.e->lut_stride, c.e->iq_capacity, c.spacing, c.n_taps, scale);
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

// The failure of a list whose lowest bad item is `index`: the message comes from the host's own look at that item.
static int bad_item(const Creation& c, int index) {
    sdr_epl_item it;
    if (c.items) it = c.items[index];
    else SDR_HIP(hipMemcpy(&it, c.p->d_items + index, sizeof(it), hipMemcpyDeviceToHost));
    int maxlen = 0, m_chip = 0;
    double step = 0.0, lo = 0.0, hi = 0.0;
    bool split = true;
    if (const int bad = check_item(it, rules_of(c, 1.0), c.e->code_len_host.data(), maxlen, step, m_chip, split, lo, hi))
        return item_error(c.e, it, index, bad, lo, hi);
    return sdr_fail(SDR_ERR_INVALID, "item %d: rejected by the device check", index);
}

// The list's word becomes the half-chip view's, where that view is taken (epl_plan.h: half_chip_view).
static int take_half_chip_view(Creation& c, bool ok2, int wide2) {
    if (!half_chip_view(c.wide, ok2, wide2, c.sw, c.lut_words, 0).taken) return SDR_OK;
    if (int rc = sdr_epl_ensure_doubled_luts(c.e, c.e->stream)) return rc;
    const HalfChipView v = half_chip_view(c.wide, ok2, wide2, c.sw, c.lut_words, c.e->lut2_stride);   // (the stride of the tables just made)
    c.doubled = true, c.wide = v.word, c.lut_words = v.lut_words;
    return SDR_OK;
}

// A short list: the host's walk, before anything is allocated.
static ListVerdict walk_items(const Creation& c, double scale) {
    const ItemRules r = rules_of(c, scale);
    ItemStats s = item_stats_initial(r.want_s12);
    for (int i = 0; i < c.n_items && s.first_bad == kNoBadItem; ++i) {
        int maxlen = 0, m_chip = 0;
        double step = 0.0, lo = 0.0, hi = 0.0;
        bool split = true;
        const int bad = check_item(c.items[i], r, c.e->code_len_host.data(), maxlen, step, m_chip, split, lo, hi);
        item_stats_add(s, i, bad, maxlen, step, m_chip, split);
    }
    return list_verdict(s, r, c.spacing, c.sw);
}
static int check_on_host(Creation& c) {
    const ListVerdict v = walk_items(c, 1.0);
    if (v.first_bad != kNoBadItem) return bad_item(c, v.first_bad);
    c.lut_words = v.lut_words, c.wide = v.word;
    if (!half_chip_view_allowed(c.wide, c.sw)) return SDR_OK;
    const ListVerdict v2 = walk_items(c, 2.0);
    return take_half_chip_view(c, v2.first_bad == kNoBadItem, v2.word);
}

static int allocate(Creation& c) {
    sdr_engine* const e = c.e;
    sdr_epl_plan* const p = c.p = new (std::nothrow) sdr_epl_plan();
    if (!p) return sdr_fail(SDR_ERR_NOMEM, "host allocation failed");
    p->n_items = c.n_items, p->n_taps = c.n_taps, p->fs = c.fs;
    p->code_generation = e->code_generation, p->ring_capacity = e->iq_capacity;
    const size_t bytes_items = (size_t)c.n_items * sizeof(sdr_epl_item), bytes_out = (size_t)c.n_items * 2 * c.n_taps * sizeof(double);
    if (c.use_workspaces) {
        if (int rc = sdr_devbuf_reserve(e, &e->ws_items, bytes_items)) return rc;
        if (int rc = sdr_devbuf_reserve(e, &e->ws_out, bytes_out)) return rc;
        if (int rc = sdr_devbuf_reserve(e, &e->ws_spacing, SDR_MAX_TAPS * sizeof(double))) return rc;
        p->borrowed = true;
        p->d_items = (sdr_epl_item*)e->ws_items.ptr;
        p->d_out = (double*)e->ws_out.ptr;
        p->d_spacing = (double*)e->ws_spacing.ptr;
    } else {
        PLAN_HIP(plan_take(e, (void**)&p->d_items, bytes_items, &p->bytes_items));
        PLAN_HIP(plan_take(e, (void**)&p->d_out, bytes_out, &p->bytes_out));
        PLAN_HIP(plan_take(e, (void**)&p->d_spacing, SDR_MAX_TAPS * sizeof(double), &p->bytes_spacing));
    }
    c.t_alloc = now_ms();
    return SDR_OK;
}

// The list's copy; behind it the check of a long list, one thread per item.  The spacings go to d_spacing on the way: behind
// the statistics' copy, in front of the wait for it.
static int upload_and_check(Creation& c) {
    sdr_engine* const e = c.e;
    PLAN_HIP(hipMemcpyAsync(c.p->d_items, c.d_src ? c.d_src : c.items, (size_t)c.n_items * sizeof(sdr_epl_item),
                            c.d_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, e->stream));
    if (!list_is_long(c.n_items, c.d_src != nullptr)) return SDR_OK;
    const ItemRules r1 = rules_of(c, 1.0), r2 = rules_of(c, 2.0);
    if (int rc = sdr_devbuf_reserve(e, &e->ws_stats, 2 * sizeof(ItemStats))) return rc;
    if (int rc = sdr_pinned_reserve(e, &e->ctx0, kPlanPinnedBytes)) return rc;
    ItemStats* const host = plan_pinned_stats(e->ctx0.pinned);
    host[0] = item_stats_initial(r1.want_s12), host[1] = item_stats_initial(r2.want_s12);
    SDR_HIP(hipMemcpyAsync(e->ws_stats.ptr, host, 2 * sizeof(ItemStats), hipMemcpyHostToDevice, e->stream));
    const unsigned check_blocks = (unsigned)((c.n_items + 255) / 256) < 2048u ? (unsigned)((c.n_items + 255) / 256) : 2048u;      // (eight per CU)
    hipLaunchKernelGGL(validate_items_kernel, dim3(check_blocks, 2), dim3(256), 0, e->stream, c.p->d_items, c.n_items, r1, r2,
                       (const int32_t*)e->code_len, static_cast<ItemStats*>(e->ws_stats.ptr));
    SDR_HIP(hipGetLastError());
    SDR_HIP(hipMemcpyAsync(host, e->ws_stats.ptr, 2 * sizeof(ItemStats), hipMemcpyDeviceToHost, e->stream));
    double* const stage = plan_pinned_spacing(e->ctx0.pinned);
    std::memcpy(stage, c.spacing, c.n_taps * sizeof(double));
    SDR_HIP(hipMemcpyAsync(c.p->d_spacing, stage, c.n_taps * sizeof(double), hipMemcpyHostToDevice, e->stream));
    // The one wait of a long list's creation.  In front of it on this stream: the copy of the caller's items (truly
    // asynchronous out of page-locked memory: the caller has its array back when this returns), the check, the statistics
    // and the spacings -- everything the setups read is in device memory from here on.
    SDR_HIP(hipStreamSynchronize(e->stream));
    const ListVerdict v = list_verdict(host[0], r1, c.spacing, c.sw), v2 = list_verdict(host[1], r2, c.spacing, c.sw);
    if (v.first_bad != kNoBadItem) return bad_item(c, v.first_bad);
    c.lut_words = v.lut_words, c.wide = v.word;
    return take_half_chip_view(c, v2.first_bad == kNoBadItem, v2.word);
}

// The list's verdict is final: what follows from it -- the period of its slots, its setups, its route.
static int decide(Creation& c) {
    c.t_checked = now_ms();
    sdr_epl_plan* const p = c.p;
    p->lut_words = c.lut_words, p->wide = c.wide, p->doubled = c.doubled;
    std::vector<sdr_epl_item> fetched;         // (a device list: the blocking copies below read it back, behind the check's wait)
    if (c.lut_words >= kLongLutWords) {
        const sdr_epl_item* h = c.items;
        if (!h) {
            fetched.resize(c.n_items);
            PLAN_HIP(hipMemcpy(fetched.data(), p->d_items, (size_t)c.n_items * sizeof(sdr_epl_item), hipMemcpyDeviceToHost));
            h = fetched.data();
        }
        p->group_stride = group_stride(&h->code_slot, sizeof(sdr_epl_item), c.n_items);
    }
    // (setups exist for lists of three or five taps, served as one chunk; `true`: whether a plan of this word is to hold them)
    const EplForm form = decode(c.wide, c.e->iq_fmt, c.n_taps, 1, true);
    if (form.setups) {
        c.ops = row_setups(form);
        if (!c.ops) return plan_fail(hipErrorInvalidValue);     // (a word whose tuple is no row of the lists)
    } else if (shape_possible(form, c.n_taps, c.sw, c.doubled, c.lut_words)) {
        sdr_epl_item first;
        if (c.items) first = c.items[0];
        else PLAN_HIP(hipMemcpy(&first, p->d_items, sizeof(first), hipMemcpyDeviceToHost));
        c.shape = list_shape(form, first.code_step, c.spacing, c.n_taps, c.sw, c.doubled, c.lut_words);
        c.ops = shape_setups(c.shape);
    }
    c.route = plan_route(c.n_items, c.d_src != nullptr, c.use_workspaces, c.doubled, form.setups, c.shape);
    return SDR_OK;
}

// The half-chip view of the items, and the spacings a check did not bring along.
static int finish_uploads(Creation& c) {
    sdr_engine* const e = c.e;
    if (c.doubled) {
        if (!c.route.check_on_device) {
            c.items2.assign(c.items, c.items + c.n_items);
            for (sdr_epl_item& it : c.items2) it.rem_code *= 2.0, it.code_step *= 2.0;
        }
        for (int t = 0; t < c.n_taps; ++t) c.spacing2[t] = 2.0 * c.spacing[t];
        hipLaunchKernelGGL(double_items_kernel, dim3((unsigned)((c.n_items + 255) / 256)), dim3(256), 0, e->stream, c.p->d_items, c.n_items);
        PLAN_HIP(hipGetLastError());
    }
    if (c.route.spacings_with_check) return SDR_OK;
    // (the doubled spacings of a long list go through the page-locked scratch its statistics came back to -- upload_and_check
    // reserved it; the wait that ends the creation is what the copy's source waits for -- not out of pageable memory)
    const double* src = c.doubled ? c.spacing2 : c.spacing;
    if (c.route.spacings_via_scratch) {
        double* const stage = plan_pinned_spacing(e->ctx0.pinned);
        std::memcpy(stage, src, c.n_taps * sizeof(double));
        src = stage;
    }
    PLAN_HIP(hipMemcpyAsync(c.p->d_spacing, src, c.n_taps * sizeof(double), hipMemcpyHostToDevice, e->stream));
    return SDR_OK;
}

// The per-item setups: reserved, made by the host or in one launch (one thread per item: items and spacings are on the device),
// kept unless too many items stray from a shape.
static int make_setups(Creation& c) {
    if (!c.ops) return SDR_OK;
    sdr_engine* const e = c.e;
    sdr_epl_plan* const p = c.p;
    p->setup_bytes = c.ops->bytes;
    const size_t bytes = p->setup_bytes * (size_t)c.n_items;
    if (c.use_workspaces) {
        if (sdr_devbuf_reserve(e, &e->ws_setups, bytes + 64) != SDR_OK) return plan_fail(hipErrorOutOfMemory);
        p->d_setups = (char*)e->ws_setups.ptr;
    } else {
        PLAN_HIP(plan_take(e, (void**)&p->d_setups, bytes + 64, &p->bytes_setups));     // (+ the counter of items a shape does not cover)
    }
    int missed = 0;
    if (c.route.setups == kSetupsOnHost) {      // (host_setups lives until the wait that ends the creation)
        c.host_setups.resize(bytes);
        missed = c.ops->on_host(c.doubled ? c.items2.data() : c.items, c.n_items, c.doubled ? c.spacing2 : c.spacing, c.fs, e->iq_capacity,
                                c.host_setups.data());
        if (shape_kept(c.n_items, missed))
            PLAN_HIP(hipMemcpyAsync(p->d_setups, c.host_setups.data(), bytes, hipMemcpyHostToDevice, e->stream));
    } else {
        // A long list with buffers of its own, run as it is: its row setups are queued on the engine's plan_stream and the
        // creation returns without waiting for them.  Beside the launch of the segment before, chip_setup_kernel (196
        // registers) gets a SIMD only where that launch drains; a caller that waits for it can queue the next launch only
        // then, and on the engine's own stream the plan after this one would have its item copy and check stuck behind it.
        // What the kernel reads is complete: the items and the spacings were waited for with the statistics.  What it
        // writes is this plan's alone until `ready`, which every reader waits for (run, fetch, destroy).
        hipStream_t on = e->stream;
        if (c.route.setups == kSetupsOnPlanStream) {
            if (!e->plan_stream) PLAN_HIP(hipStreamCreateWithFlags(&e->plan_stream, hipStreamNonBlocking));
            PLAN_HIP(hipEventCreateWithFlags(&p->ready, hipEventDisableTiming));
            on = e->plan_stream;
        }
        int* const d_missed = c.shape ? reinterpret_cast<int*>(p->d_setups + bytes) : nullptr;
        if (d_missed) PLAN_HIP(hipMemsetAsync(d_missed, 0, sizeof(int), on));
        c.ops->on_device(on, p->d_items, c.n_items, p->d_spacing, c.fs, e->iq_capacity, p->d_setups, d_missed);
        PLAN_HIP(hipGetLastError());
        if (p->ready) PLAN_HIP(hipEventRecord(p->ready, on));
        if (d_missed) {      // (a shape's setups are on the engine's stream)
            PLAN_HIP(hipMemcpyAsync(&missed, d_missed, sizeof(int), hipMemcpyDeviceToHost, on));
            PLAN_HIP(hipStreamSynchronize(on));
        }
    }
    if (shape_kept(c.n_items, missed)) {
        p->wide = c.wide = variant_with_shape(c.wide, c.shape);
    } else {                 // too many strays: the boundary variant serves the list
        if (!c.use_workspaces) plan_give(e, p->d_setups, p->bytes_setups);
        p->d_setups = nullptr;
        p->setup_bytes = 0;
    }
    return SDR_OK;
}

// (ahead: nothing of this plan is left on the engine's stream -- its last wait there was the statistics' -- and `ready` has
// been recorded behind the setups)
static int finish(Creation& c) {
    sdr_engine* const e = c.e;
    const bool ahead = c.route.ahead;
    const double t_queued = now_ms();
    if (!ahead) PLAN_HIP(hipStreamSynchronize(e->stream));
    if (ahead && e->epl_plan_wait) PLAN_HIP(hipEventSynchronize(c.p->ready));       // "epl_plan_wait": as a creation was before
    if (ahead) c.p->engine_stream_work = false;
    if (getenv("SDR_PLAN_TIMING")) {    // (last field, ahead: from the call's begin until `ready` was recorded -- the call queues, it does not wait)
        const bool queued_only = ahead && !e->epl_plan_wait;
        fprintf(stderr, "plan_create %d items: validate %.3f ms, alloc %.3f, copy+check %.3f, queue setups %.3f, %s %.3f\n", c.n_items,
                c.t_valid - c.t_begin, c.t_alloc - c.t_valid, c.t_checked - c.t_alloc, t_queued - c.t_checked,
                queued_only ? "ready recorded at" : "sync", queued_only ? t_queued - c.t_begin : now_ms() - t_queued);
    }
    return SDR_OK;
}

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
    Creation c = {e, items, d_src, n_items, spacing, n_taps, fs, use_workspaces,
                  PlanSwitches{e->iq_fmt, e->epl_no_chip, e->epl_no_double, e->epl_no_chip2, e->epl_no_split}};
    c.t_begin = now_ms();
    if (!list_is_long(n_items, d_src != nullptr))
        if (int rc = check_on_host(c)) return rc;
    c.t_valid = now_ms();
    int rc = SDR_OK;
    for (int (*stage)(Creation&) : {allocate, upload_and_check, decide, finish_uploads, make_setups, finish})
        if ((rc = stage(c)) != SDR_OK) break;
    if (rc != SDR_OK) {      // the one error exit: the half-made plan goes (destroy waits for what it queued; the failure's text stands)
        if (c.p && c.p->ready) (void)sdr_sync_plans(e);      // (`ready` may not have been recorded behind setups that were queued)
        sdr_epl_plan_destroy(e, c.p);
        return rc;
    }
    *out = c.p;
    return SDR_OK;
}

extern "C" {

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

int sdr_epl_plan_variant(const sdr_epl_plan* p) { return p ? p->wide + (p->doubled ? 65536 : 0) : -1; }

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
