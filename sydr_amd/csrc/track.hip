// Host side of the on-device loop closure (track_kernel.h holds the kernel): launch geometry, the sdr_track_closed_loop*
// entry points, the device-resident channel bank (sdr_bank_*), the tick server's host side with its doorman kernel, and
// sdr_iq_upload_begin.
#include "track_kernel.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

__global__ __launch_bounds__(kDoorThreads) void tick_doorman_kernel(const TickServer srv, int n_ch) {
    __shared__ unsigned words[8];
    __shared__ unsigned long long q[4];
    if (threadIdx.x < 8) words[threadIdx.x] = 0;
    if (threadIdx.x < 4) q[threadIdx.x] = 0;
    __syncthreads();
    tick_server_doorman(srv, n_ch, (int)threadIdx.x, words, q, (int)blockIdx.x);
}

// Device-side operands of one closed-loop launch.
struct TrackRun {
    sdr_track_state* d_states = nullptr;  // indexed through d_map when given
    const int32_t* d_map = nullptr;
    const sdr_loop_cfg* d_cfgs = nullptr;
    int cfg_stride = 0;                   // 0: d_cfgs[0] serves every channel; 1: one per state index
    int n_ch = 0, n_epochs = 0, n_taps = 3;
    sdr_track_epoch* d_traj = nullptr;    // [n_ch][n_epochs] or one scratch record when keep == 0
    int keep = 0;
    int8_t* d_bits = nullptr;
    int max_bits = 0;
    int32_t* d_nbits = nullptr;
    int32_t* d_done = nullptr;            // [n_ch] epochs completed
    sdr_track_state* d_states_copy = nullptr;  // [n_ch] end states by position in the list (nullable)
    int* fault_word = nullptr;            // where the launch's fault flag lives (already zero); nullptr: behind the exchange lines
    int force_parts = 0;                  // 0: choose
    const TickServer* server = nullptr;   // a tick-server launch: cluster form + the doorman, resident until told to leave
    unsigned* done_words = nullptr;       // page-locked [n_ch] (zero): every channel raises its word to done_seq behind its results
    unsigned done_seq = 0;
};

// Enqueue one closed-loop launch on ctx's stream.  *d_fault_out points at the launch's fault word.
int launch_track(sdr_engine* e, StreamCtx* ctx, const TrackRun& r, int* parts_used, int** d_fault_out) {
    const int lut_words = e->lut_stride;  // the whole staged row (every code period the slots were sized for)
    // exchange lines [n_ch][2 parities][8 parts][32 words] (tags zeroed: epoch tags start at 1), then the fault word
    // [head: ticket counters, ingest counter (one-launch ticks)][lines][fault word]
    const size_t xchg_bytes = (size_t)r.n_ch * 2 * kMaxParts * kXchgWordsMax * sizeof(unsigned long long);
    if (int rc = sdr_devbuf_reserve_on(e, ctx->stream, &ctx->xchg, kXchgHeadBytes + xchg_bytes + 16)) return rc;
    unsigned long long* d_xchg = (unsigned long long*)((char*)ctx->xchg.ptr + kXchgHeadBytes);
    int* d_fault = r.fault_word ? r.fault_word : (int*)((char*)d_xchg + xchg_bytes);
    *d_fault_out = d_fault;
    const void* d_iq = e->iq;
    int64_t cap = e->iq_capacity;
    const uint32_t* d_luts = e->luts;
    int lw = lut_words, ls = e->lut_stride, nch = r.n_ch, n_ep = r.n_epochs, mb = r.max_bits, keep = r.keep;
    sdr_track_state* d_st = r.d_states;
    sdr_track_state* d_st_copy = r.d_states_copy;
    const int32_t* d_map = r.d_map;
    const sdr_loop_cfg* d_cfgs = r.d_cfgs;
    int cfg_stride = r.cfg_stride;
    sdr_track_epoch* d_traj = r.d_traj;
    int8_t* d_bits = r.d_bits;
    int32_t* d_nbits = r.d_nbits;
    int32_t* d_done = r.d_done;
    const int nt = r.n_taps;

    int phase = 0;
    unsigned tag_base = 0;
    bool take_slab = false;          // the one-launch tick below pulls the staged slab in itself
    unsigned ingest_target = 0;
    // One attempt with `parts` workgroups per channel.
    auto attempt = [&](int parts, bool* too_big) -> hipError_t {
        // more channels than CUs: smaller workgroups, two or three of which share a CU, so that one channel's
        // loop update overlaps another's correlation (measured: 512 channels 20.2 -> 14.6 us per epoch,
        // 768 channels 22.3 -> 18.6)
        const bool dense = parts == 1 && r.n_ch > e->n_cus;
        const int threads = (parts >= 2 || dense) ? 256 : 512;
        const size_t shmem_base = (size_t)kRedDoubles * sizeof(double) + sizeof(EpochShared) +
                                  (size_t)((lut_words + 3) & ~3) * sizeof(uint32_t);
        const size_t prefix_bytes = (size_t)threads * kPrefixSlots * sizeof(double2);
        // The boundary variant of the correlator needs a 144-byte LDS strip per lane; long multi-period
        // replicas that leave no room for it are tracked with the per-sample variant.
        int up = shmem_base + prefix_bytes <= 160u * 1024u && e->lut_stride < kFastMaxLutWords ? 1 : 0;
        const size_t shmem = shmem_base + (up ? prefix_bytes : 0);
        *too_big = shmem > 160u * 1024u;
        if (*too_big) return hipSuccess;
        if (parts > 1 && !phase)  // tags of a previous launch must not validate this one's polls
            if (hipError_t me = hipMemsetAsync(d_xchg, 0, xchg_bytes + 16, ctx->stream)) return me;
        TickServer srv_arg = {};
        if (r.server) srv_arg = *r.server;
        else srv_arg.done_words = r.done_words, srv_arg.done_seq = r.done_seq;
        if (take_slab && phase == 3) {
            const size_t sb = sdr_fmt_bytes(e->iq_fmt);
            srv_arg.ring16 = (uint4*)e->iq;
            srv_arg.ring_flip = sdr::ring_flip_mask(e->iq_fmt);
            srv_arg.ring_n16 = (unsigned long long)((size_t)e->iq_capacity * sb / 16);
            srv_arg.ingest_src16 = (unsigned long long)((uintptr_t)e->srv_slab_src / 16);
            srv_arg.ingest_n16 = (unsigned long long)((size_t)e->srv_slab_n * sb / 16);
            srv_arg.ingest_first16 = (unsigned long long)((size_t)e->srv_slab_off * sb / 16);
            srv_arg.ingest_count = reinterpret_cast<unsigned*>(ctx->xchg.ptr) + 64;
            srv_arg.ingest_target = ingest_target;
        }
        const int extra_groups = srv_arg.ingest_n16 ? kTickIngestGroups : 0;
        void* args[] = {&d_iq, &cap, &d_st, &d_st_copy, &d_map, &d_cfgs, &cfg_stride, &n_ep, &d_traj, &keep, &d_bits, &mb,
                        &d_nbits, &d_done, &d_luts, &lw, &ls, &up, &nch, &parts, &d_xchg, &d_fault, &phase, &tag_base, &srv_arg};
        if (dense) return sdr_track_dense_launch(e->iq_fmt, nt, r.n_ch, shmem, ctx->stream, args);
        hipError_t err = hipSuccess;
        auto launch = [&](auto kernel) {
            // more than 64 KB of dynamic LDS has to be granted per kernel
            (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            if (phase)      // a two-launch tick: nobody waits for a peer inside either kernel
                err = hipLaunchKernel((const void*)kernel, dim3(phase == 2 ? r.n_ch : r.n_ch * parts + extra_groups), dim3(threads), args, shmem, ctx->stream);
            else if (parts > 1)  // the parts of a cluster wait for each other: all workgroups must be resident
                err = hipLaunchCooperativeKernel((const void*)kernel, dim3(r.n_ch * parts), dim3(threads), args,
                                                 (unsigned)shmem, ctx->stream);
            else
                err = hipLaunchKernel((const void*)kernel, dim3(r.n_ch), dim3(threads), args, shmem, ctx->stream);
        };
        auto by_shape = [&](auto fmt) {
            constexpr int F = decltype(fmt)::value;
            if (threads == 256) {
                if (nt == 5) launch(track_kernel<F, 256, 1, 5>);
                else launch(track_kernel<F, 256, 1, 3>);
            } else {
                if (nt == 5) launch(track_kernel<F, 512, 2, 5>);
                else launch(track_kernel<F, 512, 2, 3>);
            }
        };
        sdr::with_fmt(e->iq_fmt, by_shape);
        return err;
    };

    // Cluster size: as many workgroups per channel as the GPU has room for (1 per CU), up to 8.  When the
    // cooperative launch is refused (GPU shared or partitioned: not every workgroup could be resident) the
    // automatic choice halves the cluster until the launch goes through; a forced size fails instead.
    // One epoch (a receiver tick) takes the same cluster as two plain launches (below: a cooperative launch costs the host
    // +15-19 us); two epochs or more take the cooperative launch -- so that what a channel's epochs add up to does not
    // depend on how they are batched into steps (a block of 49 + a step of 2 == a block of 51, bit for bit).
    const int forced = r.force_parts ? r.force_parts : e->track_force_parts;
    int parts = 1;
    if (r.server && (forced < 2 || r.n_epochs < 2)) return sdr_fail(SDR_ERR_INVALID, "tick server: cluster size not given");
    if (forced) {
        parts = forced;
    } else if (r.n_epochs > 1) {
        while (parts < kMaxParts && (long)r.n_ch * parts * 2 <= (long)e->n_cus) parts *= 2;
    }
    if (!r.fault_word) SDR_HIP(hipMemsetAsync(d_fault, 0, 16, ctx->stream));
    // A one-epoch step (a receiver tick) on the cluster a block of epochs would get -- the same partition, the same order of
    // additions, the same bits -- as TWO plain launches cut at the exchange (see track_kernel): 17.4 us of one workgroup
    // per channel became ~11 on eight, without the +15-19 us a cooperative launch costs the host.
    int p2 = 1;
    if (!forced && r.n_epochs == 1 && !e->track_one_launch_tick && !r.server)
        while (p2 < kMaxParts && (long)r.n_ch * p2 * 2 <= (long)e->n_cus) p2 *= 2;
    // A slab staged for "the next tick's launch" (sdr_iq_upload_async: ingest_with_tick): the one-launch tick below takes it
    // along; any other launch wants it in the ring first, the ordinary way.
    const bool tick_form = p2 > 1 && !e->track_two_launch_tick && e->ingest_with_tick && ctx->stream == e->stream;
    if (!r.server) {
        if (e->srv_slab_pending && !tick_form)
            if (int rc = sdr_iq_flush_server_slab(e)) return rc;
        e->last_tick_took_slab = tick_form;
    }
    if (!forced && r.n_epochs == 1 && !e->track_one_launch_tick && !r.server) {
        if (p2 > 1) {
            // the lines are not zeroed per tick: this launch's tag (bit 31 set: no epoch tag of a block launch has it) has
            // never been stored in them -- unless the buffer is new or the 31-bit sequence wrapped: zero it then
            if (ctx->xchg_tagged != ctx->xchg.ptr || ctx->tick_seq >= 0x7ffffff0u) {
                SDR_HIP(hipMemsetAsync(ctx->xchg.ptr, 0, kXchgHeadBytes + xchg_bytes + 16, ctx->stream));
                ctx->ingest_launches = 0;
                ctx->xchg_tagged = ctx->xchg.ptr;
                ctx->tick_seq = 0;
            }
            tag_base = 0x80000000u | ++ctx->tick_seq;
            hipError_t err = hipSuccess;
            bool too_big = false;
            {
                ProfScope ps(e, "track_kernel", ctx->stream);
                if (e->track_two_launch_tick) {
                    phase = 1;
                    err = attempt(p2, &too_big);
                    phase = 2;
                    if (err == hipSuccess && !too_big) err = attempt(p2, &too_big);
                } else {
                    phase = 3;      // (both halves in one plain launch: the part that draws a channel's last ticket collects)
                    take_slab = tick_form && e->srv_slab_pending;
                    if (take_slab) ingest_target = (unsigned)kTickIngestGroups * (ctx->ingest_launches + 1);
                    err = attempt(p2, &too_big);
                    if (take_slab && err == hipSuccess && !too_big) {
                        // (the launch reads the staging half: busy until it has run)
                        ctx->ingest_launches += 1;
                        e->srv_slab_pending = false;
                        const int half = e->srv_slab_half;
                        if (half >= 0) {      // (-1: the caller's own page-locked block, the caller's to keep until the tick returns)
                            if (!e->slab_done[half]) (void)hipEventCreateWithFlags(&e->slab_done[half], hipEventDisableTiming);
                            (void)hipEventRecord(e->slab_done[half], ctx->stream);
                            e->slab_busy[half] = true;
                        }
                    }
                    take_slab = false;
                }
                phase = 0;
            }
            if (too_big) return sdr_fail(SDR_ERR_RANGE, "closed-loop tracking: code table does not fit the LDS");
            if (err != hipSuccess)
                return sdr_fail(SDR_ERR_HIP, "closed-loop tick launch (%d channels x %d parts) failed: %s", r.n_ch, p2, hipGetErrorString(err));
            SDR_HIP(hipGetLastError());
            if (parts_used) *parts_used = p2;
            return SDR_OK;
        }
    }
    hipError_t launch_err = hipSuccess;
    {
        ProfScope ps(e, "track_kernel", ctx->stream);
        for (;;) {
            bool too_big = false;
            launch_err = attempt(parts, &too_big);
            if (too_big) return sdr_fail(SDR_ERR_RANGE, "closed-loop tracking: code table does not fit the LDS");
            if (launch_err == hipSuccess || forced || parts == 1) break;
            (void)hipGetLastError();
            parts /= 2;
        }
    }
    if (launch_err != hipSuccess)
        return sdr_fail(SDR_ERR_HIP, "closed-loop tracking launch (%d channels x %d parts) failed: %s", r.n_ch, parts,
                        hipGetErrorString(launch_err));
    SDR_HIP(hipGetLastError());
    if (parts_used) *parts_used = parts;
    return SDR_OK;
}

int check_cfg(const sdr_loop_cfg* cfg, int index) {
    if (cfg->n_taps != 3 && cfg->n_taps != 5)
        return sdr_fail(SDR_ERR_UNSUPPORTED, "channel %d: closed-loop tracking runs 3 (E/P/L) or 5 (VE/E/P/L/VL) taps, got %d",
                        index, cfg->n_taps);
    if (cfg->loop_kind != 0 && cfg->loop_kind != 1)
        return sdr_fail(SDR_ERR_INVALID, "channel %d: loop_kind %d is neither 0 (Borre) nor 1 (Kaplan)", index, cfg->loop_kind);
    if (!(cfg->fs > 0.0)) return sdr_fail(SDR_ERR_INVALID, "channel %d: fs must be positive", index);
    if (cfg->epoch_chips < 0.0 || cfg->epochs_per_bit < 0 || !(cfg->epoch_seconds >= 0.0))
        return sdr_fail(SDR_ERR_INVALID, "channel %d: negative epoch_chips / epochs_per_bit / epoch_seconds", index);
    return SDR_OK;
}

int check_state(sdr_engine* e, const sdr_track_state* st, int index) {
    const int slot = st->code_slot;
    if (slot < 0 || slot >= e->n_slots || e->code_len_host[slot] <= 0)
        return sdr_fail(SDR_ERR_INVALID, "channel %d: code slot %d is not staged", index, slot);
    if (st->n_samples <= 0) return sdr_fail(SDR_ERR_INVALID, "channel %d: n_samples must be positive", index);
    return SDR_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------- channel bank
struct BankPending;
struct sdr_bank;
static void sdr_bank_free_pending(sdr_bank* b);
struct sdr_bank {
    int max_channels = 0;
    sdr_track_state* d_states = nullptr;  // [max_channels] -- the tracking state of this GPU's channels lives here
    sdr_loop_cfg* d_cfgs = nullptr;       // [max_channels]
    std::vector<int32_t> n_taps;          // host mirror of what was put: taps per channel, 0 = channel never put
    std::vector<int32_t> slot;
    int64_t code_generation = 0;
    // sdr_bank_step_begin / _end: scratch of their own (a tick between the two halves must not touch the results), on the engine's stream
    StreamCtx async_ctx;
    BankPending* pending = nullptr;
    // scratch of sdr_bank_tick_mirrored (kept between ticks: no allocation in the steady state)
    std::vector<int32_t> tick_list, tick_done;
    std::vector<sdr_track_state> tick_states;
    // a tick between its two halves (sdr_bank_tick_mirrored_begin / _end): one queued launch per tap group
    BankPending* tick_pending[2] = {nullptr, nullptr};
    StreamCtx tick_ctx[2];                // their scratch and page-locked blocks, the bank's own: other calls on the engine
                                          // between the two halves (an upload, a search) cannot move them
    bool tick_open = false, tick_two = false, tick_slab_queued = false;
    bool tick_served = false;             // ... answered by the resident tick server instead
    std::vector<int32_t> tick_candidates; // every tracking channel of the bank (what a tick server serves)
    int tick_groups = 0, tick_group_n[2] = {0, 0}, tick_rc = 0;
    int64_t tick_write_index = 0;
};

extern "C" {

int sdr_track_cluster(sdr_engine* e, int parts) {
    if (!e) return sdr_fail(SDR_ERR_INVALID, "null engine");
    if (parts != 0 && parts != 1 && parts != 2 && parts != 4 && parts != 8)
        return sdr_fail(SDR_ERR_INVALID, "cluster size %d: must be 0 (automatic), 1, 2, 4 or 8", parts);
    e->track_force_parts = parts;
    return SDR_OK;
}

int sdr_track_closed_loop(sdr_engine* e, int n_ch, sdr_track_state* st, const sdr_loop_cfg* cfg, int n_epochs,
                          sdr_track_epoch* traj) {
    return sdr_track_closed_loop_bits(e, n_ch, st, cfg, n_epochs, traj, nullptr, 0, nullptr);
}

int sdr_track_closed_loop_bits(sdr_engine* e, int n_ch, sdr_track_state* st, const sdr_loop_cfg* cfg, int n_epochs,
                               sdr_track_epoch* traj, int8_t* nav_bits, int max_bits, int32_t* n_bits) {
    if (n_ch < 1) return sdr_fail(SDR_ERR_INVALID, "bad closed-loop request");
    std::vector<int32_t> done((size_t)n_ch, 0);
    if (int rc = sdr_track_closed_loop_ex(e, n_ch, st, cfg, 0, n_epochs, traj, nav_bits, max_bits, n_bits, done.data()))
        return rc;
    // one status for the whole call (the per-channel outcome is what sdr_track_closed_loop_ex reports); the
    // states handed back are valid either way
    for (int c = 0; c < n_ch; ++c)
        if (done[c] < n_epochs)
            return sdr_fail(SDR_ERR_RANGE, "channel %d stopped after %d epochs: NCO state left the staged replica / ring",
                            c, done[c]);
    return SDR_OK;
}

int sdr_track_closed_loop_ex(sdr_engine* e, int n_ch, sdr_track_state* st, const sdr_loop_cfg* cfgs,
                             int cfg_per_channel, int n_epochs, sdr_track_epoch* traj, int8_t* nav_bits,
                             int max_bits, int32_t* n_bits, int32_t* epochs_done) {
    if (int rc = sdr_set_device(e)) return rc;
    if ((nav_bits && (max_bits < 1 || !n_bits)) || (!nav_bits && n_bits))
        return sdr_fail(SDR_ERR_INVALID, "nav_bits, max_bits and n_bits go together");
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if (!st || !cfgs || n_ch < 1 || n_epochs < 1) return sdr_fail(SDR_ERR_INVALID, "bad closed-loop request");
    const int n_cfg = cfg_per_channel ? n_ch : 1;
    for (int c = 0; c < n_cfg; ++c) {
        if (int rc = check_cfg(&cfgs[c], c)) return rc;
        if (cfgs[c].n_taps != cfgs[0].n_taps)
            return sdr_fail(SDR_ERR_UNSUPPORTED, "channels of one launch must run the same number of taps (%d vs %d)",
                            cfgs[c].n_taps, cfgs[0].n_taps);
    }
    for (int c = 0; c < n_ch; ++c)
        if (int rc = check_state(e, &st[c], c)) return rc;
    StreamCtx* ctx = &e->ctx0;
    const size_t traj_bytes = traj ? (size_t)n_ch * n_epochs * sizeof(sdr_track_epoch) : 0;
    int rc = sdr_devbuf_reserve(e, &e->track_state, (size_t)n_ch * sizeof(sdr_track_state));
    if (!rc) rc = sdr_devbuf_reserve(e, &e->track_cfg, (size_t)n_cfg * sizeof(sdr_loop_cfg));
    if (!rc) rc = sdr_devbuf_reserve(e, &ctx->traj, traj ? traj_bytes : sizeof(sdr_track_epoch));
    const size_t bits_bytes = nav_bits ? (size_t)n_ch * max_bits : 0;
    const size_t head = ((size_t)2 * n_ch * sizeof(int32_t) + 15) & ~(size_t)15;   // [n_bits][epochs_done] then the bits
    if (!rc) rc = sdr_devbuf_reserve(e, &ctx->bits, head + bits_bytes + 16);
    if (rc) return rc;
    TrackRun r;
    r.d_states = (sdr_track_state*)e->track_state.ptr;
    r.d_cfgs = (const sdr_loop_cfg*)e->track_cfg.ptr;
    r.cfg_stride = cfg_per_channel ? 1 : 0;
    r.n_ch = n_ch, r.n_epochs = n_epochs, r.n_taps = cfgs[0].n_taps;
    r.d_traj = (sdr_track_epoch*)ctx->traj.ptr;
    r.keep = traj ? 1 : 0;
    r.d_nbits = nav_bits ? (int32_t*)ctx->bits.ptr : nullptr;
    r.d_done = (int32_t*)ctx->bits.ptr + n_ch;
    r.d_bits = nav_bits ? (int8_t*)ctx->bits.ptr + head : nullptr;
    r.max_bits = max_bits;
    SDR_HIP(hipMemsetAsync(ctx->bits.ptr, 0, head + bits_bytes, ctx->stream));
    SDR_HIP(hipMemcpyAsync(e->track_state.ptr, st, (size_t)n_ch * sizeof(sdr_track_state), hipMemcpyHostToDevice, ctx->stream));
    SDR_HIP(hipMemcpyAsync(e->track_cfg.ptr, cfgs, (size_t)n_cfg * sizeof(sdr_loop_cfg), hipMemcpyHostToDevice, ctx->stream));
    int parts = 1;
    int* d_fault = nullptr;
    if (int rc2 = launch_track(e, ctx, r, &parts, &d_fault)) return rc2;
    int fault_host = 0;
    std::vector<int32_t> done_host((size_t)n_ch, 0);
    SDR_HIP(hipMemcpyAsync(&fault_host, d_fault, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SDR_HIP(hipMemcpyAsync(st, e->track_state.ptr, (size_t)n_ch * sizeof(sdr_track_state), hipMemcpyDeviceToHost, ctx->stream));
    SDR_HIP(hipMemcpyAsync(done_host.data(), r.d_done, (size_t)n_ch * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (traj) SDR_HIP(hipMemcpyAsync(traj, ctx->traj.ptr, traj_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (nav_bits) {
        SDR_HIP(hipMemcpyAsync(nav_bits, r.d_bits, bits_bytes, hipMemcpyDeviceToHost, ctx->stream));
        SDR_HIP(hipMemcpyAsync(n_bits, r.d_nbits, (size_t)n_ch * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    SDR_HIP(hipStreamSynchronize(ctx->stream));
    if (fault_host)
        return sdr_fail(SDR_ERR_HIP, "closed-loop tracking: a workgroup of a %d-part cluster never published its sums", parts);
    if (epochs_done)
        for (int c = 0; c < n_ch; ++c) epochs_done[c] = done_host[c];
    return SDR_OK;
}

/* ------------------------------------------------------------------------------------------ channel bank */

int sdr_bank_create(sdr_engine* e, int max_channels, sdr_bank** out) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!out) return sdr_fail(SDR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (max_channels < 1 || max_channels > 65536) return sdr_fail(SDR_ERR_INVALID, "max_channels %d outside 1..65536", max_channels);
    sdr_bank* b = new (std::nothrow) sdr_bank();
    if (!b) return sdr_fail(SDR_ERR_NOMEM, "host allocation failed");
    b->max_channels = max_channels;
    b->n_taps.assign((size_t)max_channels, 0);
    b->slot.assign((size_t)max_channels, -1);
    hipError_t err = hipMalloc(&b->d_states, (size_t)max_channels * sizeof(sdr_track_state));
    if (err == hipSuccess) err = hipMalloc(&b->d_cfgs, (size_t)max_channels * sizeof(sdr_loop_cfg));
    if (err == hipSuccess) err = hipMemsetAsync(b->d_states, 0, (size_t)max_channels * sizeof(sdr_track_state), e->ctx0.stream);
    if (err == hipSuccess) err = hipMemsetAsync(b->d_cfgs, 0, (size_t)max_channels * sizeof(sdr_loop_cfg), e->ctx0.stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->ctx0.stream);
    if (err != hipSuccess) {
        sdr_bank_destroy(e, b);
        return sdr_fail(err == hipErrorOutOfMemory ? SDR_ERR_NOMEM : SDR_ERR_HIP, "bank setup failed: %s", hipGetErrorString(err));
    }
    *out = b;
    return SDR_OK;
}

void sdr_bank_destroy(sdr_engine* e, sdr_bank* b) {
    if (!b) return;
    if (e) {
        (void)hipSetDevice(e->device);
        (void)sdr_tick_server_stop(e);      // (a resident tick server serves this bank: it leaves before the bank goes)
        (void)hipDeviceSynchronize();
    }
    if (b->d_states) (void)hipFree(b->d_states);
    if (b->d_cfgs) (void)hipFree(b->d_cfgs);
    for (StreamCtx* c : {&b->async_ctx, &b->tick_ctx[0], &b->tick_ctx[1]}) {
        for (DevBuf* d : {&c->traj, &c->bits, &c->xchg})
            if (d->ptr) (void)hipFree(d->ptr);
        if (c->pinned) (void)hipHostFree(c->pinned);
    }
    sdr_bank_free_pending(b);
    delete b;
}

int sdr_bank_put(sdr_engine* e, sdr_bank* b, int ch, const sdr_track_state* st, const sdr_loop_cfg* cfg) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!b || !st || !cfg) return sdr_fail(SDR_ERR_INVALID, "NULL bank, state or configuration");
    if (ch < 0 || ch >= b->max_channels) return sdr_fail(SDR_ERR_RANGE, "channel %d outside the bank's %d", ch, b->max_channels);
    if (b->tick_open) return sdr_fail(SDR_ERR_STATE, "a tick of this bank is in flight: sdr_bank_tick_mirrored_end first");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if (int rc = check_cfg(cfg, ch)) return rc;
    if (int rc = check_state(e, st, ch)) return rc;
    hipStream_t s = e->ctx0.stream;
    SDR_HIP(hipMemcpyAsync(b->d_states + ch, st, sizeof(*st), hipMemcpyHostToDevice, s));
    SDR_HIP(hipMemcpyAsync(b->d_cfgs + ch, cfg, sizeof(*cfg), hipMemcpyHostToDevice, s));
    SDR_HIP(hipStreamSynchronize(s));
    b->n_taps[ch] = cfg->n_taps;
    b->slot[ch] = st->code_slot;
    return SDR_OK;
}

int sdr_bank_get(sdr_engine* e, sdr_bank* b, int ch, sdr_track_state* st) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!b || !st) return sdr_fail(SDR_ERR_INVALID, "NULL bank or state");
    if (ch < 0 || ch >= b->max_channels) return sdr_fail(SDR_ERR_RANGE, "channel %d outside the bank's %d", ch, b->max_channels);
    if (!b->n_taps[ch]) return sdr_fail(SDR_ERR_STATE, "channel %d was never put into the bank", ch);
    SDR_HIP(hipMemcpyAsync(st, b->d_states + ch, sizeof(*st), hipMemcpyDeviceToHost, e->ctx0.stream));
    SDR_HIP(hipStreamSynchronize(e->ctx0.stream));
    return SDR_OK;
}

// Diagnostics build (-DSDR_TICK_TIMING): where the host side of a one-epoch step spends its time (stderr, every 128 calls).
#ifdef SDR_TICK_TIMING
static double g_tick_t[8], g_tick_sum[8];
static long g_tick_calls;
#define TICK_CLOCK(k) g_tick_t[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count()
#define TICK_REPORT()                                                                                                       \
    do {                                                                                                                    \
        for (int k_ = 1; k_ <= 4; ++k_) g_tick_sum[k_] += g_tick_t[k_] - g_tick_t[k_ - 1];                                  \
        if (++g_tick_calls % 128 == 0) {                                                                                    \
            fprintf(stderr, "[tick timing] prepare %.2f  launch %.2f  wait %.2f  copy-out %.2f us\n", g_tick_sum[1] / 128,   \
                    g_tick_sum[2] / 128, g_tick_sum[3] / 128, g_tick_sum[4] / 128);                                          \
            for (int k_ = 0; k_ < 8; ++k_) g_tick_sum[k_] = 0;                                                              \
        }                                                                                                                   \
    } while (0)
#else
#define TICK_CLOCK(k) ((void)0)
#define TICK_REPORT() ((void)0)
#endif

// A bank step whose launch and result copies are queued but not waited for (sdr_bank_step_begin / _end).
struct BankPending {
    bool active = false;
    StreamCtx* ctx = nullptr;
    int n_ch = 0, n_epochs = 0, parts = 1;
    int32_t* p_head = nullptr;
    sdr_track_state* p_states = nullptr;
    sdr_track_epoch* p_rec = nullptr;
    int8_t* p_bits = nullptr;
    size_t rec_bytes = 0, st_bytes = 0, bits_bytes = 0;
    volatile unsigned* done_words = nullptr;   // (results straight into page-locked memory) the channels' done words ...
    unsigned done_seq = 0;                     // ... and what they show when a channel's results are there
};

static void sdr_bank_free_pending(sdr_bank* b) {
    delete b->pending;
    b->pending = nullptr;
    for (int g = 0; g < 2; ++g) {
        delete b->tick_pending[g];
        b->tick_pending[g] = nullptr;
    }
}

// What is left of a step once everything is queued: wait, check, hand the results out of the page-locked block.
static int bank_collect(BankPending& P, sdr_track_epoch* records, sdr_track_state* states_out, int32_t* epochs_done, int8_t* nav_bits,
                        int32_t* n_bits) {
    P.active = false;
#ifdef SDR_TICK_TIMING
    {   // (how long before the stream's signal are the channels' results in page-locked memory?)
        static double early_sum; static long early_n;
        const double t0 = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
        volatile int32_t* done = P.p_head + 4;
        long spins = 0;
        for (int c = 0; c < P.n_ch; ++c) while (!done[c] && ++spins < 2000000) {}
        const double t1 = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
        (void)hipStreamSynchronize(P.ctx->stream);
        const double t2 = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
        early_sum += t2 - t1;
        if (++early_n % 128 == 0) {
            fprintf(stderr, "[tick timing] results seen %.2f us after the wait began, the stream's signal %.2f us after that\n", t1 - t0, early_sum / 128);
            early_sum = 0;
        }
    }
#endif
    // The results are in page-locked memory ~9 us before the stream says so (the kernel's end, its release, the signal, the
    // runtime's wake-up: measured on the receiver tick, 18.6 against 27.8 us after the wait began): every channel raises a word
    // behind its results, and those are what is waited for.  Bounded: a launch that died never raises them -- the stream is
    // asked then, and says why.
    bool seen = false;
    if (P.done_words) {
        const auto t0 = std::chrono::steady_clock::now();
        int c = 0;
        for (long spins = 0;; ++spins) {
            while (c < P.n_ch && __atomic_load_n(&P.done_words[c], __ATOMIC_ACQUIRE) == P.done_seq) ++c;
            if (c == P.n_ch) {
                seen = true;
                break;
            }
            if ((spins & 4095) == 4095 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.02) break;
        }
    }
    if (!seen) {
        if (P.done_words) P.ctx->xchg_tagged = nullptr;      // (whatever kept the words from coming: the next tick zeroes lines and ticket counters)
        SDR_HIP(hipStreamSynchronize(P.ctx->stream));
    }
    TICK_CLOCK(3);
    if (P.p_head[0]) P.ctx->xchg_tagged = nullptr;     // (a part that never showed up has drawn no ticket: start the counters over)
    if (P.p_head[0] == 2)
        return sdr_fail(SDR_ERR_HIP, "closed-loop tracking: the slab the tick's launch was to pull into the ring never arrived");
    if (P.p_head[0])
        return sdr_fail(SDR_ERR_HIP, "closed-loop tracking: a workgroup of a %d-part cluster never published its sums", P.parts);
    if (epochs_done) memcpy(epochs_done, P.p_head + 4, (size_t)P.n_ch * sizeof(int32_t));
    if (nav_bits) {
        memcpy(n_bits, P.p_head + 4 + P.n_ch, (size_t)P.n_ch * sizeof(int32_t));
        memcpy(nav_bits, P.p_bits, P.bits_bytes);
    }
    if (states_out) memcpy(states_out, P.p_states, P.st_bytes);
    if (records) memcpy(records, P.p_rec, P.rec_bytes);
    TICK_CLOCK(4);
    TICK_REPORT();
    return SDR_OK;
}

// Shared by sdr_bank_step / sdr_bank_tick: everything between the optional ingest and the final synchronisation.
// defer != nullptr: queue only (records and states are produced whatever the pointers say) and describe the step in *defer.
static int bank_run(sdr_engine* e, sdr_bank* b, StreamCtx* ctx, const int32_t* channels, int n_ch, int n_epochs,
                    sdr_track_epoch* records, sdr_track_state* states_out, int32_t* epochs_done, int8_t* nav_bits,
                    int max_bits, int32_t* n_bits, BankPending* defer = nullptr) {
    TICK_CLOCK(0);
    if (defer) {   // (any non-null value: the queueing part below only asks whether they are wanted)
        records = reinterpret_cast<sdr_track_epoch*>(defer);
        states_out = reinterpret_cast<sdr_track_state*>(defer);
    }
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!e->codes) return sdr_fail(SDR_ERR_STATE, "code slots not allocated");
    if ((nav_bits && (max_bits < 1 || !n_bits)) || (!nav_bits && n_bits))
        return sdr_fail(SDR_ERR_INVALID, "nav_bits, max_bits and n_bits go together");
    if (!channels || n_ch < 1 || n_epochs < 1) return sdr_fail(SDR_ERR_INVALID, "bad bank step request");
    int nt = 0;
    for (int c = 0; c < n_ch; ++c) {
        const int ch = channels[c];
        if (ch < 0 || ch >= b->max_channels || !b->n_taps[ch])
            return sdr_fail(SDR_ERR_INVALID, "entry %d: channel %d is not in the bank", c, ch);
        if (b->slot[ch] >= e->n_slots || e->code_len_host[b->slot[ch]] <= 0)
            return sdr_fail(SDR_ERR_STATE, "entry %d: channel %d's code slot %d is no longer staged", c, ch, b->slot[ch]);
        if (nt && b->n_taps[ch] != nt)
            return sdr_fail(SDR_ERR_UNSUPPORTED, "channels of one step must run the same number of taps (%d vs %d)", b->n_taps[ch], nt);
        nt = b->n_taps[ch];
        for (int d = 0; d < c; ++d)
            if (channels[d] == ch) return sdr_fail(SDR_ERR_INVALID, "channel %d listed twice", ch);
    }
    const size_t rec_bytes = records ? (size_t)n_ch * n_epochs * sizeof(sdr_track_epoch) : 0;
    const size_t st_bytes = (size_t)n_ch * sizeof(sdr_track_state);
    const size_t bits_bytes = nav_bits ? (size_t)n_ch * max_bits : 0;
    const size_t head = ((size_t)3 * n_ch * sizeof(int32_t) + 15) & ~(size_t)15;  // [map][n_bits][epochs_done], then the bits
    // page-locked block: [fault (4 words)][epochs_done n][n_bits n][channel list n][done words n] [states][records][bits]
    const size_t pin_head = ((size_t)(4 + 4 * n_ch) * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t pin_bytes = pin_head + st_bytes + rec_bytes + bits_bytes;
    int rc = sdr_pinned_reserve(e, ctx, pin_bytes);
    if (rc) return rc;
    char* pin = (char*)ctx->pinned;
    int32_t* p_head = (int32_t*)pin;
    sdr_track_state* p_states = (sdr_track_state*)(pin + pin_head);
    sdr_track_epoch* p_rec = (sdr_track_epoch*)(pin + pin_head + st_bytes);
    int8_t* p_bits = (int8_t*)(pin + pin_head + st_bytes + rec_bytes);
    // A receiver tick (or any step with a few KB of results) has the kernel read its channel list from, and write its
    // outputs straight into, the page-locked block -- it is device-accessible -- so the call is one launch and one
    // synchronisation, with no copy commands around them (each costs the stream several microseconds).  Steps with
    // long trajectories keep device buffers and copy once at the end.
    const bool direct = pin_bytes <= 96u * 1024u;
    if (!direct) {
        rc = sdr_devbuf_reserve_on(e, ctx->stream, &ctx->traj, records ? rec_bytes : sizeof(sdr_track_epoch));
        if (!rc) rc = sdr_devbuf_reserve_on(e, ctx->stream, &ctx->bits, head + bits_bytes + 16);
    } else if (!records) {
        rc = sdr_devbuf_reserve_on(e, ctx->stream, &ctx->traj, sizeof(sdr_track_epoch));   // (the kernel's scratch record)
    }
    if (rc) return rc;
    memset(p_head, 0, pin_head);
    memcpy(p_head + 4 + 2 * n_ch, channels, (size_t)n_ch * sizeof(int32_t));  // (the caller's list is not kept past return)
    TrackRun r;
    r.d_states = b->d_states;
    r.d_cfgs = b->d_cfgs;
    r.cfg_stride = 1;
    r.n_ch = n_ch, r.n_epochs = n_epochs, r.n_taps = nt;
    r.keep = records ? 1 : 0;
    r.max_bits = max_bits;
    bool identity = true;             // channels 0 .. n-1 in order (a receiver's usual tick): the kernel needs no list
    for (int c = 0; c < n_ch && identity; ++c) identity = channels[c] == c;
    if (direct) {
        r.d_map = identity ? nullptr : p_head + 4 + 2 * n_ch;   // (a list in page-locked memory costs every workgroup a PCIe round trip)
        r.d_done = p_head + 4;
        r.d_nbits = nav_bits ? p_head + 4 + n_ch : nullptr;
        r.d_bits = nav_bits ? p_bits : nullptr;
        r.d_traj = records ? p_rec : (sdr_track_epoch*)ctx->traj.ptr;
        r.d_states_copy = states_out ? p_states : nullptr;
        r.fault_word = p_head;
        r.done_words = (unsigned*)(p_head + 4 + 3 * n_ch);      // (zeroed with the head above)
        r.done_seq = ++ctx->done_seq ? ctx->done_seq : ++ctx->done_seq;
        if (nav_bits) memset(p_bits, 0, bits_bytes);
    } else {
        int32_t* d_map = (int32_t*)ctx->bits.ptr;
        r.d_map = d_map;
        r.d_traj = (sdr_track_epoch*)ctx->traj.ptr;
        r.d_nbits = nav_bits ? d_map + n_ch : nullptr;
        r.d_done = d_map + 2 * n_ch;
        r.d_bits = nav_bits ? (int8_t*)ctx->bits.ptr + head : nullptr;
        SDR_HIP(hipMemsetAsync(ctx->bits.ptr, 0, head + bits_bytes, ctx->stream));
        SDR_HIP(hipMemcpyAsync(d_map, p_head + 4 + 2 * n_ch, (size_t)n_ch * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    int parts = 1;
    int* d_fault = nullptr;
    TICK_CLOCK(1);
    if (int rc2 = launch_track(e, ctx, r, &parts, &d_fault)) return rc2;
    TICK_CLOCK(2);
    if (!direct) {
        SDR_HIP(hipMemcpyAsync(p_head, d_fault, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        SDR_HIP(hipMemcpyAsync(p_head + 4, r.d_done, (size_t)n_ch * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (nav_bits) SDR_HIP(hipMemcpyAsync(p_head + 4 + n_ch, r.d_nbits, (size_t)n_ch * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        if (states_out) {
            // contiguous runs of channel indices come back in one copy each
            int c = 0;
            while (c < n_ch) {
                int run = 1;
                while (c + run < n_ch && channels[c + run] == channels[c] + run) ++run;
                SDR_HIP(hipMemcpyAsync(p_states + c, b->d_states + channels[c], (size_t)run * sizeof(sdr_track_state),
                                       hipMemcpyDeviceToHost, ctx->stream));
                c += run;
            }
        }
        if (records) SDR_HIP(hipMemcpyAsync(p_rec, ctx->traj.ptr, rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
        if (nav_bits) SDR_HIP(hipMemcpyAsync(p_bits, r.d_bits, bits_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    BankPending local;
    BankPending& P = defer ? *defer : local;
    P.active = true, P.ctx = ctx, P.n_ch = n_ch, P.n_epochs = n_epochs, P.parts = parts;
    P.p_head = p_head, P.p_states = p_states, P.p_rec = p_rec, P.p_bits = p_bits;
    P.rec_bytes = rec_bytes, P.st_bytes = st_bytes, P.bits_bytes = bits_bytes;
    P.done_words = r.done_words, P.done_seq = r.done_seq;
    if (defer) return SDR_OK;
    return bank_collect(P, records, states_out, epochs_done, nav_bits, n_bits);
}

int sdr_bank_step(sdr_engine* e, sdr_bank* b, const int32_t* channels, int n_ch, int n_epochs,
                  sdr_track_epoch* records, sdr_track_state* states_out, int32_t* epochs_done,
                  int8_t* nav_bits, int max_bits, int32_t* n_bits, int stream_id) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!b) return sdr_fail(SDR_ERR_INVALID, "bank is NULL");
    if (b->tick_open) return sdr_fail(SDR_ERR_STATE, "a tick of this bank is in flight: sdr_bank_tick_mirrored_end first");
    StreamCtx* ctx = sdr_stream_ctx(e, stream_id);
    if (!ctx) return sdr_fail(SDR_ERR_INVALID, "stream id %d does not exist", stream_id);
    if (int rc = sdr_iq_order_reader(e, ctx)) return rc;      // (behind the uploads queued on the engine's stream so far)
    return bank_run(e, b, ctx, channels, n_ch, n_epochs, records, states_out, epochs_done, nav_bits, max_bits, n_bits);
}

// sdr_bank_step in two halves.  _begin queues the launch and the copies of its results into page-locked memory on the
// engine's stream and returns; _end waits for them and hands them out.  One step may be in flight per bank; whatever is
// queued on the stream in between (a tick, an upload) runs after the step, as the stream orders it.
int sdr_bank_step_begin(sdr_engine* e, sdr_bank* b, const int32_t* channels, int n_ch, int n_epochs) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!b) return sdr_fail(SDR_ERR_INVALID, "bank is NULL");
    if (b->tick_open) return sdr_fail(SDR_ERR_STATE, "a tick of this bank is in flight: sdr_bank_tick_mirrored_end first");
    if (!b->pending) b->pending = new BankPending();
    if (b->pending->active) return sdr_fail(SDR_ERR_STATE, "a step of this bank is already in flight: sdr_bank_step_end first");
    b->async_ctx.stream = e->ctx0.stream;
    return bank_run(e, b, &b->async_ctx, channels, n_ch, n_epochs, nullptr, nullptr, nullptr, nullptr, 0, nullptr, b->pending);
}

int sdr_bank_step_end(sdr_engine* e, sdr_bank* b, sdr_track_epoch* records, sdr_track_state* states_out, int32_t* epochs_done) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!b) return sdr_fail(SDR_ERR_INVALID, "bank is NULL");
    if (!b->pending || !b->pending->active) return sdr_fail(SDR_ERR_STATE, "no step of this bank is in flight");
    return bank_collect(*b->pending, records, states_out, epochs_done, nullptr, nullptr);
}


}  // extern "C"

// ------------------------------------------------------------------------------------------- the tick server, host side
struct TickServerState {
    sdr_bank* bank = nullptr;
    std::vector<int32_t> channels;          // the channels it serves (every tracking channel of the bank when it started), ascending
    int parts = 0, n_taps = 0;
    StreamCtx ctx;                          // the trackers' own stream and exchange lines
    hipStream_t door_stream = nullptr;      // the doorman's
    TickServerHost* host = nullptr;         // page-locked: control words, then [ran][states][records]
    size_t host_bytes = 0;
    int* h_ran = nullptr;
    sdr_track_state* h_st = nullptr;
    sdr_track_epoch* h_rec = nullptr;
    unsigned* h_done = nullptr;             // per served channel: the last request it has answered
    DevBuf dev;                             // TickServerDev, then [release words][records][channel map]
    unsigned seq = 0;                       // requests posted to the running server
    unsigned pull_seq = 0;                  // slabs announced to it
    unsigned stamps_seq = 0;                // the last request whose stamps went into the sums below
    bool disabled = false;                  // a launch was refused, or a server died at work: plain ticks from then on
    int64_t served_total = 0, starts = 0;   // requests answered / servers started, over the engine's life
    double phase_us[4] = {0, 0, 0, 0};      // summed over the answered requests: slab pull, release, channels' answers, gather
    double tracker_us[6] = {0, 0, 0, 0, 0, 0};
    double seen_us[4] = {0, 0, 0, 0};       // (trace build) release -> the doorman sees 1, n/2, n - 1, n answers
    double fence_add_us = 0;                // channel 0: its release + count, as the NEXT tick's stamps tell (t[6] of the tick before)
    unsigned long long prev_t5 = 0;   // channel 0: release -> seen, -> samples visible, -> correlated, -> exchanged, -> updated, -> answered
    int64_t code_generation = -1;
    void* ring = nullptr;
};

static bool server_wait(volatile unsigned* word, unsigned want, double seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long spins = 0;; ++spins) {
        if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == want) return true;
        if ((spins & 1023) == 1023 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
    }
}

// Every served channel's done word at `want` (bounded; gives up at once when the doorman has left).
#ifdef SDR_SRV_HOSTTRACE
static double g_ht[8]; static long g_htn;
static inline double ht_now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define HT(k, t0) do { const double t1_ = ht_now(); g_ht[k] += t1_ - (t0); (t0) = t1_; } while (0)
#else
#define HT(k, t0) ((void)0)
#endif
static bool server_wait_all(volatile unsigned* words, int n, unsigned want, volatile unsigned* alive, double seconds) {
    const auto t0 = std::chrono::steady_clock::now();
    int k = 0;
    for (long spins = 0;; ++spins) {
        while (k < n && __atomic_load_n(&words[k], __ATOMIC_ACQUIRE) == want) ++k;
        if (k == n) return true;
        if ((spins & 1023) == 1023) {
            if (!__atomic_load_n(alive, __ATOMIC_ACQUIRE)) return false;
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) return false;
        }
    }
}

// The doorman's stamps of the last request it has closed, into the sums sdr_tick_server_phases reports (once per request;
// the doorman closes a request a microsecond or two after the host has its answers: read when the next one is posted).
static void server_absorb_stamps(TickServerState* s) {
    TickServerHost* h = s->host;
    const unsigned closed = __atomic_load_n(&h->done_seq, __ATOMIC_ACQUIRE);
    if (closed == s->stamps_seq || closed != s->seq) return;
    s->stamps_seq = closed;
    for (int k = 0; k < 4; ++k) s->phase_us[k] += (double)(h->stamps[k + 1] - h->stamps[k]) * 0.01;
    if (h->tracker[5] > h->stamps[2]) {     // (channel 0 ran in this tick)
        s->tracker_us[0] += (double)((long long)(h->tracker[0] - h->stamps[2])) * 0.01;
        for (int k = 1; k < 6; ++k) s->tracker_us[k] += (double)((long long)(h->tracker[k] - h->tracker[k - 1])) * 0.01;
#ifdef SDR_SRV_TRACE
        for (int k = 0; k < 4; ++k) s->seen_us[k] += (double)h->tracker[8 + k] * 0.01;
#endif
        if (h->tracker[6] > h->tracker[5]) s->fence_add_us += (double)(h->tracker[6] - h->tracker[5]) * 0.01, s->prev_t5 += 1;
    }
}

// The request line (see TickServerHost): words 1-5, then the numbers' copy, then the numbers.
static void server_post(TickServerState* s, const unsigned long long* words5) {
    TickServerHost* h = s->host;
    for (int k = 0; k < 5; ++k) h->line[1 + k] = words5[k];
    const unsigned long long seqs = (unsigned long long)s->seq | ((unsigned long long)s->pull_seq << 32);
    __atomic_store_n(&h->line[kReqSeqsCopy], seqs, __ATOMIC_RELEASE);
    __atomic_store_n(&h->line[kReqSeqs], seqs, __ATOMIC_RELEASE);
}
static void server_post_stop(TickServerState* s) {
    __atomic_store_n(&s->host->line[kReqSeqsCopy], (unsigned long long)kServerStop, __ATOMIC_RELEASE);
    __atomic_store_n(&s->host->line[kReqSeqs], (unsigned long long)kServerStop, __ATOMIC_RELEASE);
}

int sdr_tick_server_stop(sdr_engine* e) {
    if (e) e->srv_steady_ticks = 0;
    if (!e || !e->srv_running) return SDR_OK;
    TickServerState* s = e->srv;
    e->srv_running = false;
    server_post_stop(s);
    // (the doorman looks at the word every few microseconds; the trackers follow its release word.  Should the words never be
    // seen -- they always are -- every workgroup still leaves by its own clock: the stream synchronisation below ends either way)
    (void)server_wait(&s->host->alive, 0u, 1.0);
    SDR_HIP(hipStreamSynchronize(s->door_stream));
    SDR_HIP(hipStreamSynchronize(s->ctx.stream));
    server_absorb_stamps(s);
    s->seq = s->pull_seq = s->stamps_seq = 0;
    // a slab the server had not pulled yet: into the ring the ordinary way
    if (e->srv_slab_pending) return sdr_iq_flush_server_slab(e);
    return SDR_OK;
}

void sdr_tick_server_free(sdr_engine* e) {
    if (!e || !e->srv) return;
    (void)sdr_tick_server_stop(e);
    TickServerState* s = e->srv;
    for (DevBuf* d : {&s->ctx.traj, &s->ctx.bits, &s->ctx.xchg, &s->dev})
        if (d->ptr) (void)hipFree(d->ptr);
    if (s->ctx.pinned) (void)hipHostFree(s->ctx.pinned);
    if (s->host) (void)hipHostFree(s->host);
    if (s->ctx.stream) (void)hipStreamDestroy(s->ctx.stream);
    if (s->door_stream) (void)hipStreamDestroy(s->door_stream);
    delete s;
    e->srv = nullptr;
}

// Start a server for `channels` (ascending, one tap count, n <= 64 so that the cluster form applies).  On return the
// kernel is queued on the server's own stream; it raises `alive` when it runs.
static int tick_server_start(sdr_engine* e, sdr_bank* b, const int32_t* channels, int n, int nt) {
    if (!e->srv) e->srv = new TickServerState();
    TickServerState* s = e->srv;
    if (!s->ctx.stream) SDR_HIP(hipStreamCreateWithFlags(&s->ctx.stream, hipStreamNonBlocking));
    if (!s->door_stream) SDR_HIP(hipStreamCreateWithFlags(&s->door_stream, hipStreamNonBlocking));
    int parts = 1;
    while (parts < kMaxParts && (long)n * parts * 2 <= (long)e->n_cus) parts *= 2;     // (the cluster a tick of these channels takes)
    if (parts < 2) return sdr_fail(SDR_ERR_UNSUPPORTED, "tick server: %d channels leave no cluster", n);
    const size_t res_bytes = (size_t)n * (sizeof(int) + sizeof(unsigned) + sizeof(sdr_track_state) + sizeof(sdr_track_epoch));
    const size_t host_bytes = ((sizeof(TickServerHost) + 63) & ~(size_t)63) + res_bytes + 64;
    if (host_bytes > s->host_bytes) {
        if (s->host) SDR_HIP(hipHostFree(s->host));
        s->host = nullptr;
        s->host_bytes = 0;
        hipError_t err = hipHostMalloc((void**)&s->host, host_bytes, hipHostMallocDefault);
        if (err != hipSuccess) {
            s->host = nullptr;
            return sdr_fail(SDR_ERR_NOMEM, "hipHostMalloc(%zu) for the tick server failed: %s", host_bytes, hipGetErrorString(err));
        }
        s->host_bytes = host_bytes;
    }
    memset(s->host, 0, host_bytes);
    char* hp = (char*)s->host + ((sizeof(TickServerHost) + 63) & ~(size_t)63);
    s->h_st = (sdr_track_state*)hp;                                   // (8-byte fields first: the channels write 8 bytes per lane)
    s->h_rec = (sdr_track_epoch*)(hp + (size_t)n * sizeof(sdr_track_state));
    s->h_ran = (int*)(hp + (size_t)n * (sizeof(sdr_track_state) + sizeof(sdr_track_epoch)));
    s->h_done = (unsigned*)(s->h_ran + n);
    const size_t dev_head = (sizeof(TickServerDev) + 127) & ~(size_t)127;
    const size_t go_bytes = (size_t)n * kGoStride * sizeof(unsigned);
    const size_t dev_bytes = dev_head + go_bytes + (size_t)n * (sizeof(sdr_track_epoch) + sizeof(int32_t)) + 64;
    if (int rc = sdr_devbuf_reserve_on(e, s->ctx.stream, &s->dev, dev_bytes)) return rc;
    SDR_HIP(hipMemsetAsync(s->dev.ptr, 0, dev_bytes, s->ctx.stream));
    char* dp = (char*)s->dev.ptr + dev_head;
    TickServer a = {};
    a.host = s->host;
    a.dev = (TickServerDev*)s->dev.ptr;
    a.go = (unsigned*)dp;
    a.ring16 = (uint4*)e->iq;
    a.ring_flip = sdr::ring_flip_mask(e->iq_fmt);
    a.ring_n16 = (unsigned long long)((size_t)e->iq_capacity * sdr_fmt_bytes(e->iq_fmt) / 16);
    a.rec_out = (sdr_track_epoch*)(dp + go_bytes);
    int32_t* d_map = (int32_t*)(dp + go_bytes + (size_t)n * sizeof(sdr_track_epoch));
    a.h_ran = s->h_ran, a.h_st = s->h_st, a.h_rec = s->h_rec, a.h_done = s->h_done;
    a.idle_ticks = 20000000ull;      // 0.2 s of the 100 MHz wall clock without a request: leave (the next tick starts a new server)
    a.busy_ticks = 5000000ull;       // 50 ms for the channels' answers to one request: something is wrong, leave
    SDR_HIP(hipMemcpyAsync(d_map, channels, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s->ctx.stream));
    if (int rc = sdr_devbuf_reserve_on(e, s->ctx.stream, &s->ctx.traj, sizeof(sdr_track_epoch))) return rc;
    TrackRun r;
    r.d_states = b->d_states;
    r.d_cfgs = b->d_cfgs;
    r.cfg_stride = 1;
    r.d_map = d_map;
    r.n_ch = n, r.n_epochs = 0x7fffffff, r.n_taps = nt;
    r.keep = 0;
    r.d_traj = (sdr_track_epoch*)s->ctx.traj.ptr;
    r.fault_word = &a.dev->fault;
    r.force_parts = parts;
    r.server = &a;
    int used = 0;
    int* d_fault = nullptr;
    // the trackers first (a cooperative launch: it goes through or is refused as a whole), then the doorman; trackers without
    // a doorman leave by their own clock
    SDR_HIP(hipStreamSynchronize(s->ctx.stream));      // (the control block is zero, the channel list in place)
    if (int rc = launch_track(e, &s->ctx, r, &used, &d_fault)) {
        (void)hipGetLastError();                       // (a refused launch must not surface at somebody else's check)
        return rc;
    }
    hipLaunchKernelGGL(tick_doorman_kernel, dim3(kDoorGroups), dim3(kDoorThreads), 0, s->door_stream, a, n);
    const hipError_t door_err = hipGetLastError();
    // the doorman has to be RESIDENT beside the trackers (they fill the device): it says so itself
    if (door_err != hipSuccess || !server_wait(&s->host->alive, 1u, 0.05)) {
        // no doorman: tell it (should it still arrive) and the trackers (they poll the device word) to leave, wait for them
        server_post_stop(s);
        (void)hipMemsetAsync(a.go, 0xFF, go_bytes, e->ctx0.stream);
        (void)hipStreamSynchronize(e->ctx0.stream);
        (void)hipStreamSynchronize(s->ctx.stream);
        (void)hipStreamSynchronize(s->door_stream);
        return sdr_fail(SDR_ERR_HIP, "tick server: the doorman did not become resident beside the trackers (%s)",
                        door_err != hipSuccess ? hipGetErrorString(door_err) : "no room on a compute unit");
    }
    s->bank = b;
    s->channels.assign(channels, channels + n);
    s->parts = parts, s->n_taps = nt;
    s->seq = s->pull_seq = s->stamps_seq = 0;
    s->code_generation = e->code_generation;
    s->ring = e->iq;
    s->starts += 1;
    e->srv_running = true;
    return SDR_OK;
}

extern "C" {

int sdr_bank_tick(sdr_engine* e, sdr_bank* b, const void* iq, int64_t n_samples, int64_t ring_offset,
                  const int32_t* channels, int n_ch, sdr_track_epoch* records, sdr_track_state* states_out,
                  int32_t* epochs_done) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!b) return sdr_fail(SDR_ERR_INVALID, "bank is NULL");
    if (b->tick_open) return sdr_fail(SDR_ERR_STATE, "a tick of this bank is in flight: sdr_bank_tick_mirrored_end first");
    if (n_samples > 0)
        if (int rc = sdr_iq_upload_async(e, iq, n_samples, ring_offset)) return rc;
    if (n_ch == 0) {
        SDR_HIP(hipStreamSynchronize(e->ctx0.stream));
        return SDR_OK;
    }
    return bank_run(e, b, &e->ctx0, channels, n_ch, 1, records, states_out, epochs_done, nullptr, 0, nullptr);
}


// The tick with its bookkeeping here instead of in the caller's language: which channels are ready (channel.py:137-146
// -- the ring holds their next epoch completely), their epoch, and the caller's mirrors brought up to date in place.
// In two halves so that ONE host thread can drive several devices (channelManager.py:149-188 starts every channel
// before it waits for any): _begin decides who is ready and queues their epoch -- nothing is waited for -- and _end waits,
// absorbs the results into the mirrors and writes the tick's update rows.  sdr_bank_tick_mirrored is the two in a row.
int sdr_bank_tick_mirrored_begin(sdr_engine* e, sdr_bank* b, const void* iq, int64_t n_samples, int64_t ring_offset,
                                 int64_t write_index, sdr_tick_mirror* m) {
#ifdef SDR_SRV_HOSTTRACE
    double ht0 = ht_now();
#endif
    if (int rc = sdr_set_device_keep(e)) return rc;        // (a resident tick server stays: this may be its next request)
    if (!b) return sdr_fail(SDR_ERR_INVALID, "bank is NULL");
    if (b->tick_open) return sdr_fail(SDR_ERR_STATE, "a tick of this bank is already in flight: sdr_bank_tick_mirrored_end first");
    if (!m || !m->states || !m->last || !m->tracking || !m->lost || !m->ran || !m->records || !m->updates)
        return sdr_fail(SDR_ERR_INVALID, "tick mirror: a required array is NULL");
    if (m->max_channels != b->max_channels)
        return sdr_fail(SDR_ERR_INVALID, "tick mirror has %d rows, the bank %d channels", m->max_channels, b->max_channels);
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    const int64_t cap = e->iq_capacity;
    if (write_index < 0 || write_index >= cap) return sdr_fail(SDR_ERR_RANGE, "write index outside the ring");
    if (n_samples > 0)
        if (int rc = sdr_iq_upload_async(e, iq, n_samples, ring_offset)) return rc;
    auto unread_of = [&](int ch) {
        int64_t cur = m->states[ch].current_sample % cap;
        if (cur < 0) cur += cap;
        return cur <= write_index ? write_index - cur : cap - cur + write_index;   // circularbuffer.py:139-148
    };
    // ready channels, grouped by tap count (one launch per group: the kernels are compiled per tap count)
    std::vector<int32_t>& list = b->tick_list;
    m->n_ran = m->n_nav_bits = m->n_lost = 0;
    int taps_seen[2] = {0, 0};
    list.clear();
    for (int ch = 0; ch < b->max_channels; ++ch) {
        if (!m->tracking[ch] || m->lost[ch] || !b->n_taps[ch]) continue;
        if (unread_of(ch) < m->states[ch].n_samples) continue;
        list.push_back(ch);
        const int nt = b->n_taps[ch];
        if (taps_seen[0] == 0 || taps_seen[0] == nt) taps_seen[0] = nt;
        else taps_seen[1] = nt;
    }
    b->tick_write_index = write_index;
    b->tick_slab_queued = n_samples > 0;
    b->tick_rc = SDR_OK;
    b->tick_groups = 0;
    b->tick_two = taps_seen[1] != 0;
    b->tick_served = false;
    // ---- the resident tick server ("tick_server"): the request goes to the kernel that is already there
    if (e->tick_server_opt && !(e->srv && e->srv->disabled) && !b->tick_two && !e->track_force_parts && !e->track_one_launch_tick &&
        !e->prof && !(b->pending && b->pending->active)) {
        // the server serves EVERY tracking channel of the bank (who is ready is decided there, as it is above)
        std::vector<int32_t>& cand = b->tick_candidates;
        cand.clear();
        int nt = 0;
        bool one_tap_count = true;
        for (int ch = 0; ch < b->max_channels; ++ch) {
            if (!m->tracking[ch] || m->lost[ch] || !b->n_taps[ch]) continue;
            cand.push_back(ch);
            if (nt && b->n_taps[ch] != nt) one_tap_count = false;
            nt = b->n_taps[ch];
        }
        TickServerState* s = e->srv;
        if (e->srv_running && !__atomic_load_n(&s->host->alive, __ATOMIC_ACQUIRE)) {
            // the server has left by its own clock (0.2 s without a request: a host that paused) -- or given up: tidy up after
            // it (its streams, the channels' states it wrote on the way out); this tick and the next few are plain ones
            const unsigned why = __atomic_load_n(&s->host->fault, __ATOMIC_ACQUIRE);
            if (int rc = sdr_tick_server_stop(e)) return rc;
            if (why >= 2) s->disabled = true;
        }
        const bool same = e->srv_running && s->bank == b && s->channels == cand && s->code_generation == e->code_generation &&
                          s->ring == e->iq;
        bool use = one_tap_count && !cand.empty() && (long)cand.size() * 4 <= (long)e->n_cus;
        // A server costs ~25 ms to start (a cooperative launch, the doormen becoming resident): it is started for a receiver
        // that HAS settled into steady ticks -- eight in a row with nothing else on the engine in between -- not for the
        // ticks between two other calls (a manager that replays read-ahead blocks uploads and steps in between).
        if (use && !same && ++e->srv_steady_ticks < 8) use = false;
        if (use && !same) {
            if (e->srv_running)
                if (int rc = sdr_tick_server_stop(e)) return rc;
            // (what is queued on the engine's stream -- an ingest, the states a put uploaded -- is done before the server reads it)
            SDR_HIP(hipStreamSynchronize(e->ctx0.stream));
            if (int rc = tick_server_start(e, b, cand.data(), (int)cand.size(), nt)) {
                (void)rc;                       // refused (no room for the cooperative launch, ...): plain ticks from now on
                if (e->srv) e->srv->disabled = true;
                use = false;
            }
        }
        if (!use && e->srv_running)
            if (int rc = sdr_tick_server_stop(e)) return rc;
        if (use) {
            s = e->srv;
            // a slab that went into the ring the ordinary way while the server was resident (a second sdr_iq_upload_begin before
            // this tick: sdr_iq_flush_server_slab) is an ingest kernel on the engine's stream: it has to be IN the ring before
            // the trackers are released on it
            if (e->slab_busy[0] || e->slab_busy[1]) {
                SDR_HIP(hipStreamSynchronize(e->ctx0.stream));
                e->slab_busy[0] = e->slab_busy[1] = false;
            }
            HT(0, ht0);                       // begin: checks, ready list
            server_absorb_stamps(s);          // (the request before this one: the doorman has closed it long since)
            HT(1, ht0);                       // absorb
            // The slab this tick brought (staged by sdr_iq_upload_begin while the server was resident) is announced WITH the
            // request, not when it was staged: pulled earlier, its 800 cache lines are taken out of the host core's cache while
            // the caller is still at work between the two calls -- measured from Python: 43.1 us per tick against 36.4.
            unsigned long long words[5] = {(unsigned long long)write_index, 0, 0, 0, 0};
            if (e->srv_slab_pending) {
                const size_t sb = sdr_fmt_bytes(e->iq_fmt);
                words[1] = (unsigned long long)((uintptr_t)e->srv_slab_src / 16);
                words[2] = (unsigned long long)((size_t)e->srv_slab_n * sb / 16);
                words[3] = (unsigned long long)((size_t)e->srv_slab_off * sb / 16);
                words[4] = ++s->pull_seq;
            }
            ++s->seq;
            server_post(s, words);
            HT(2, ht0);                       // post
            b->tick_served = true;
            b->tick_open = true;
            return SDR_OK;
        }
    } else if (e->srv_running) {
        if (int rc = sdr_tick_server_stop(e)) return rc;
    } else {
        e->srv_steady_ticks = 0;
    }
    if (list.empty() && e->srv_slab_pending)        // (nobody to take it along: the slab goes into the ring the ordinary way)
        if (int rc = sdr_iq_flush_server_slab(e)) return rc;
    if (!list.empty()) {
        int n = (int)list.size();
        b->tick_states.resize((size_t)n);
        b->tick_done.resize((size_t)n);
        if (!b->tick_pending[0]) b->tick_pending[0] = new BankPending();
        if (b->tick_two && !b->tick_pending[1]) b->tick_pending[1] = new BankPending();
        b->tick_ctx[0].stream = b->tick_ctx[1].stream = e->ctx0.stream;      // (the engine's stream, the bank's scratch)
        int at = 0;
        for (int g = 0; g < 2 && taps_seen[g]; ++g) {
            // (stable partition: the group's channels to the front of the remaining range, ascending)
            int n_g = n - at;
            if (taps_seen[1]) {
                n_g = (int)(std::stable_partition(list.begin() + at, list.end(),
                                                  [&](int32_t ch) { return b->n_taps[ch] == taps_seen[g]; }) -
                            (list.begin() + at));
            }
            if (int rc = bank_run(e, b, &b->tick_ctx[g], list.data() + at, n_g, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                  b->tick_pending[g])) {
                // a group queued before this one WILL advance its channels on the device: its results are absorbed by _end
                // (the caller's mirrors must keep matching the bank), which then returns the error
                if (at == 0) return rc;
                b->tick_rc = rc;
                list.resize((size_t)at);
                break;
            }
            b->tick_group_n[g] = n_g;
            b->tick_groups = g + 1;
            at += n_g;
        }
    }
    b->tick_open = true;
    return SDR_OK;
}

int sdr_bank_tick_mirrored_end(sdr_engine* e, sdr_bank* b, sdr_tick_mirror* m) {
    if (int rc = sdr_set_device_keep(e)) return rc;
    if (!b) return sdr_fail(SDR_ERR_INVALID, "bank is NULL");
    if (!b->tick_open) return sdr_fail(SDR_ERR_STATE, "no tick of this bank is in flight");
    if (!m || !m->states || !m->last || !m->tracking || !m->lost || !m->ran || !m->records || !m->updates || m->max_channels != b->max_channels)
        return sdr_fail(SDR_ERR_INVALID, "tick mirror: not the one the tick was begun with");
    b->tick_open = false;
    const int64_t cap = e->iq_capacity, write_index = b->tick_write_index;
    auto unread_of = [&](int ch) {
        int64_t cur = m->states[ch].current_sample % cap;
        if (cur < 0) cur += cap;
        return cur <= write_index ? write_index - cur : cap - cur + write_index;
    };
    std::vector<int32_t>& list = b->tick_list;
    int run_rc = b->tick_rc;
    if (b->tick_served) {
        // ---- the answer of the resident server: wait for its done word (bounded), take the listed channels' rows
        TickServerState* s = e->srv;
        TickServerHost* h = s->host;
#ifdef SDR_SRV_HOSTTRACE
        double ht0 = ht_now();
#endif
        const bool answered = server_wait_all(s->h_done, (int)s->channels.size(), s->seq, &h->alive, 0.25);
        HT(3, ht0);                           // wait
        if (!answered) {
            const unsigned alive = __atomic_load_n(&h->alive, __ATOMIC_ACQUIRE), why = __atomic_load_n(&h->fault, __ATOMIC_ACQUIRE);
            if (!alive && why <= 1) {
                // the doorman left by its idle clock just as this request was posted: it never saw it (a doorman that sees a
                // request answers it), no channel has moved.  The server is tidied up and the tick done over the plain way.
                if (int rc = sdr_tick_server_stop(e)) return rc;
                b->tick_served = false;
                if (int rc = sdr_bank_tick_mirrored_begin(e, b, nullptr, 0, 0, b->tick_write_index, m)) return rc;
                return sdr_bank_tick_mirrored_end(e, b, m);
            }
            (void)sdr_tick_server_stop(e);
            s->disabled = true;
            return sdr_fail(SDR_ERR_HIP, "the resident tick server did not answer request %u (alive %u, fault %u): stopped; plain "
                                         "ticks from now on -- the bank's channels may have advanced, read them back (sdr_bank_get)",
                            s->seq, alive, why);
        }
        s->served_total += 1;
        if (e->srv_slab_pending) {              // (the doorman has pulled it: its staging half is free again)
            e->srv_slab_pending = false;
            if (e->srv_slab_half >= 0) e->slab_busy[e->srv_slab_half] = false;
        }
        bool xchg_fault = __atomic_load_n(&h->fault, __ATOMIC_ACQUIRE) != 0;
        for (size_t c = 0; c < s->channels.size(); ++c) xchg_fault = xchg_fault || s->h_ran[c] == -2;
        if (xchg_fault) {
            (void)sdr_tick_server_stop(e);
            s->disabled = true;
            return sdr_fail(SDR_ERR_HIP, "closed-loop tracking: a workgroup of a %d-part cluster never published its sums (tick server)", s->parts);
        }
        const int n = (int)list.size();
        b->tick_states.resize((size_t)n);
        b->tick_done.resize((size_t)n);
        size_t k = 0;
        int i = 0;
        for (size_t c = 0; c < s->channels.size(); ++c) {
            const int ch = s->channels[c];
            const bool listed = i < n && list[(size_t)i] == ch;
            const int ran = s->h_ran[c];
            if (listed != (ran != 0)) {
                (void)sdr_tick_server_stop(e);
                s->disabled = true;
                return sdr_fail(SDR_ERR_STATE, "tick server: channel %d %s on the device but the mirror says otherwise -- the mirror and "
                                               "the bank disagree", ch, ran ? "ran" : "did not run");
            }
            if (!listed) continue;
            b->tick_states[(size_t)i] = s->h_st[c];
            b->tick_done[(size_t)i] = ran == 1 ? 1 : 0;
            m->records[i] = s->h_rec[c];
            if (ran != 1) b->tick_states[(size_t)i] = m->states[ch];        // (stopped before its epoch: the state it had)
            ++i, ++k;
        }
        if (i != n) {
            (void)sdr_tick_server_stop(e);
            s->disabled = true;
            return sdr_fail(SDR_ERR_STATE, "tick server: a listed channel is not among the channels it serves");
        }
        b->tick_two = false;
        b->tick_groups = 0;
        HT(4, ht0);                           // answers copied
#ifdef SDR_SRV_HOSTTRACE
        if (++g_htn % 500 == 0) {
            fprintf(stderr, "host trace (us per tick): begin %.2f absorb %.2f post %.2f wait %.2f copy %.2f\n", g_ht[0] / 500, g_ht[1] / 500,
                    g_ht[2] / 500, g_ht[3] / 500, g_ht[4] / 500);
            for (double& v : g_ht) v = 0;
        }
#endif
    } else if (list.empty()) {
        // (no channel ready: nothing of this tick waits for the stream -- but a slab queued with the tick, or one read IN PLACE
        // out of the caller's page-locked block by an ingest kernel, must be in the ring before the caller has its buffer back)
        if (b->tick_slab_queued || e->inplace_slab_in_flight) SDR_HIP(hipStreamSynchronize(e->ctx0.stream));
    }
    e->inplace_slab_in_flight = false;   // (ready channels: their kernel ran behind the ingest kernel on the same stream)
    if (!list.empty()) {
        int n = (int)list.size();
        int at = 0;
        for (int g = 0; g < b->tick_groups; ++g) {
            const int n_g = b->tick_group_n[g];
            if (int rc = bank_collect(*b->tick_pending[g], m->records + at, b->tick_states.data() + at, b->tick_done.data() + at, nullptr,
                                      nullptr)) {
                if (b->tick_pending[1]) b->tick_pending[1]->active = false;
                return rc;      // (a cluster that never published: the device's state is unknown, nothing to absorb)
            }
            at += n_g;
        }
        if (b->tick_two) {   // back to ascending channel order, records and states with them
            std::vector<int> order((size_t)n);
            for (int i = 0; i < n; ++i) order[(size_t)i] = i;
            std::sort(order.begin(), order.end(), [&](int x, int y) { return list[(size_t)x] < list[(size_t)y]; });
            std::vector<int32_t> l2((size_t)n), d2((size_t)n);
            std::vector<sdr_track_state> s2((size_t)n);
            std::vector<sdr_track_epoch> r2((size_t)n);
            for (int i = 0; i < n; ++i) {
                const size_t o = (size_t)order[(size_t)i];
                l2[(size_t)i] = list[o], d2[(size_t)i] = b->tick_done[o], s2[(size_t)i] = b->tick_states[o], r2[(size_t)i] = m->records[o];
            }
            list = l2, b->tick_done = d2, b->tick_states = s2;
            memcpy(m->records, r2.data(), (size_t)n * sizeof(sdr_track_epoch));
        }
        // mirrors; a channel the device parked (its NCO left the replica / the ring) reports no epoch
        int w = 0;
        for (int i = 0; i < n; ++i) {
            const int ch = list[(size_t)i];
            m->states[ch] = b->tick_states[(size_t)i];
            if (b->tick_done[(size_t)i] < 1) {
                m->lost[ch] = 1;
                ++m->n_lost;
                continue;
            }
            if (w != i) m->records[w] = m->records[i];
            m->last[ch] = m->records[w];
            if (m->epochs_since_tow) m->epochs_since_tow[ch] += 1;
            if (m->records[w].nav_bit >= 0) ++m->n_nav_bits;
            m->ran[w++] = ch;
        }
        m->n_ran = w;
    }
    // what each tracking channel's CHANNEL_UPDATE reports after this tick (channel.py:205-228)
    int nu = 0;
    int64_t max_unread = 0;
    for (int ch = 0; ch < b->max_channels; ++ch) {
        if (!m->tracking[ch]) continue;
        sdr_tick_update& u = m->updates[nu++];
        u.channel = ch;
        u.track_flags = m->states[ch].track_flags | (m->host_flags ? (int32_t)m->host_flags[ch] : 0);
        u.unread = unread_of(ch);
        u.epochs_since_tow = m->epochs_since_tow ? m->epochs_since_tow[ch] : 0;
        if (!m->lost[ch] && u.unread > max_unread) max_unread = u.unread;
    }
    m->n_updates = nu;
    m->max_unread = max_unread;
    return run_rc;
}

int sdr_bank_tick_mirrored(sdr_engine* e, sdr_bank* b, const void* iq, int64_t n_samples, int64_t ring_offset,
                           int64_t write_index, sdr_tick_mirror* m) {
    if (int rc = sdr_bank_tick_mirrored_begin(e, b, iq, n_samples, ring_offset, write_index, m)) return rc;
    return sdr_bank_tick_mirrored_end(e, b, m);
}

int sdr_tick_server_stats(sdr_engine* e, int64_t* out4) {
    if (!e || !out4) return sdr_fail(SDR_ERR_INVALID, "null engine or output");
    out4[0] = e->srv_running ? 1 : 0;
    out4[1] = e->srv ? e->srv->served_total : 0;
    out4[2] = e->srv ? e->srv->starts : 0;
    out4[3] = e->srv && e->srv->disabled ? 1 : 0;
    return SDR_OK;
}

// Where the served requests' time went on the device, in microseconds summed over them (the doorman's wall-clock stamps):
// {the slab's shares in the ring (pulled since it was staged: what is left of that when the request arrives), channels released,
// every channel has answered (the host has the answers by then: the channels write them themselves), the request closed}.
int sdr_tick_server_phases(sdr_engine* e, double* out4) {
    if (!e || !out4) return sdr_fail(SDR_ERR_INVALID, "null engine or output");
    if (e->srv && e->srv_running) server_absorb_stamps(e->srv);
    for (int k = 0; k < 4; ++k) out4[k] = e->srv ? e->srv->phase_us[k] : 0.0;
    return SDR_OK;
}

// ... and channel 0's own tick (lane 0 of its first part), the same way: {release seen, samples visible (L2 invalidated),
// correlated, sums exchanged, loops updated, answer written}.
int sdr_tick_server_tracker_phases(sdr_engine* e, double* out6) {
    if (!e || !out6) return sdr_fail(SDR_ERR_INVALID, "null engine or output");
    if (e->srv && e->srv_running) server_absorb_stamps(e->srv);
    for (int k = 0; k < 6; ++k) out6[k] = e->srv ? e->srv->tracker_us[k] : 0.0;
#ifdef SDR_SRV_TRACE
    if (e->srv && e->srv->served_total)
        fprintf(stderr, "tick server: the doorman sees 1 / half / all but one / all answers %.2f / %.2f / %.2f / %.2f us after the release\n",
                e->srv->seen_us[0] / e->srv->served_total, e->srv->seen_us[1] / e->srv->served_total, e->srv->seen_us[2] / e->srv->served_total,
                e->srv->seen_us[3] / e->srv->served_total);
#endif
#ifdef SDR_SRV_TRACE
    if (e->srv && e->srv->dev.ptr) {
        TickServerDev d;
        if (hipMemcpy(&d, e->srv->dev.ptr, sizeof(d), hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "tick server: per channel, us after the request was seen: release seen / answered  [xcc:hw_id of the recording part]\n");
            fprintf(stderr, "  doormen at");
            for (int g = 0; g < 8; ++g) fprintf(stderr, " [%u:%04x]", d.door_where[g] >> 16, d.door_where[g] & 0xffff);
            fprintf(stderr, "\n");
            for (int c = 0; c < 64; ++c)
                if (d.ch_n[c])
                    fprintf(stderr, "  ch %2d: %6.2f %6.2f  [%u:%04x]\n", c, (double)d.ch_gate[c] / d.ch_n[c] * 0.01, (double)d.ch_done[c] / d.ch_n[c] * 0.01,
                            d.ch_where[c] >> 16, d.ch_where[c] & 0xffff);
        }
    }
    if (e->srv) fprintf(stderr, "tick server: channel 0 release fence + count: %.2f us (mean of %llu)\n", e->srv->fence_add_us / (double)(e->srv->prev_t5 ? e->srv->prev_t5 : 1), e->srv->prev_t5);
#endif
    return SDR_OK;
}

int sdr_iq_upload_begin(sdr_engine* e, const void* iq, int64_t n_samples, int64_t ring_offset) {
    if (!e) return sdr_fail(SDR_ERR_INVALID, "null engine");
    return sdr_iq_upload_async(e, iq, n_samples, ring_offset);
}

}  // extern "C"
