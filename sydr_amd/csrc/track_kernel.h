// On-device loop closure: persistent workgroups run
// correlate -> discriminators -> loop filters -> NCO update for n_epochs without leaving the
// GPU.  A channel is served by ONE workgroup (512 threads; or 256 threads capped at
// 168 registers so that three share a CU when there are more channels than CUs) or by a CLUSTER of 2, 4 or 8
// workgroups (chosen so that the launch fills the GPU: 32 channels x 8 parts = 256 CUs): every epoch each part
// correlates its share of the samples, publishes its partial sums through global memory, collects its peers' and
// adds all of them in the same fixed order -- so every part holds bit-identical totals and runs the scalar loop
// update redundantly; there is no second exchange.  The PRN replica stays in LDS for the whole run; the loop
// arithmetic is fp64, spread over four waves by dependency (carrier loop / code loop / lock indicators + state
// machine + bit decisions / carrier phase over the epoch) and, inside each, over lanes for the divisions, roots
// and arctangents -- following the two reference plugins statement by statement:
//   kind 0  Borre  : channel_l1ca_borre.py:333-451  (DLL NNEML + Costas PLL, Borre filters, np.pi NCO)
//   kind 1  Kaplan : channel_l1ca_kaplan.py:342-619 (FLL-assisted 2nd-order PLL, lock-state machine,
//                    GPS-ICD pi in the NCO and the discriminators: SURVEY.md T3)
// built on sydr/dsp/tracking.py:120-186,246-279 and sydr/dsp/lockindicator.py:6-122, generalised by configuration
// only (taps, chips per epoch, epochs per symbol, epoch duration: BASELINE configs 4-5).
//
// This header is the device side: the tick server's shared structs and device functions, the loop update and the
// track_kernel template.  track.hip (the host side) and track_dense.hip (the dense form, a translation unit of its own)
// include it.
#pragma once
#include "correlator.h"
#include "correlator_chip.h"

#ifdef SDR_TRACE_TRACK
// Debug build only (tools/track_phases.py): per-phase clock totals of channel 0's epoch loop.
__device__ unsigned long long g_track_phase[64];   // [0,8) phases, [8,40) per-wave arrival (8 parts x 4 waves), [48,52) per-role, [62,64) clocks
extern "C" __attribute__((visibility("default"))) int sdr_debug_track_phases(unsigned long long* dst) {
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_track_phase), sizeof(g_track_phase));
}
#define TRACK_MARK(k)                                                     \
    do {                                                                  \
        if (tid == 0 && ch == 0 && part == 0) {                           \
            const unsigned long long now_ = wall_clock64();               \
            g_track_phase[k] += now_ - mark_;                             \
            mark_ = now_;                                                 \
        }                                                                 \
    } while (0)
#else
#define TRACK_MARK(k) ((void)0)
#endif

namespace {

using namespace sdr;

constexpr int kMaxParts = 8;

// ------------------------------------------------------------------------------------------------ the tick server
// The receiver's per-millisecond loop (receiver.py:120-131: addNewRFData(1 ms); run()) pays a kernel launch and a stream
// synchronisation per tick: ~13 of a tick's ~29 us in the library (tools/ubench_pingpong.hip: a round trip host -> resident
// workgroup -> host through page-locked words takes 1.8 us, an empty launch + synchronisation 12.5).  With
// sdr_set_option("tick_server", 1) the cluster form of the kernel stays RESIDENT between ticks, and eight more workgroups, the
// doormen, watch two words in page-locked memory.  A SLAB (sdr_iq_upload_begin) is announced at once: every doorman pulls
// an eighth of it out of the staging block into the ring and says so in device memory -- while the host is still on its way to
// the tick.  A REQUEST (sdr_bank_tick_mirrored) carries the ring's write index and the slab it needs; the first doorman waits
// for the eight shares and releases the channels, each through a word of its own; every channel whose next epoch is complete
// runs it exactly as a block launch would (same cluster, same order of additions: the bits of a plain tick) and ANSWERS THE
// HOST ITSELF: one wave writes state and record into page-locked memory and, behind a system-wide release, the request's
// number into the channel's done word; the host spins on those words.  The doorman only counts the answers (its clock bounds
// them) and stamps the request.
// Nothing waits without a bound: the doormen give up after `idle_ticks` without a request (the host starts a new server
// with the next tick), a tracker after twice that without a release, the doorman after `busy_ticks` without the channels'
// answers (fault), the exchange as ever after kSpinLimit polls; the host waits a bounded time for the done words and falls
// back to plain launches.  Every other call on the engine stops the server first (sdr_set_device).
constexpr unsigned kServerStop = 0xFFFFFFFFu;
constexpr int kGoStride = 32;      // unsigned words between two channels' release words: a 128-byte line each
// The request line: 64 bytes, 64-byte aligned, read by the doormen in ONE access (eight lanes x 8 bytes).  The host writes
// words 1-5, then word 7, then word 0 (both hold the same numbers); a reader takes the line when words 0 and 7 agree -- each
// 32-byte half of the access is then at least as new as its number, should the access ever be split.
enum { kReqSeqs = 0, kReqWriteIndex = 1, kReqSlabSrc16 = 2, kReqSlabN16 = 3, kReqSlabFirst16 = 4, kReqNeedPull = 5, kReqSeqsCopy = 7 };
struct TickServerHost {            // page-locked: the words the host and the doormen share
    // [0] / [7]: request number (low half: 1, 2, 3, ...; kServerStop = leave) and slab number (high half: 1, 2, 3, ...: "pull
    // this slab into the ring"); [1] the ring's write index after the slab; [2] where the slab lies in page-locked memory
    // (its address / 16: a staging half of the engine's or the caller's own block), [3] its granules, [4] its first ring granule; [5] the slab the request needs in the ring before the channels
    // are released (0: none)
    unsigned long long line[8];
    unsigned done_seq;             // doorman: the last request it has seen answered by every channel (stamps below are that request's)
    unsigned alive;                // doorman: 1 while the server runs
    unsigned fault;                // doorman: why it gave up (1 idle, 2 a channel never answered, 3 exchange fault)
    unsigned pad_;
    // doorman: wall-clock stamps (100 MHz) of the last request -- seen, slab in the ring, channels released, all channels
    // answered, stamps written (sdr_tick_server_phases: where a served tick's time goes on the device)
    unsigned long long stamps[6];
    unsigned long long tracker[12]; // ... and channel 0's own: release seen, samples visible, correlated, exchanged, updated, answered
};
struct TickServerDev {             // device memory: the words the doormen and the trackers share
    unsigned done_count;           // trackers: channels that have answered, all requests together (the doorman's watch on them)
    unsigned stop;                 // doorman: it has left (the helpers follow)
    unsigned pulled[8];            // doormen: the last slab whose share each has put into the ring
    long long write_index;
    int fault;                     // a cluster exchange timed out
    unsigned long long t[12];      // channel 0, part 0, lane 0: wall-clock stamps of its last tick (sdr_tick_server_phases); [8..11]: trace build
#ifdef SDR_SRV_TRACE
    unsigned long long seen_at;          // the doorman: when it saw the current request
    unsigned long long ch_gate[64], ch_done[64], ch_n[64];   // per channel, summed over requests: request seen -> release seen / answered (recording part)
    unsigned ch_where[64];               // ... and where that part runs (XCC_ID << 16 | HW_ID's CU bits)
    unsigned door_where[8];              // ... and the doormen
#endif
};
struct TickServer {
    TickServerHost* host;          // nullptr: not a server launch
    TickServerDev* dev;
    unsigned* go;                  // device [n_ch * kGoStride]: channel c's release word (the request its cluster may work on; kServerStop: leave)
    uint4* ring16;
    unsigned long long ring_n16;
    unsigned ring_flip;            // what a slab's dwords are xor-ed with on their way into the ring (ring_format.h ring_flip_mask)
    sdr_track_epoch* rec_out;      // device [n_ch]: where the roles write the epoch's record
    // page-locked, written by the channels themselves: the answer (state, record, 1 ran / 0 not ready / -1 stopped), then -- behind a
    // system-wide release -- the number of the request it answers
    int* h_ran;
    sdr_track_state* h_st;
    sdr_track_epoch* h_rec;
    unsigned* h_done;
    unsigned long long idle_ticks, busy_ticks;   // of wall_clock64() (100 MHz)
    // NOT the server's (host == nullptr): a plain launch whose results go straight into page-locked memory has every channel
    // raise done_words[its position in the list] = done_seq behind them -- the host reads the results when the words are
    // there instead of waiting for the stream's signal, which follows the kernel's last store by ~9 us (bank_collect)
    unsigned* done_words;
    unsigned done_seq;
    // Likewise a plain launch's (the one-launch receiver tick): its first kTickIngestGroups workgroups pull the tick's slab out
    // of page-locked memory (address / 16 = ingest_src16, ingest_n16 granules) into the ring (`ring16`, from ingest_first16) and
    // count themselves in at *ingest_count; the trackers stage their tables and parameters meanwhile and read their first
    // sample when the count has reached ingest_target.  ingest_n16 = 0: no slab with this launch.
    unsigned long long ingest_src16, ingest_n16, ingest_first16;
    unsigned* ingest_count;
    unsigned ingest_target;
};
// In front of the exchange lines (one-launch ticks): 64 ticket counters (a cluster of two parts or more means 64 channels at
// most), then the ingest workgroups' counter.
constexpr int kXchgHeadBytes = 512;
constexpr int kTickIngestGroups = 16;    // (a multiple of 8: the trackers' blockIdx % 8 -- their XCD -- is what it was without them)

// The doormen: kDoorGroups workgroups, a launch of their own beside the trackers' (the cluster of 32 channels x 8 parts fills
// the cooperative launch's 256 workgroups; a doorman needs a few registers and no LDS to speak of, and shares a compute unit
// with one of them).
// (eight waves, two per SIMD, few registers: it has to fit beside a tracker workgroup that holds 256 registers per lane on
// every SIMD of its compute unit -- sixteen waves did not.  A 50 KB slab is seven 16-byte loads per lane, four in flight.)
constexpr int kDoorThreads = 512;
// One workgroup reads the host's memory at a few GB/s (a 50 KB slab took it 19 us): kDoorGroups workgroups pull an equal share
// each.  All of them watch the host's words; the first is the doorman proper (requests are its business alone), the others
// leave when it does (or by their own, longer, clock).
constexpr int kDoorGroups = 8;
static_assert(kDoorGroups == 8, "TickServerDev::pulled has eight words");
__device__ __forceinline__ unsigned long long lane_u64(unsigned long long x, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)x, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(x >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __attribute__((unused)) void tick_server_doorman(const TickServer& s, const int n_ch, const int tid, unsigned* sh_words,
                                                            unsigned long long* sh_q, const int group) {
    unsigned served = 0, pulled = 0, requests = 0;
    unsigned quiet = 0;                // long sleeps before the next look at the host's line (see below)
    unsigned long long t_last = wall_clock64();
    unsigned why = 0;
    const bool helper = group != 0;
    if (tid == 0 && !helper) __hip_atomic_store(&s.host->alive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#ifdef SDR_SRV_TRACE
    if (tid == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        s.dev->door_where[group] = (xcc << 16) | (hw & 0xffff);
    }
#endif
    for (;;) {
        if (tid < 64) {
            // A compute unit returns its waves' loads IN ORDER: while a doorman's look at the host's line is on its way over the
            // link (~1.5 us), every load of the tracker workgroup it shares the compute unit with waits behind it -- measured
            // per channel (-DSDR_SRV_TRACE): the channels with a part beside a doorman answered 5-7 us after the others, and the
            // tick is as long as its last channel.  So the doormen keep QUIET while the channels work: a helper for ~12 us after
            // its share of a slab (the request it came with takes longer than that), the doorman proper between the release
            // and the time the first answers are due (its count of the answers is not on the host's path any more).
            for (unsigned k = 0; k < quiet; ++k) __builtin_amdgcn_s_sleep(127);      // (8128 clocks each)
            quiet = 0;
            // (one look per turn of the loop, a short sleep between turns: eight workgroups reading the host's line back to back
            // slowed the trackers' own traffic -- the channels' answers took 14.9 instead of 12.0 us.  The whole request comes
            // with the look: eight lanes, 8 bytes each, one access over the link -- no second round trip for its words)
            unsigned long long w = 0;
            if (tid < 8) w = __hip_atomic_load(&s.host->line[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            const unsigned long long w0 = lane_u64(w, kReqSeqs), w7 = lane_u64(w, kReqSeqsCopy);
            const unsigned long long q_wi = lane_u64(w, kReqWriteIndex), q_src = lane_u64(w, kReqSlabSrc16), q_n = lane_u64(w, kReqSlabN16),
                                     q_first = lane_u64(w, kReqSlabFirst16), q_need = lane_u64(w, kReqNeedPull);
            if (tid == 0) {
                const bool whole = w0 == w7;
                const unsigned seq = whole ? (unsigned)w0 : served, pseq = whole ? (unsigned)(w0 >> 32) : pulled;
                unsigned act = 0;                            // 1: a slab to pull, 2: a request (doorman proper), 4: leave
                if ((unsigned)w0 == kServerStop || (unsigned)w7 == kServerStop) {
                    act = 4;
                } else {
                    if (pseq != pulled) act |= 1;
                    if (!helper && seq != served) act |= 2;
                }
                if (!act && wall_clock64() - t_last > (helper ? 2 * s.idle_ticks : s.idle_ticks)) act = 4, sh_words[1] = 1;
                if (helper && !act && __hip_atomic_load(&s.dev->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) act = 4;   // (the doorman has left)
                if (act & 3) sh_q[0] = q_wi, sh_q[1] = q_n, sh_q[2] = q_src, sh_q[3] = q_first, sh_words[6] = (unsigned)q_need;
                sh_words[0] = act, sh_words[4] = seq, sh_words[5] = pseq;
            }
        }
        __syncthreads();
        const unsigned act = sh_words[0], seq = sh_words[4], pseq = sh_words[5], need_pull = sh_words[6];
        const long long wi = (long long)sh_q[0];
        const unsigned long long n16 = sh_q[1], src16 = sh_q[2], first16 = sh_q[3];
        __syncthreads();
        if (!act) {
            __builtin_amdgcn_s_sleep(4);
            continue;
        }
        if (act & 4) {
            why = sh_words[1];
            break;
        }
        unsigned long long stamp[6];
        stamp[0] = wall_clock64();
        if (act & 1) {
            // (the staging block is the host's memory, written since this compute unit last read it: nothing of it may come out
            // of a cache -- one invalidation by the first wave, the barrier hands it on)
            if (tid < 64) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            __syncthreads();
            // this workgroup's share of the slab: granules [lo, hi)
            const unsigned long long lo = n16 * (unsigned long long)group / kDoorGroups, hi = n16 * (unsigned long long)(group + 1) / kDoorGroups;
            const uint4* const src = reinterpret_cast<const uint4*>(static_cast<uintptr_t>(src16) << 4);   // (an address in the host's memory / 16)
            for (unsigned long long i0 = lo + tid; i0 < hi; i0 += 4 * kDoorThreads) {     // four loads per lane in flight, then their stores
                uint4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (i0 + (unsigned long long)k * kDoorThreads < hi) v[k] = src[i0 + (unsigned long long)k * kDoorThreads];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned long long i = i0 + (unsigned long long)k * kDoorThreads;
                    if (i < hi) {
                        unsigned long long d = first16 + i;
                        if (d >= s.ring_n16) d -= s.ring_n16;
                        uint4 o = v[k];
                        o.x ^= s.ring_flip, o.y ^= s.ring_flip, o.z ^= s.ring_flip, o.w ^= s.ring_flip;
                        s.ring16[d] = o;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // every wave: its stores have left (the barrier orders them ...)
            __syncthreads();                                          // ... before lane 0's device-wide release below)
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __hip_atomic_store(&s.dev->pulled[group], pseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            pulled = pseq;
            t_last = wall_clock64();
            if (helper) quiet = 3;
        }
        if (!(act & 2)) continue;
        // ---- a request (the doorman proper)
        ++requests;
        if (tid == 0) {
            s.dev->write_index = wi;
#ifdef SDR_SRV_TRACE
            s.dev->seen_at = stamp[0];
#endif
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            // the eight shares of the slab it needs (bounded: a helper that never shows up is a fault like a channel that never answers)
            unsigned ok_pull = 1;
            if (need_pull) {
                const unsigned long long t0 = wall_clock64();
                for (int g = 0; g < kDoorGroups && ok_pull; ++g) {
                    while ((int)(__hip_atomic_load(&s.dev->pulled[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - need_pull) < 0) {
                        if (wall_clock64() - t0 > s.busy_ticks) {
                            ok_pull = 0;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
            }
            sh_words[3] = ok_pull;
            stamp[1] = wall_clock64();
        }
        __syncthreads();
        // the release: every channel's word (n_ch <= 64: one store of the first wave)
        if (sh_words[3] && tid < n_ch) __hip_atomic_store(&s.go[(size_t)tid * kGoStride], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) {
            stamp[2] = wall_clock64();
            const unsigned target = requests * (unsigned)n_ch;
            const unsigned long long t0 = wall_clock64();
            unsigned ok = 1;
            __builtin_amdgcn_s_sleep(127);       // (quiet while the channels work: see the top of the loop)
            __builtin_amdgcn_s_sleep(127);
#ifdef SDR_SRV_TRACE
            unsigned long long seen[4] = {0, 0, 0, 0};      // first sight of 1, n/2, n - 1, n answers
#endif
            for (;;) {
                const unsigned c = __hip_atomic_load(&s.dev->done_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef SDR_SRV_TRACE
                const unsigned have = c - (target - (unsigned)n_ch);
                const unsigned long long now = wall_clock64();
                if (have >= 1 && !seen[0]) seen[0] = now;
                if (have >= (unsigned)n_ch / 2 && !seen[1]) seen[1] = now;
                if (have >= (unsigned)n_ch - 1 && !seen[2]) seen[2] = now;
                if (have >= (unsigned)n_ch && !seen[3]) seen[3] = now;
#endif
                if (c == target) break;
                if (wall_clock64() - t0 > s.busy_ticks) {
                    ok = 0;
                    break;
                }
                __builtin_amdgcn_s_sleep(32);
            }
#ifdef SDR_SRV_TRACE
            for (int k = 0; k < 4; ++k) s.dev->t[8 + k] = seen[k] - t0;
#endif
            sh_words[2] = ok && sh_words[3];
            stamp[3] = wall_clock64();
            if (sh_words[2]) {
                // (the channels have answered the host themselves; what is left is the request's bookkeeping)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                stamp[4] = wall_clock64();
                for (int k = 0; k < 5; ++k) s.host->stamps[k] = stamp[k];
                for (int k = 0; k < 12; ++k) s.host->tracker[k] = s.dev->t[k];
                if (__hip_atomic_load(&s.dev->fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    __hip_atomic_store(&s.host->fault, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
                __hip_atomic_store(&s.host->done_seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        __syncthreads();
        if (!sh_words[2]) {
            why = 2;
            break;
        }
        served = seq;
        t_last = wall_clock64();
    }
    if (!helper) {
        // the channels (their release words) and the helpers (the stop word) follow; then the host is told
        if (tid < n_ch) __hip_atomic_store(&s.go[(size_t)tid * kGoStride], kServerStop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) {
            __hip_atomic_store(&s.dev->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (why) __hip_atomic_store(&s.host->fault, why, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(&s.host->alive, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// Exchange line of one part and parity: 4*NT tagged half-values padded to whole 128-byte lines (16 words for E/P/L,
// 32 for five taps).
constexpr int xchg_words(int nt) { return 4 * nt <= 16 ? 16 : 32; }
constexpr int kXchgWordsMax = 32;
constexpr long kSpinLimit = 1L << 20;      // peer polls before a part gives up (about a second): never hang the GPU
#ifndef SDR_XCHG_SLEEP
#define SDR_XCHG_SLEEP 16
#endif
constexpr int kXchgSleep = SDR_XCHG_SLEEP;             // x 64 cycles between publishing a part's sums and the first look at the peers'

constexpr double kGpsPi = 3.1415926535898;  // sydr/utils/constants.py:4
constexpr double kGpsTwoPi = kGpsPi * 2.0;
constexpr double kGpsHalfPi = kGpsPi / 2.0;
constexpr double kDefaultEpochChips = 1023.0;  // GPS_L1CA_CODE_SIZE_BITS (kaplan:529-532)
constexpr int kDefaultEpochsPerBit = 20;       // LNAV_MS_PER_BIT
constexpr double kDefaultEpochSeconds = 1e-3;  // the dt the Kaplan plugin hard-codes (kaplan:417,425,443,494)
constexpr double kW0Bw1 = 0.25, kW0Bw2 = 0.53, kW0A2 = 1.414;

enum { FLAG_CODE_LOCK = 1, FLAG_BIT_SYNC = 2 };
enum { LOCK_PULL_IN = 1, LOCK_WIDE = 2, LOCK_NARROW = 3 };

// Python / NumPy float modulo (result takes the sign of the divisor).
__device__ __forceinline__ double py_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}
__device__ __forceinline__ double np_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }

// The discriminators and filters of sydr/dsp/tracking.py -- DLL NNEML (:120-129), Costas PLL (:133-142),
// FLL atan (:156-176), BorreLoopFilter (:180-186) -- are evaluated inside the kernel's loop update, their
// divisions / square roots / arctangents spread over lanes (see there).

// The lock role's share of the loop state, held in registers of its lane 0 for the whole run (19 LDS reads and as many
// writes per epoch otherwise -- and this role is the longest of the four: tools/track_phases.py).  Written back to
// the LDS copy of the state once, after the last epoch.
struct LockRegs {
    double fll_lock, pll_lock, cn0, ratio_acc, ipp, qpp, fll_bw, pll_bw, nav_sum;
    int accum, lock_state, time_in_state, spacing_sel, flags, code_counter, nav_count, bits_emitted, bits_run;
};
// The run's constants the update roles divide and scale with.  The forms with registers to spare keep them in registers
// (UpdateCtx); the dense form (three workgroups per compute unit, 168 registers) reads them from LDS when a role needs them.
struct UpdateConsts {
    double fs, chips, dt;
    double by_fs_b, by_fs_y, by_dt_b, by_dt_y, by_2pi_b, by_2pi_y;
    int epochs_per_bit, ok_bits;       // ok_bits: InvDen::ok of by_fs | by_dt << 1 | by_2pi << 2
};

struct alignas(16) EpochShared {  // (size a multiple of 16: the replica behind it is copied with 16-byte stores)
    EpochParams ep;
    double spacing[SDR_MAX_TAPS];
    double dphi;
    int epochs_done;
    int fault;                 // a peer part never showed up: leave the epoch loop (reported to the host)
    // what the update roles hand to each other (written before an epoch's first barrier, read after it)
    double corr[2 * SDR_MAX_TAPS];  // this epoch's correlator totals (one-workgroup kernels: for the roles on waves 1 and 2)
    double fll_bw, pll_bw;     // Kaplan bandwidths chosen by the lock-state machine, for the carrier loop
    int lock_state;            // lock state the NEXT epoch's discriminators run under
    int c_code_counter, l_code_counter, l_bits_run;  // private copies of the roles on waves 0 and 2
    int stop_code, stop_carrier;  // the next epoch would leave the staged replica / the ring, or the carrier NCO is not finite
    double smin, smax;         // extreme tap offsets over both tap sets (constant for the run)
    double l_ipp, l_qpp;       // the lock role's copy of the previous prompt (the carrier role owns st.i/q_prompt_prev)
    // quotients that only change with the configuration or the lock state, kept instead of re-divided every epoch
    // (same operands => same bits): atan(qP'/iP') of the previous epoch, the Kaplan natural frequencies for the
    // bandwidths they were computed from, the Borre filter ratios
    double at_prev, w0f, w0p, w0f_bw, w0p_bw, pll_r1, pll_r2, dll_r1, dll_r2;
    unsigned gate;             // (tick server) the release the workgroup's lane 0 saw at the top of the tick
    unsigned pad_sh_;          // (keeps the struct a multiple of 16 bytes)
    long long gate_wi;         // ... and the request's write index
    long long pad_sh2_;
    sdr_track_state st;        // the loop state; each update role owns a disjoint set of its fields
    sdr_loop_cfg cfg;
    // the dense form: what the other forms carry in registers across the whole epoch -- the lock role's state and the run's
    // constants.  At 168 registers per lane the compiler spilled them to scratch memory and the roles fetched them back one
    // dependent load at a time, on the epoch's critical path (76 scratch loads behind the reduction barrier, round 5).
    LockRegs lk;
    UpdateConsts uc;
    long long pad_dense_;
};
static_assert(sizeof(EpochShared) % 16 == 0, "the replica behind it is copied with 16-byte stores");

// a / b for a denominator that does not change during the run (fs, 2*pi, the epoch duration), given y = RN(1/b):
// two Newton corrections of the quotient with exact FMA residuals.  The second one rounds correctly (Markstein's
// theorem: y within half an ulp of 1/b and q within one ulp of a/b => RN(q + r*y) = RN(a/b), b's significand not
// all ones) -- the SAME bits as the reference's division, on a dependent chain of 5 operations instead of the ~12
// of v_div_scale / v_rcp / v_fma... / v_div_fmas / v_div_fixup.  tests/test_div_by_constant.py checks the identity
// on 10^8 operands per denominator.  ok == false (significand all ones, never the case for a sampling rate):
// plain division.
struct InvDen {
    double b, y;
    bool ok;
};
__device__ __forceinline__ InvDen inv_den(double b) {
    InvDen d;
    d.b = b;
    d.y = 1.0 / b;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(b);
    d.ok = (bits & 0xFFFFFFFFFFFFFull) != 0xFFFFFFFFFFFFFull && b == b && fabs(b) > 1e-290 && fabs(b) < 1e290;
    return d;
}
__device__ __forceinline__ double div_by(double a, const InvDen& d) {
    if (!d.ok) return a / d.b;
    const double q0 = a * d.y;
    const double r0 = __builtin_fma(-d.b, q0, a);
    const double q1 = __builtin_fma(r0, d.y, q0);
    const double r1 = __builtin_fma(-d.b, q1, a);
    return __builtin_fma(r1, d.y, q1);
}

__device__ __forceinline__ LockRegs lock_regs_from(const sdr_track_state& s) {
    LockRegs r;
    r.fll_lock = s.fll_lock, r.pll_lock = s.pll_lock, r.cn0 = s.cn0, r.ratio_acc = s.cn0_ratio_acc;
    r.ipp = s.i_prompt_prev, r.qpp = s.q_prompt_prev, r.fll_bw = s.fll_bw, r.pll_bw = s.pll_bw, r.nav_sum = s.nav_prompt_sum;
    r.accum = s.accum_counter, r.lock_state = s.lock_state, r.time_in_state = s.time_in_state;
    r.spacing_sel = s.spacing_sel, r.flags = s.track_flags, r.code_counter = s.code_counter;
    r.nav_count = s.nav_sum_counter, r.bits_emitted = s.nav_bits_emitted, r.bits_run = 0;
    return r;
}
__device__ __forceinline__ void lock_regs_store(const LockRegs& r, EpochShared* sh);

// What the update roles need besides the shared state: the run's constants and this epoch's inputs (all wave-uniform).
struct UpdateCtx {
    double fs, chips, dt;          // sampling rate, chips per epoch, epoch duration the Kaplan filters are scaled with
    int epochs_per_bit;
    InvDen by_fs, by_dt, by_2pi;   // 1/fs, 1/dt, 1/(GPS 2 pi)
    int64_t capacity;
    int lut_words;
    EpochParams ep;                // the epoch that has just been correlated
    double cur_fll_bw, cur_pll_bw; // the state machine's previous decision (captured at the top of the epoch)
    int cur_lock_state;
    int epoch, n_epochs, ch;
    bool writer;
    sdr_track_epoch* rec;          // this epoch's record (recording part only, trajectory requested) or nullptr
    int8_t* nav_bits;
    int max_bits;
};

__device__ __forceinline__ bool carrier_bad(double hz) { return !(hz == hz && fabs(hz) < 1e9); }

// The replica LUT and the ring bound what an epoch may touch; a loop that has run away (loss of lock) stops
// instead of reading out of range.  Checked by the role that produces the values, for the epoch it announces.
__device__ __forceinline__ bool code_out_of_range(const EpochShared* sh, int64_t capacity, int lut_words, int64_t start,
                                                  int n, double rem_code, double code_step) {
    const double lo = ceil(rem_code + sh->smin);
    const double hi = ceil(code_step * (double)n + rem_code + sh->smax);
    return !(n > 0 && (int64_t)n <= capacity && code_step > 0.0 && lo >= -(double)SDR_LUT_PAD &&
             hi <= (double)(lut_words - SDR_LUT_PAD - 2) && start >= 0);
}

// Loop update.  The reference's per-epoch sequence is scalar arithmetic whose cost is instruction LATENCY
// (~15 fp64 divisions, two square roots, two arctangents, a float modulo, ~1250 instructions when one lane
// does it all).  It splits into four chains that only meet through the previous epoch's results:
//   wave 0  carrier loop : FLL/PLL discriminators, carrier filter, carrier frequency        (kaplan:405-447,506-534)
//   wave 1  code loop    : DLL discriminator, code filter, code NCO, next epoch length      (kaplan:451-461,506-534)
//   wave 2  lock role    : lock indicators, C/N0, lock-state machine, flags, bit sync, nav bits (kaplan:465-619)
//   wave 3  carrier phase: remCarrier advanced over the epoch, modulo 2 pi -- depends on nothing this epoch
//                          measured (kaplan:523-524, borre:364-365)
// Each wave evaluates its divisions / roots / arctangents side by side, one per lane (same IEEE operations on
// the same operands as the reference's statements: bit-identical), then lane 0 runs the rest of its chain and
// publishes its share of the next epoch's parameters.  corr[2*NT]: this epoch's correlator totals.
template <int NT, bool DENSE = false>
__device__ __forceinline__ void loop_update(EpochShared* sh, const UpdateCtx& u, const double* corr, int role, int rlane,
                                            LockRegs& lk_regs) {
    constexpr int kTaps = NT;
    constexpr int kPrompt = NT / 2;                       // centre tap; its neighbours are early and late
    sdr_track_state& st = sh->st;
    const sdr_loop_cfg& cfg = sh->cfg;
    const EpochParams& ep = u.ep;
    double fs = u.fs, kChips = u.chips, kDt = u.dt;
    int kMsPerBit = u.epochs_per_bit;
    InvDen by_fs = u.by_fs, by_dt = u.by_dt, by_2pi = u.by_2pi;
    LockRegs lk_local;
    if constexpr (DENSE) {
        // (through a pointer the compiler cannot see through: read HERE, every epoch -- hoisted out of the epoch loop they
        // would be registers again, and spilled again)
        const UpdateConsts* c = &sh->uc;
        asm volatile("" : "+v"(c));
        fs = c->fs, kChips = c->chips, kDt = c->dt, kMsPerBit = c->epochs_per_bit;
        const int okb = c->ok_bits;
        by_fs = InvDen{c->by_fs_b, c->by_fs_y, (okb & 1) != 0};
        by_dt = InvDen{c->by_dt_b, c->by_dt_y, (okb & 2) != 0};
        by_2pi = InvDen{c->by_2pi_b, c->by_2pi_y, (okb & 4) != 0};
        if (role == 2 && rlane == 0) lk_local = sh->lk;
    }
    LockRegs& lk = DENSE ? lk_local : lk_regs;
    const double ie = corr[2 * kPrompt - 2], qe = corr[2 * kPrompt - 1], ip = corr[2 * kPrompt], qp = corr[2 * kPrompt + 1],
                 il = corr[2 * kPrompt + 2], ql = corr[2 * kPrompt + 3];
    const int n = ep.n;
    const bool kaplan = cfg.loop_kind != 0;
    sdr_track_epoch* rec = u.rec;
    if (role == 0) {
        // ------------------------------------------------------------------ carrier loop
        // (every lane evaluates the same chain on the same wave-uniform operands: no lane specialisation, no
        // v_readlane -- a lone wave pays per instruction, not per lane)
        const double at_now = atan(qp / ip);                      // atan(qP/iP): Costas PLL, FLL (tracking.py:133-176)
        const double at_prev = sh->at_prev;                       // atan(qP'/iP') as the previous epoch computed it
        double fll_err = at_now - at_prev;
        if (fll_err != fll_err) fll_err = 0.0;
        if (fll_err >= kGpsHalfPi) fll_err = fll_err - kGpsPi;
        else if (fll_err <= -kGpsHalfPi) fll_err = fll_err + kGpsPi;
        const double costas = div_by(at_now, by_2pi);                          // atan/2pi (pll_costas)
        const double fll_full = div_by(div_by(fll_err, by_dt), by_2pi);       // (err/dt)/2pi (fll_atan)
        double w0f = sh->w0f, w0p = sh->w0p;
        if (kaplan && (sh->w0f_bw != u.cur_fll_bw || sh->w0p_bw != u.cur_pll_bw)) {   // (the lock state changed the bandwidths)
            w0f = u.cur_fll_bw / kW0Bw1;
            w0p = u.cur_pll_bw / kW0Bw2;
            if (rlane == 0) {
                sh->w0f = w0f, sh->w0p = w0p;
                sh->w0f_bw = u.cur_fll_bw, sh->w0p_bw = u.cur_pll_bw;
            }
        }
        const double pll_r1 = sh->pll_r1, pll_r2 = sh->pll_r2;  // Borre PLL filter ratios tau2/tau1, pdi/tau1 (tracking.py:180-186)
        __builtin_amdgcn_wave_barrier();  // (every lane has read the previous prompt before lane 0 replaces it)
        if (rlane == 0) {
            double c_pll_mem = st.pll_mem;
            const int c_code_counter = sh->c_code_counter;
            double carrier_hz = ep.carrier_hz;
            double rec_pll, rec_fll, rec_carrier_err;
            if (!kaplan) {  // Borre: channel_l1ca_borre.py:364-429
                const double phase_err = costas;
                double nco_carrier = pll_r1 * (phase_err - c_pll_mem);
                nco_carrier += pll_r2 * phase_err;
                c_pll_mem = phase_err;
                carrier_hz += nco_carrier;
                rec_pll = nco_carrier, rec_fll = 0.0, rec_carrier_err = phase_err;
            } else {        // Kaplan: runDiscriminators / runCarrierFrequencyFilter / postTrackingUpdate
                double fll_d = 0.0, pll_d = 0.0;
                if (u.cur_lock_state == LOCK_PULL_IN) {
                    if (c_code_counter > 1) fll_d = fll_full;
                } else {
                    fll_d = fll_full;
                    pll_d = costas;
                }
                const double upd = (pll_d * (w0p * w0p) + fll_d * w0f) * kDt;  // FLLassistedPLL_2ndOrder (tracking.py:246-279)
                double carrier_err = upd + c_pll_mem;
                c_pll_mem = upd;
                carrier_err += pll_d * kW0A2 * w0p;
                carrier_hz += carrier_err;
                rec_pll = pll_d, rec_fll = fll_d, rec_carrier_err = carrier_err;
            }
            st.pll_mem = c_pll_mem;
            st.i_prompt_prev = ip;
            st.q_prompt_prev = qp;
            sh->at_prev = at_now;
            sh->c_code_counter = c_code_counter + 1;
            sh->ep.carrier_hz = carrier_hz;
            sh->stop_carrier = carrier_bad(carrier_hz) ? 1 : 0;
            sh->dphi = div_by((carrier_hz * 2.0) * M_PI, by_fs);  // carrier_step(): tracking.py:102 uses np.pi
            if (rec) {
                rec->carrier_hz_in = ep.carrier_hz;
                rec->rem_carrier_in = ep.rem_carrier;
                rec->pll = rec_pll;
                rec->fll = rec_fll;
                rec->carrier_err = rec_carrier_err;
                rec->carrier_hz = carrier_hz;
            }
        }
    } else if (role == 1) {
        // ------------------------------------------------------------------ code loop
        const double env_e = sqrt(ie * ie + qe * qe), env_l = sqrt(il * il + ql * ql);  // DLL NNEML envelopes (tracking.py:120-129)
        const double dll_nn = (env_e - env_l) / (env_e + env_l);
        const double dll_r1 = sh->dll_r1, dll_r2 = sh->dll_r2;   // BorreLoopFilter ratios tau2/tau1, pdi/tau1 (tracking.py:180-186)
        if (rlane == 0) {
            const double dll_d = dll_nn;
            double code_err = dll_r1 * (dll_d - st.dll_mem);
            code_err += dll_r2 * dll_d;
            st.dll_mem = dll_d;
            st.code_counter += 1;
            const double k_code_hz = st.code_hz - code_err;
            st.code_hz = k_code_hz;
            double rem_code = ep.rem_code;
            rem_code += (double)n * ep.code_step - kChips;
            const double code_step = div_by(k_code_hz, by_fs);
            const int64_t next_start = ep.start_sample + n;
            const int next_n = (int)ceil((kChips - rem_code) / code_step);
            sh->stop_code = code_out_of_range(sh, u.capacity, u.lut_words, next_start, next_n, rem_code, code_step) ? 1 : 0;
            sh->ep.start_sample = next_start;
            sh->ep.n = next_n;
            sh->ep.rem_code = rem_code;
            sh->ep.code_step = code_step;
            sh->epochs_done = u.epoch + 1;
            if (rec) {
                rec->start_sample = ep.start_sample;
                rec->n_samples = n;
                rec->rem_code_in = ep.rem_code;
                rec->code_step_in = ep.code_step;
                for (int k = 0; k < 2 * SDR_MAX_TAPS; ++k) rec->corr[k] = k < 2 * kTaps ? corr[k < 2 * kTaps ? k : 0] : 0.0;
                // Kaplan records the discriminator and the filter output; Borre the NCO command and the error
                rec->dll = kaplan ? dll_d : code_err;
                rec->code_err = kaplan ? code_err : dll_d;
                rec->code_hz = k_code_hz;
            }
        }
    } else if (role == 2) {
        // ------------------------------------------------------------------ lock indicators, state machine, bits
        const double pw = ip * ip + qp * qp;
        double num = 0.0, den = 1.0;
        switch (rlane) {
            case 0: {                                             // FLL lock (lockindicator.py:6-18)
                const double l_ipp = lk.ipp, l_qpp = lk.qpp;
                double v = ip * l_ipp - qp * l_qpp;
                v *= np_sign(ip * l_ipp + qp * l_qpp);
                num = v, den = pw;
                break;
            }
            case 1: num = ip * ip - qp * qp, den = pw; break;     // PLL lock (:22-36)
            case 2: {                                             // C/N0 (Beaulieu) ratio term (kaplan:488)
                const double d = fabs(ip) - fabs(qp);
                num = pw, den = d * d;
                break;
            }
            default: break;
        }
        const double quot = num / den;
        const double fll_lock_v = lane_value(quot, 0), pll_lock_v = lane_value(quot, 1), cn0_term = lane_value(quot, 2);
        if (rlane == 0) {
            double l_fll_lock = lk.fll_lock, l_pll_lock = lk.pll_lock, l_cn0 = lk.cn0, l_ratio_acc = lk.ratio_acc;
            double l_ipp = lk.ipp, l_qpp = lk.qpp, l_fll_bw = lk.fll_bw, l_pll_bw = lk.pll_bw, l_nav_sum = lk.nav_sum;
            int l_accum = lk.accum, l_lock_state = lk.lock_state, l_time_in_state = lk.time_in_state;
            int l_spacing_sel = lk.spacing_sel, l_flags = lk.flags, l_code_counter = lk.code_counter;
            int l_nav_count = lk.nav_count, l_bits_emitted = lk.bits_emitted, l_bits_run = lk.bits_run;
            int nav_bit = -1;
            if (!kaplan) {
                // Borre bit sync: first prompt sign flip after MIN_CONVERGENCE_TIME = 100 epochs (borre:384-391)
                if (!(l_flags & FLAG_BIT_SYNC) && (l_flags & FLAG_CODE_LOCK) && l_code_counter > 100 &&
                    np_sign(l_ipp) != np_sign(ip))
                    l_flags |= FLAG_BIT_SYNC;
                l_flags |= FLAG_CODE_LOCK;
                l_ipp = ip;
                l_qpp = qp;
                l_code_counter += 1;
            } else {
                // runCorrelators bookkeeping (kaplan:392-399)
                if (l_accum == kMsPerBit) l_accum = 0;
                l_accum += 1;
                // runLoopIndicators (:465-502)
                if (l_code_counter != 0) {
                    const double v = fabs(fll_lock_v);
                    l_fll_lock = (1.0 - 0.005) * l_fll_lock + 0.005 * v;
                    if (l_lock_state > LOCK_PULL_IN) l_pll_lock = (1.0 - 0.005) * l_pll_lock + 0.005 * pll_lock_v;
                    l_ratio_acc += cn0_term;
                    if (l_accum == kMsPerBit) {
                        const double lam = 1.0 / (l_ratio_acc / (double)l_accum);
                        const double c = lam * (1.0 / ((double)l_accum * kDt));
                        l_cn0 = (1.0 - 0.1) * l_cn0 + 0.1 * c;
                        l_ratio_acc = 0.0;
                    }
                }
                l_code_counter += 1;
                // trackingStateUpdate (:538-619)
                if (l_lock_state != LOCK_PULL_IN && l_cn0 > cfg.dll_threshold && !(l_flags & FLAG_CODE_LOCK))
                    l_flags |= FLAG_CODE_LOCK;
                else if (l_cn0 < cfg.dll_threshold && (l_flags & FLAG_CODE_LOCK))
                    l_flags ^= FLAG_CODE_LOCK;
                if ((l_flags & FLAG_CODE_LOCK) && !(l_flags & FLAG_BIT_SYNC)) {
                    if (np_sign(l_ipp) != np_sign(ip)) {
                        l_flags |= FLAG_BIT_SYNC;
                        l_accum = 1;
                        l_ratio_acc = 0.0;
                    }
                }
                l_ipp = ip;
                l_qpp = qp;
                if (l_lock_state != LOCK_NARROW && l_fll_lock >= cfg.fll_thr_narrow && l_pll_lock >= cfg.pll_thr_narrow) {
                    l_lock_state = LOCK_NARROW;
                    l_fll_bw = cfg.fll_bw_narrow;
                    l_pll_bw = cfg.pll_bw_narrow;
                    l_spacing_sel = 1;
                    l_time_in_state = 0;
                } else if (l_lock_state != LOCK_WIDE && l_fll_lock >= cfg.fll_thr_wide && l_fll_lock < cfg.fll_thr_narrow) {
                    l_lock_state = LOCK_WIDE;
                    l_fll_bw = cfg.fll_bw_wide;
                    l_pll_bw = cfg.pll_bw_wide;
                    l_spacing_sel = 0;
                    l_time_in_state = 0;
                } else if (l_lock_state != LOCK_PULL_IN && l_fll_lock <= cfg.fll_thr_wide) {
                    l_lock_state = LOCK_PULL_IN;
                    l_fll_bw = cfg.fll_bw_pullin;
                    l_pll_bw = 0.0;
                    l_spacing_sel = 0;
                    l_time_in_state = 0;
                } else {
                    l_time_in_state += 1;
                }
            }
            // decodeBit (kaplan:728-754, borre:470-491): 20 prompts after bit sync -> one bit (Prompt2Bit)
            if (!(l_flags & FLAG_BIT_SYNC)) {
                l_nav_sum = 0.0;
                l_nav_count = 0;
            } else {
                l_nav_sum += ip;
                l_nav_count += 1;
                if (l_nav_count == kMsPerBit) {
                    nav_bit = l_nav_sum > 0.0 ? 1 : 0;
                    if (u.writer && u.nav_bits && l_bits_run < u.max_bits) u.nav_bits[(size_t)u.ch * u.max_bits + l_bits_run] = (int8_t)nav_bit;
                    l_bits_run += 1;
                    l_bits_emitted += 1;
                    l_nav_sum = 0.0;
                    l_nav_count = 0;
                }
            }
            // hand-over to the other roles / the next epoch: only what changed (taps and bandwidths move with the lock state)
            if (l_spacing_sel != lk.spacing_sel) {
                const double* sp = l_spacing_sel ? cfg.spacing_narrow : cfg.spacing_wide;
                for (int t = 0; t < kTaps; ++t) sh->spacing[t] = sp[t];
            }
            if (l_lock_state != lk.lock_state || l_fll_bw != lk.fll_bw || l_pll_bw != lk.pll_bw) {
                sh->fll_bw = l_fll_bw;
                sh->pll_bw = l_pll_bw;
                sh->lock_state = l_lock_state;
            }
            lk.fll_lock = l_fll_lock, lk.pll_lock = l_pll_lock, lk.cn0 = l_cn0, lk.ratio_acc = l_ratio_acc;
            lk.ipp = l_ipp, lk.qpp = l_qpp, lk.fll_bw = l_fll_bw, lk.pll_bw = l_pll_bw, lk.nav_sum = l_nav_sum;
            lk.accum = l_accum, lk.lock_state = l_lock_state, lk.time_in_state = l_time_in_state;
            lk.spacing_sel = l_spacing_sel, lk.flags = l_flags, lk.code_counter = l_code_counter;
            lk.nav_count = l_nav_count, lk.bits_emitted = l_bits_emitted, lk.bits_run = l_bits_run;
            if constexpr (DENSE) sh->lk = lk;
            if (rec) {
                rec->cn0 = kaplan ? l_cn0 : 0.0;
                rec->pll_lock = kaplan ? l_pll_lock : 0.0;
                rec->fll_lock = kaplan ? l_fll_lock : 0.0;
                rec->lock_state = l_lock_state;
                rec->track_flags = l_flags;
                rec->nav_bit = nav_bit;
            }
        }
    } else if (role == 3 && rlane == 0) {
        // ------------------------------------------------------------------ carrier phase over the epoch
        // remCarrier -= f * 2 pi * n / fs; remCarrier %= 2 pi -- Kaplan with the GPS-ICD pi (kaplan:523-524), Borre with
        // np.pi (borre:364-365): SURVEY.md T3.  Needs nothing this epoch measured, so it is off the carrier role's chain.
        const double adv = (kaplan ? ep.carrier_hz * kGpsTwoPi * (double)n : ep.carrier_hz * 2.0 * M_PI * (double)n) / fs;
        double rem_carrier = ep.rem_carrier;
        rem_carrier -= adv;
        sh->ep.rem_carrier = py_mod(rem_carrier, kaplan ? kGpsTwoPi : 2.0 * M_PI);
    }
}

__device__ __forceinline__ void lock_regs_store(const LockRegs& r, EpochShared* sh) {
    sdr_track_state& st = sh->st;
    st.fll_lock = r.fll_lock, st.pll_lock = r.pll_lock, st.cn0 = r.cn0, st.cn0_ratio_acc = r.ratio_acc;
    st.fll_bw = r.fll_bw, st.pll_bw = r.pll_bw, st.nav_prompt_sum = r.nav_sum;
    st.accum_counter = r.accum, st.lock_state = r.lock_state, st.time_in_state = r.time_in_state;
    st.spacing_sel = r.spacing_sel, st.track_flags = r.flags;
    st.nav_sum_counter = r.nav_count, st.nav_bits_emitted = r.bits_emitted;
    sh->l_bits_run = r.bits_run;
}

// Wave-uniform copy of the epoch parameters in LDS.  What comes out of LDS is the same in every lane, but only
// readfirstlane tells the compiler so: as scalars the epoch parameters (and everything derived from them: group
// counts, ring positions, linspace constants) live in SGPRs and are computed on the scalar unit -- ~100 VGPRs per lane.
__device__ __forceinline__ EpochParams uniform_params(const EpochParams& v) {
    EpochParams ep;
    ep.start_sample = ((int64_t)__builtin_amdgcn_readfirstlane((int)(v.start_sample >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)v.start_sample);
    ep.n = __builtin_amdgcn_readfirstlane(v.n);
    ep.carrier_hz = uniform(v.carrier_hz);
    ep.rem_carrier = uniform(v.rem_carrier);
    ep.rem_code = uniform(v.rem_code);
    ep.code_step = uniform(v.code_step);
    return ep;
}

// LDS layout in doubles: [0, 256) workgroup reduction scratch, [256, 640) three role waves x 256 words of exchange staging
constexpr int kRedDoubles = 640;
constexpr int kXchgStageWords = 256;   // per role wave: up to 4 wave-wide loads of 64 words

// WAVES: resident waves per SIMD the register allocation has to leave room for (2 = two 256-thread
// workgroups can share a CU, at the price of a few spills).
// states / cfgs are indexed through ch_map when it is given (the device-resident channel bank: the launch serves
// the listed channels of a larger array); everything this launch produces (trajectory, bits, epochs_done, states_copy)
// is indexed by the position in the list.  Any of these outputs, ch_map and the fault word may live in page-locked
// host memory (a receiver tick reads its few KB of results without a single copy command).
// THREADS == 256 && WAVES == 1 is the CLUSTER form (parts >= 2 workgroups per channel, cooperative launch).
// A ONE-EPOCH step of that form (a receiver tick) needs no cooperative launch when it is cut at the exchange: phase 1 =
// the cluster's workgroups correlate and publish their sums, then end; phase 2 = one workgroup per channel collects the
// parts' sums (same order, same bits as the cooperative kernel) and runs the loop update.  Nobody waits for a peer inside
// a kernel, so two plain launches do (phase = 0: the whole epoch loop in one launch).  tag_base: added to the exchange
// words' epoch tag, so that lines left by earlier launches cannot validate (the phases do not zero the lines).
template <int FMT, int THREADS, int WAVES, int NT>
__global__ __launch_bounds__(THREADS, WAVES) void track_kernel(const void* __restrict__ ring, int64_t capacity,
                                                        sdr_track_state* __restrict__ states,
                                                        sdr_track_state* __restrict__ states_copy,
                                                        const int32_t* __restrict__ ch_map,
                                                        const sdr_loop_cfg* __restrict__ cfgs, int cfg_stride,
                                                        int n_epochs, sdr_track_epoch* __restrict__ traj,
                                                        int keep_traj, int8_t* __restrict__ nav_bits, int max_bits,
                                                        int32_t* __restrict__ n_bits,
                                                        int32_t* __restrict__ epochs_done_out,
                                                        const uint32_t* __restrict__ luts,
                                                        int lut_words, int lut_stride, int use_prefix,
                                                        int n_ch, int parts, unsigned long long* xchg,
                                                        int* __restrict__ fault, int phase, unsigned tag_base, const TickServer srv) {
    constexpr int kTaps = NT;
    constexpr int kXchgWords = xchg_words(NT);
    constexpr bool kCluster = THREADS == 256 && WAVES == 1;
    extern __shared__ double smem[];
    double* red = smem;                                   // kWaves * 2*NT wave sums, then the exchange staging
    EpochShared* sh = reinterpret_cast<EpochShared*>(red + kRedDoubles);
    double2* prefix = reinterpret_cast<double2*>(sh + 1);  // THREADS * kPrefixSlots, when the launcher found room
    uint32_t* lut = reinterpret_cast<uint32_t*>(prefix + (use_prefix ? THREADS * kPrefixSlots : 0));

    const int tid = threadIdx.x;
    // (uniform) a tick-server launch of the cluster form: resident, every tick behind the doorman's release
    const bool server = kCluster && srv.host != nullptr;
    int n_wg = (int)gridDim.x;
    int bid = (int)blockIdx.x;
    // (uniform) a one-launch receiver tick that brings its slab along: the launch's first workgroups are the ingest
    const bool with_slab = kCluster && !server && srv.ingest_n16 != 0;
    if constexpr (kCluster) {
        if (with_slab) {
            if (bid < kTickIngestGroups) {
                const uint4* const src = reinterpret_cast<const uint4*>(static_cast<uintptr_t>(srv.ingest_src16) << 4);
                for (unsigned long long i = (unsigned long long)bid * THREADS + tid; i < srv.ingest_n16; i += (unsigned long long)kTickIngestGroups * THREADS) {
                    unsigned long long d = srv.ingest_first16 + i;
                    if (d >= srv.ring_n16) d -= srv.ring_n16;
                    uint4 o = src[i];
                    o.x ^= srv.ring_flip, o.y ^= srv.ring_flip, o.z ^= srv.ring_flip, o.w ^= srv.ring_flip;
                    srv.ring16[d] = o;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // every wave: its stores have left (the barrier orders them ...)
                __syncthreads();                                          // ... before lane 0's device-wide release)
                if (tid == 0) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                    __hip_atomic_fetch_add(srv.ingest_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                return;
            }
            bid -= kTickIngestGroups;
            n_wg -= kTickIngestGroups;
        }
    }
    // Workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8): the parts of one channel are
    // blockIdx-es with the same residue, so a cluster shares one XCD's L2 for its exchange lines.
    int ch, part;
    const bool collect_only = kCluster && phase == 2;      // (uniform) second half of a two-launch tick: no correlation here
    const bool publish_only = kCluster && phase == 1;      // (uniform) first half: ends after publishing its sums
    // (uniform) the two halves in ONE plain launch: every part publishes its sums and draws a ticket; the part that draws its
    // channel's last one carries on as phase 2 would (it polls the lines, its own among them, and adds them in part order:
    // the same bits), the others end.  Nobody waits for a peer that may not be resident: a line that is still on its way is
    // a store already issued by a workgroup that has run.
    const bool last_collects = kCluster && phase == 3;
    if (collect_only) {
        ch = bid;
        part = 0;
    } else if (parts == 1 || n_wg % (8 * parts) != 0) {
        ch = bid / parts;
        part = bid % parts;
    } else {
        const int per_xcd = n_wg / 8;                    // workgroups per XCD = channels per XCD * parts
        const int xcd = bid % 8, q = bid / 8;
        ch = xcd * (per_xcd / parts) + q / parts;
        part = q % parts;
    }
    const int lane_global = part * THREADS + tid;          // index among the cluster's lanes
    const int cluster_lanes = parts * THREADS;
    const bool edge_wave = lane_global >= cluster_lanes - 64;
    const int edge_lane = edge_wave ? lane_global - (cluster_lanes - 64) : -1;
    const int sidx = ch_map ? ch_map[ch] : ch;             // where this channel's state and configuration live
    const sdr_loop_cfg* __restrict__ cfg_ptr = cfgs + (size_t)sidx * cfg_stride;
    {   // the channel's state and configuration into LDS, one 64-bit word per lane (a single thread copying the 472
        // bytes is ~60 loads one after the other: microseconds of a one-epoch receiver tick)
        constexpr int kStWords = (int)(sizeof(sdr_track_state) / 8), kCfgWords = (int)(sizeof(sdr_loop_cfg) / 8);
        static_assert(sizeof(sdr_track_state) % 8 == 0 && sizeof(sdr_loop_cfg) % 8 == 0 && kStWords <= 64 && kCfgWords <= 64,
                      "state / configuration are copied as 64-bit words by the first two waves");
        if (tid < kStWords)
            reinterpret_cast<unsigned long long*>(&sh->st)[tid] = reinterpret_cast<const unsigned long long*>(states + sidx)[tid];
        else if (tid >= 64 && tid < 64 + kCfgWords)
            reinterpret_cast<unsigned long long*>(&sh->cfg)[tid - 64] = reinterpret_cast<const unsigned long long*>(cfg_ptr)[tid - 64];
    }
    if (tid == 0) {
        sh->epochs_done = 0;
        sh->fault = 0;
    }
    const int slot = states[sidx].code_slot;
    if (!collect_only) stage_lut<THREADS>(lut, luts + (size_t)slot * lut_stride, lut_words, tid);
    const double fs = cfg_ptr->fs;
    UpdateCtx u;
    u.fs = fs;
    u.chips = cfg_ptr->epoch_chips > 0.0 ? cfg_ptr->epoch_chips : kDefaultEpochChips;
    u.epochs_per_bit = cfg_ptr->epochs_per_bit > 0 ? cfg_ptr->epochs_per_bit : kDefaultEpochsPerBit;
    u.dt = cfg_ptr->epoch_seconds > 0.0 ? cfg_ptr->epoch_seconds : kDefaultEpochSeconds;
    u.by_fs = inv_den(fs);
    u.by_dt = inv_den(u.dt);
    u.by_2pi = inv_den(kGpsTwoPi);
    // the one-workgroup forms (three 256-thread workgroups per compute unit at 168 registers per lane; 512 threads, two waves
    // per SIMD): no registers to spare for what only the roles read
    constexpr bool kDense = !kCluster;
    if constexpr (kDense) {
        if (tid == 0) {
            UpdateConsts c;
            c.fs = u.fs, c.chips = u.chips, c.dt = u.dt, c.epochs_per_bit = u.epochs_per_bit;
            c.by_fs_b = u.by_fs.b, c.by_fs_y = u.by_fs.y, c.by_dt_b = u.by_dt.b, c.by_dt_y = u.by_dt.y;
            c.by_2pi_b = u.by_2pi.b, c.by_2pi_y = u.by_2pi.y;
            c.ok_bits = (u.by_fs.ok ? 1 : 0) | (u.by_dt.ok ? 2 : 0) | (u.by_2pi.ok ? 4 : 0);
            sh->uc = c;
        }
    } else {
        // (vector registers: the scalar file is full of per-epoch constants, and spilled SGPRs come back as v_readlane)
        asm volatile("" : "+v"(u.fs), "+v"(u.chips), "+v"(u.dt));
        asm volatile("" : "+v"(u.by_fs.b), "+v"(u.by_fs.y), "+v"(u.by_dt.b), "+v"(u.by_dt.y), "+v"(u.by_2pi.b), "+v"(u.by_2pi.y));
    }
    u.capacity = capacity;
    u.lut_words = lut_words;
    u.n_epochs = n_epochs;
    u.ch = ch;
    u.nav_bits = nav_bits;
    u.max_bits = max_bits;
    sdr_track_state& st = sh->st;
    bool writer = part == 0;                               // one part records trajectory, bits and the end state (phase 3: the
    u.writer = writer;                                     // part that drew the channel's last ticket; part 0 of a stopped channel)

#ifdef SDR_TRACE_TRACK
    unsigned long long mark_ = wall_clock64();
    const unsigned long long clk0_ = clock64(), wall0_ = wall_clock64();   // shader clock the kernel really runs at
    if (tid == 0 && ch == 0 && part == 0) for (int k = 0; k < 64; ++k) g_track_phase[k] = 0;
    __syncthreads();
#endif
    // Each update role owns a disjoint set of fields of the state's LDS copy (loaded into registers for the
    // duration of its update only: carried across the correlation they cost ~50 VGPRs and spill) and publishes its
    // part of the next epoch's parameters.
    const int role = tid >> 6, rlane = tid & 63;
    const sdr_track_state s_init = states[sidx];
    if (tid == 0) {  // parameters of the first epoch
        double smin = cfg_ptr->spacing_wide[0], smax = smin;
        for (int t = 0; t < kTaps; ++t) {
            smin = fmin(smin, fmin(cfg_ptr->spacing_wide[t], cfg_ptr->spacing_narrow[t]));
            smax = fmax(smax, fmax(cfg_ptr->spacing_wide[t], cfg_ptr->spacing_narrow[t]));
        }
        sh->smin = smin;
        sh->smax = smax;
        sh->stop_code = code_out_of_range(sh, capacity, lut_words, s_init.current_sample, s_init.n_samples, s_init.rem_code,
                                          s_init.code_step) ? 1 : 0;
        sh->stop_carrier = carrier_bad(s_init.carrier_hz) ? 1 : 0;
        const double* sp = s_init.spacing_sel ? cfg_ptr->spacing_narrow : cfg_ptr->spacing_wide;
        sh->ep.start_sample = s_init.current_sample;
        sh->ep.n = s_init.n_samples;
        sh->ep.carrier_hz = s_init.carrier_hz;
        sh->ep.rem_carrier = s_init.rem_carrier;
        sh->ep.rem_code = s_init.rem_code;
        sh->ep.code_step = s_init.code_step;
        for (int t = 0; t < kTaps; ++t) sh->spacing[t] = sp[t];
        sh->dphi = carrier_step(s_init.carrier_hz, fs);
        sh->fll_bw = s_init.fll_bw;
        sh->pll_bw = s_init.pll_bw;
        sh->lock_state = s_init.lock_state;
        sh->c_code_counter = sh->l_code_counter = s_init.code_counter;
        sh->l_ipp = s_init.i_prompt_prev;
        sh->l_qpp = s_init.q_prompt_prev;
        sh->l_bits_run = 0;
        // the quotients the roles keep instead of re-dividing (see EpochShared)
        sh->at_prev = atan(s_init.q_prompt_prev / s_init.i_prompt_prev);
        sh->w0f_bw = s_init.fll_bw, sh->w0p_bw = s_init.pll_bw;
        sh->w0f = s_init.fll_bw / kW0Bw1, sh->w0p = s_init.pll_bw / kW0Bw2;
        sh->pll_r1 = cfg_ptr->pll_tau2 / cfg_ptr->pll_tau1, sh->pll_r2 = cfg_ptr->pll_pdi / cfg_ptr->pll_tau1;
        sh->dll_r1 = cfg_ptr->dll_tau2 / cfg_ptr->dll_tau1;
        sh->dll_r2 = (cfg_ptr->loop_kind != 0 ? cfg_ptr->dll_pdi * 1.0 : cfg_ptr->dll_pdi) / cfg_ptr->dll_tau1;
    }
    // (cluster form) this lane's 16-sample group of the current epoch and of the next one: where epoch k+1 starts is
    // known when epoch k starts, so its samples are requested a whole epoch ahead
    Raw8<FMT> cur[2], nxt[2];
    bool have_next = false;
    LockRegs lk = lock_regs_from(s_init);                  // (meaningful in lane 0 of the lock role's wave only)
    if constexpr (kDense)
        if (tid == 0) sh->lk = lk;                         // (the dense form keeps it in LDS: see EpochShared)
    // ring position of the current epoch's first sample: start % capacity once, then += n (minus the capacity when it
    // passes it) -- the 64-bit modulo is not paid three times per epoch
    int64_t ring_pos;
    {
        const int64_t p0 = s_init.current_sample % capacity;
        ring_pos = ((int64_t)__builtin_amdgcn_readfirstlane((int)(p0 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)p0);
    }
    // the channel's state as the roles' LDS copy and their last announcement give it (lane 0 of the recording part)
    auto compose_state = [&]() {
        st.current_sample = sh->ep.start_sample;
        st.n_samples = sh->ep.n;
        st.carrier_hz = sh->ep.carrier_hz;
        st.rem_carrier = sh->ep.rem_carrier;
        st.rem_code = sh->ep.rem_code;
        st.code_step = sh->ep.code_step;
    };
    unsigned server_tick = 0;                              // (server) requests this workgroup has seen
    for (int epoch = 0; epoch < n_epochs; ++epoch) {
        TRACK_MARK(5);
        __syncthreads();
        TRACK_MARK(0);
#ifdef SDR_TRACE_TRACK
        const unsigned long long wave_mark_ = wall_clock64();
#endif
        if constexpr (kCluster) {
            if (server) {
                // ---- the gate: wait for the doorman's release of the next request (bounded), see the samples it brought
                if (tid == 0) {
                    const unsigned want = server_tick + 1;
                    const unsigned long long t0 = wall_clock64();
                    unsigned g;
                    // (four looks in flight, a quarter of a round trip apart: a look that left just before the release landed
                    // is followed by one that sees it a quarter of a round trip later, not a whole one)
                    unsigned* const go = &srv.go[(size_t)ch * kGoStride];
                    auto look = [&]() { return __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
                    auto hit = [&](unsigned v) { return v == want || v == kServerStop; };
                    unsigned l0 = look();
                    __builtin_amdgcn_s_sleep(3);
                    unsigned l1 = look();
                    __builtin_amdgcn_s_sleep(3);
                    unsigned l2 = look();
                    __builtin_amdgcn_s_sleep(3);
                    unsigned l3 = look();
                    for (;;) {
                        if (hit(l0)) { g = l0; break; }
                        l0 = look();
                        if (hit(l1)) { g = l1; break; }
                        l1 = look();
                        if (hit(l2)) { g = l2; break; }
                        l2 = look();
                        if (hit(l3)) { g = l3; break; }
                        l3 = look();
                        if (wall_clock64() - t0 > 2 * srv.idle_ticks) {
                            g = kServerStop;
                            break;
                        }
                    }
                    sh->gate = g;
#ifdef SDR_SRV_TRACE
                    if (writer) {
                        const unsigned long long at = __hip_atomic_load(&srv.dev->seen_at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        srv.dev->ch_gate[ch] += wall_clock64() - at;
                        unsigned hw, xcc;
                        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
                        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                        srv.dev->ch_where[ch] = (xcc << 16) | (hw & 0xffff);
                    }
#endif
                    // (the request's write index now, past the L2: its round trip runs beside the invalidation below)
                    sh->gate_wi = __hip_atomic_load(&srv.dev->write_index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (ch == 0 && part == 0) srv.dev->t[0] = wall_clock64();
                }
                __syncthreads();
                if (sh->gate == kServerStop) break;
                ++server_tick;
                // (the slab was written through another XCD's L2: one invalidation serves the compute unit; the barrier hands it on)
                if (tid < 64) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __syncthreads();
                if (tid == 0 && ch == 0 && part == 0) srv.dev->t[1] = wall_clock64();
                const bool dead = (sh->fault | sh->stop_code | sh->stop_carrier) != 0;
                bool ready = false;
                if (!dead) {
                    const int64_t wi = sh->gate_wi;
                    const int64_t unread = ring_pos <= wi ? wi - ring_pos : capacity - ring_pos + wi;   // circularbuffer.py:139-148
                    ready = unread >= (int64_t)sh->ep.n;
                }
                if (!ready) {       // (uniform over the channel's parts: same state, same write index)
                    if (tid == 0 && writer) {
                        __hip_atomic_store(&srv.h_ran[ch], dead ? -1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (acknowledged: in the host's memory -- see the answer below)
                        __hip_atomic_store(&srv.h_done[ch], server_tick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        __hip_atomic_fetch_add(&srv.dev->done_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    --epoch;        // (this channel's next epoch is still the same one)
                    continue;
                }
            }
        }
        if constexpr (kCluster) {
            if (with_slab && epoch == 0) {
                // the slab this launch brought along: in the ring when the ingest workgroups have all counted themselves in (they
                // were dispatched in front of this one; bounded all the same), visible once this compute unit's caches are told
                if (tid == 0) {
                    const unsigned long long t0 = wall_clock64();
                    while ((int)(__hip_atomic_load(srv.ingest_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - srv.ingest_target) < 0) {
                        if (wall_clock64() - t0 > 200000ull) {      // 2 ms of the 100 MHz clock
                            sh->fault = 1;
                            *fault = 2;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                __syncthreads();
                if (tid < 64) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __syncthreads();
            }
        }
        if (sh->fault | sh->stop_code | sh->stop_carrier) break;
        const EpochParams ep = uniform_params(sh->ep);
        const double dphi = uniform(sh->dphi);
        // what the carrier loop needs from the state machine's previous decision (captured now: the lock role
        // rewrites these while the carrier role is still running)
        u.ep = ep;
        u.cur_fll_bw = uniform(sh->fll_bw), u.cur_pll_bw = uniform(sh->pll_bw);
        u.cur_lock_state = __builtin_amdgcn_readfirstlane(sh->lock_state);
        u.epoch = epoch;
        u.rec = (writer && keep_traj) ? traj + ((size_t)ch * n_epochs + epoch) : nullptr;
        if constexpr (kCluster)
            if (server) u.rec = writer ? srv.rec_out + ch : nullptr;

        double accr[kTaps], acci[kTaps];
#pragma unroll
        for (int t = 0; t < kTaps; ++t) accr[t] = acci[t] = 0.0;
        bool single = collect_only;                            // (phase 2: neither correlator runs)
        int64_t ring_pos_next = ring_pos + ep.n;               // (n <= capacity: checked by the role that announced it)
        if (ring_pos_next >= capacity) ring_pos_next -= capacity;
        if constexpr (kCluster) if (!collect_only) {
            const SingleGeometry geo = single_geometry(ring_pos, ep.n, capacity);
            single = use_prefix && ep.code_step >= kFastMinCodeStep && ep.code_step <= kFastMaxCodeStep && geo.fits &&
                     geo.groups <= cluster_lanes;
            if (single) {
                if (have_next) {
                    cur[0] = nxt[0];
                    cur[1] = nxt[1];
                } else {
                    single_load<FMT>(ring, single_load_pos(geo, lane_global, capacity), cur);
                }
                EpochConsts<kTaps> K;
                compute_constants<kTaps>(K, ep, sh->spacing, dphi, cluster_lanes);
                TRACK_MARK(1);
                correlate_epoch_single<FMT, kTaps>(cur, ep, dphi, K, lut, prefix, tid, lane_global, geo, accr, acci);
            }
        }
        if (!single) {
            const bool boundary_ok = use_prefix && ep.code_step >= kFastMinCodeStep && !epoch_wraps(ep, capacity);  // (uniform)
            EpochConsts<kTaps> K;
            // (uniform) the chip-aligned core will be tried: it reads the taps' constants only, not the in-group rotations
            bool try_chip = false;
            // (the 256-thread dense form only: in the 512-thread form a lane owns two chips and the routine's per-epoch part
            // outweighs them -- measured 10.1 against 9.4 us per epoch at 256 channels)
            if constexpr (FMT == SDR_FMT_CI8 && kTaps == 3 && !kCluster && THREADS == 256)
                try_chip = boundary_ok && ep.code_step >= kChipMinCodeStep && ep.code_step <= kChipMaxCodeStep && ring_pos + ep.n + 32 <= capacity;
            // (the in-group rotations are computed either way: taking compute_tap_constants() on the chip path and these only
            // on a fallback was measured at 26.5 instead of 15.8 us per epoch in the 168-register form -- it spills)
            compute_constants<kTaps>(K, ep, sh->spacing, dphi, cluster_lanes);
            TRACK_MARK(1);
            // one-workgroup forms, ci8, three taps, 24 / 25 samples per chip (the headline 25 MHz): lanes own whole chips
            // (correlator_chip.h, block length compiled in, tap positions at run time: ~14 instead of ~17.5 issue slots per
            // sample); its strips and rotations live where the boundary variants keep their prefix sums
            bool chip_done = false;
            if constexpr (FMT == SDR_FMT_CI8 && kTaps == 3 && !kCluster && THREADS == 256) {
                static_assert(THREADS * chip_strip_slots<3>() + (THREADS / 64) * kChipRotSlots <= THREADS * kPrefixSlots, "strips + rotations fit the prefix area");
                if (try_chip) {
                    ChipGeom<3> G;
                    chip_geometry<3, 24, 0, 0>(ep.n, K.shift, K.step, K.inv_step, G);
                    if (!__builtin_amdgcn_readfirstlane(G.bad))
                        chip_done = correlate_epoch_chip<3, false, 24, 0, 0>(ring, nullptr, capacity, ep, dphi, K, G, ring_pos, nullptr, lut, prefix,
                                                                             prefix + THREADS * chip_strip_slots<3>() + (tid >> 6) * kChipRotSlots,
                                                                             tid, lane_global, cluster_lanes, edge_lane, accr, acci);
                }
            }
            if (chip_done) {
            } else if (boundary_ok && ep.code_step <= kFastMaxCodeStep)         // 16-sample boundary variant above ~17 MHz
                correlate_epoch_wide<FMT, kTaps, false, 16>(ring, capacity, ep, dphi, K, lut, prefix, tid, lane_global, cluster_lanes, edge_lane, accr, acci);
            else if (boundary_ok && ep.code_step <= kFastMaxCodeStep8)   // 8-sample boundary variant above ~8.2 MHz
                correlate_epoch_wide<FMT, kTaps, false, 8>(ring, capacity, ep, dphi, K, lut, prefix, tid, lane_global, cluster_lanes, edge_lane, accr, acci);
            else
                correlate_epoch<FMT, kTaps>(ring, capacity, ep, dphi, K, lut, lane_global, cluster_lanes, edge_lane, accr, acci);
        }
#ifdef SDR_TRACE_TRACK
        if ((tid & 63) == 0 && ch == 0) g_track_phase[8 + part * (THREADS / 64) + (tid >> 6)] += wall_clock64() - wave_mark_;
#endif
        TRACK_MARK(2);
        if constexpr (kCluster)
            if (server && tid == 0 && ch == 0 && part == 0) srv.dev->t[2] = wall_clock64();
        // (cluster form: the totals go to wave 3, which publishes them while the three measuring roles already wait for
        // the peers' -- their chains are the epoch's critical path, the carrier-phase role's is short)
        double total;
#ifdef SDR_TRACE_TRACK
        unsigned long long role_mark_ = 0;
#endif
        if constexpr (kCluster) total = collect_only ? 0.0 : reduce_taps_rows<kTaps, THREADS, 3>(accr, acci, red, tid);   // value v in lanes v*G.. of wave 3
        else total = reduce_taps<kTaps, THREADS, 0>(accr, acci, red, tid);
        TRACK_MARK(3);
#ifdef SDR_TRACE_TRACK
        role_mark_ = wall_clock64();   // (all waves leave the reduction barrier together: per-role time from here to the end of its update)
#endif

        double corr[2 * kTaps];
        bool role_ok = true;
        if constexpr (kCluster) {
            // Cluster exchange: wave 3 publishes this part's sums; each of the three measuring roles collects the
            // parts' sums for itself and adds them in part order -- every role wave of every part holds bit-identical
            // totals, there is no second hand-over.  No fences, no separate flag: every 64-bit word carries half a
            // double and the epoch tag (epoch+1), is written and read whole, and validates itself (the "LL" idea of
            // collective libraries) -- an agent-scope release/acquire pair would write back and invalidate the whole
            // L2 every epoch (measured: 2.9 us); a relaxed device-scope word costs ~0.4 us one way
            // (tools/ubench_xchg.hip), on the same XCD or across XCDs.
            // Lines are double-buffered by epoch parity: a part can run at most one exchange ahead of a peer (its
            // wave 3 publishes epoch k+1 only after the workgroup's reduction barrier of that epoch, i.e. after
            // all its role waves have finished reading epoch k).
            unsigned long long* lines = xchg + ((size_t)ch * 2 + (epoch & 1)) * kMaxParts * kXchgWordsMax;
            const unsigned long long tag = (unsigned long long)((unsigned)(epoch + 1) + tag_base) << 32;
            if (role == 3 && !collect_only) {   // lane 2v+h publishes half h of value v (lanes 0..2*NT-1 hold the values)
                const double v = __shfl(total, ((rlane >> 1) & 15) * collector_group_lanes(NT), 64);
                if (rlane < 4 * kTaps) {
                    const unsigned half = (rlane & 1) ? (unsigned)__double2hiint(v) : (unsigned)__double2loint(v);
                    __hip_atomic_store(lines + part * kXchgWords + rlane, tag | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (publish_only) return;   // (the whole workgroup: phase 2 takes it from here, in the next launch)
            if (last_collects) {
                // tickets: one counter per position in the launch's list, in front of the lines, never reset -- every launch of this
                // form adds `parts` to the counters it uses, so "the last of this launch" is the ticket that completes a multiple
                // of `parts`, whichever channel had the position the tick before
                if (tid == 192) {
                    unsigned* tickets = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(xchg) - kXchgHeadBytes);
                    sh->gate = __hip_atomic_fetch_add(tickets + ch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();
                if ((sh->gate + 1u) % (unsigned)parts != 0u) return;      // (the whole workgroup: a later part collects)
                writer = true;
                u.writer = true;
                u.rec = keep_traj ? traj + ((size_t)ch * n_epochs + epoch) : nullptr;
            }
            // Request the next epoch's samples now -- after this epoch's last use of `cur`, before the wait for the
            // peers, so that nothing waits on them: they arrive while this wave sleeps (the counter a wave waits on
            // retires loads in order, and these are ~0.4 us older than the first poll).
            have_next = single && epoch + 1 < n_epochs && !server;   // (server: the next epoch's samples are not in the ring yet)
            if (have_next) {
                const SingleGeometry next = single_geometry(ring_pos_next, ep.n, capacity);
                single_load<FMT>(ring, single_load_pos(next, lane_global, capacity), nxt);
            }
            if (role < 3) {
                // lane l polls word l % W of parts l / W + j * (64 / W), j = 0 .. W/8 - 1 (words 4*NT.. of a line are padding)
                constexpr int kPerPass = 64 / kXchgWords;      // parts covered by one wave-wide load
                constexpr int kPasses = kMaxParts / kPerPass;  // 2 (16-word lines) or 4 (32-word lines)
                const int k = rlane & (kXchgWords - 1), pbase = rlane / kXchgWords;
                bool want[kPasses];
                const unsigned long long* addr[kPasses];
#pragma unroll
                for (int j = 0; j < kPasses; ++j) {
                    const int p = pbase + j * kPerPass;
                    want[j] = k < 4 * kTaps && p < parts;
                    addr[j] = lines + (want[j] ? p : part) * kXchgWords + (want[j] ? k : 0);
                }
                unsigned long long w[kPasses];
                bool done = false;
                // The peers' words cannot be there before a store has crossed to the L2 (~0.4 us): a poll issued at
                // once is wasted -- and 768 waves polling the lines their peers are storing to slow those stores
                // down (tools/ubench_sload.hip: a store -> load round trip is 1029 cycles alone, 1664 with every
                // workgroup polling).  Sleeping ~1000 cycles before the first poll: 5.2 -> 4.8 us per epoch at 32
                // channels (measured 4 / 8 / 12 / 16 / 20 / 28 x 64 cycles: 5.13, 4.97, 4.94, 4.82, 4.87, 5.04).
                // (phase 2: the words were there before this launch began; phase 3: every peer had stored its own before it drew
                // the ticket in front of this workgroup's)
                if (!collect_only && !last_collects) __builtin_amdgcn_s_sleep(kXchgSleep);
                for (long spins = 0; spins < kSpinLimit; ++spins) {
                    bool ok = true;
#pragma unroll
                    for (int j = 0; j < kPasses; ++j) {
                        w[j] = __hip_atomic_load(addr[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ok = ok && (!want[j] || (w[j] >> 32 << 32) == tag);
                    }
                    if (__all(ok)) {
                        done = true;
                        break;
                    }
                }
                if (!done) {
                    role_ok = false;
                    if (rlane == 0) {
                        sh->fault = 1;
                        *fault = 1;
                    }
                } else {
                    unsigned* halves = reinterpret_cast<unsigned*>(red + 256) + role * kXchgStageWords;  // this wave's staging
#pragma unroll
                    for (int j = 0; j < kPasses; ++j) halves[j * 64 + rlane] = (unsigned)w[j];  // [(p)*W + k], p = pbase + j*kPerPass
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (LDS serves a wave's operations in order)
                    __builtin_amdgcn_wave_barrier();
                    double sum = 0.0;
                    if (rlane < 2 * kTaps) {
                        for (int p = 0; p < parts; ++p) {
                            const int at = ((p / kPerPass) * 64) + (p % kPerPass) * kXchgWords;
                            sum += __hiloint2double((int)halves[at + 2 * rlane + 1], (int)halves[at + 2 * rlane]);
                        }
                    }
#pragma unroll
                    for (int k2 = 0; k2 < 2 * kTaps; ++k2) corr[k2] = lane_value(sum, k2);
                }
            } else {
#pragma unroll
                for (int k2 = 0; k2 < 2 * kTaps; ++k2) corr[k2] = 0.0;   // (the carrier-phase role measures nothing)
            }
            TRACK_MARK(6);
        } else {
            // one workgroup per channel: the totals reach the roles on waves 1 and 2 through LDS
            if (tid < 2 * kTaps) sh->corr[tid] = total;
            __syncthreads();
            TRACK_MARK(7);
#pragma unroll
            for (int k2 = 0; k2 < 2 * kTaps; ++k2) corr[k2] = uniform(sh->corr[k2]);
        }
        ring_pos = ring_pos_next;
        if constexpr (kCluster)
            if (server && tid == 0 && ch == 0 && part == 0) srv.dev->t[3] = wall_clock64();
        if (role_ok && role < 4) loop_update<kTaps, kDense>(sh, u, corr, role, rlane, lk);
#ifdef SDR_TRACE_TRACK
        if (rlane == 0 && role < 4 && ch == 0 && part == 0) g_track_phase[48 + role] += wall_clock64() - role_mark_;
#endif
        TRACK_MARK(4);
        if constexpr (kCluster) {
            if (server) {       // ---- the channel's answer, straight to the host: state and record, then the request's number
                if (tid == 0 && ch == 0 && part == 0) srv.dev->t[4] = wall_clock64();
                if (role == 2 && rlane == 0) lock_regs_store(lk, sh);
                __syncthreads();
                if (writer && tid < 64) {
                    if (tid == 0) compose_state();                          // (the NCO values the roles announced, into the LDS copy)
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (LDS serves a wave's operations in order)
                    __builtin_amdgcn_wave_barrier();
                    // one wave, 8 bytes per lane: the state out of LDS, the record the roles wrote (this workgroup's own stores:
                    // the barrier above orders them), the flag -- page-locked memory, one store instruction
                    constexpr int kStateWords = (int)(sizeof(sdr_track_state) / 8), kRecWords = (int)(sizeof(sdr_track_epoch) / 8);
                    static_assert(sizeof(sdr_track_state) % 8 == 0 && sizeof(sdr_track_epoch) % 8 == 0 && kStateWords + kRecWords < 64,
                                  "the answer is one 8-byte store per lane of one wave");
                    // (system-scope stores: past every cache, so that "the wave's stores are acknowledged" below means "they are in
                    // the host's memory".  A release FENCE here writes the whole XCD's L2 back -- the four channels that answer on
                    // one XCD queued behind each other for it: the last answer came 3 us after the median one)
                    if (tid < kStateWords)
                        __hip_atomic_store(reinterpret_cast<unsigned long long*>(srv.h_st + ch) + tid,
                                           reinterpret_cast<const unsigned long long*>(&sh->st)[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    else if (tid < kStateWords + kRecWords)
                        __hip_atomic_store(reinterpret_cast<unsigned long long*>(srv.h_rec + ch) + (tid - kStateWords),
                                           reinterpret_cast<const unsigned long long*>(srv.rec_out + ch)[tid - kStateWords], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                    else if (tid == 63)
                        __hip_atomic_store(&srv.h_ran[ch], sh->fault ? -2 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (-2: a part of the cluster never published its sums)
                    if (tid == 0 && ch == 0) srv.dev->t[5] = wall_clock64();
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the wave's stores have been acknowledged ...)
                    if (tid == 0) {
                        __hip_atomic_store(&srv.h_done[ch], server_tick, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);     // ... before this one
                        const unsigned before = __hip_atomic_fetch_add(&srv.dev->done_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (ch == 0) srv.dev->t[6] = wall_clock64() + (before & 0);      // (stamped after the add has returned: the next tick reports it)
#ifdef SDR_SRV_TRACE
                        srv.dev->ch_done[ch] += wall_clock64() - __hip_atomic_load(&srv.dev->seen_at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        srv.dev->ch_n[ch] += 1;
#endif
                    }
                }
            }
        }
        // the next iteration's first barrier orders the roles' LDS writes against everyone's reads
    }
#ifdef SDR_TRACE_TRACK
    if (tid == 0 && ch == 0 && part == 0) {
        g_track_phase[62] = clock64() - clk0_;
        g_track_phase[63] = wall_clock64() - wall0_;
    }
#endif
    // End state: the roles kept the LDS copy of the state current (the lock role hands its registers back now); one lane
    // of the recording part writes it out.
    if (publish_only) return;   // (only reached when the channel was stopped before its epoch: phase 2 reports that)
    if (last_collects && !writer) return;   // (likewise: a stopped channel's parts draw no tickets, part 0 reports)
    if (role == 2 && rlane == 0) {
        if constexpr (kDense) lk = sh->lk;
        lock_regs_store(lk, sh);
    }
    // (done words: what this wave wrote of the results -- records, bits -- has been acknowledged before the barrier lets the
    // recording lane raise the channel's word)
    if (srv.done_words) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0 && writer) {
        const int epochs_done = sh->epochs_done;
        // the NCO values of the next epoch are the ones the roles published last
        compose_state();
        // stopped early (the NCO left the staged replica / the ring, or a peer part never showed up): the state is
        // the one after the last completed epoch; the records of the epochs that did not run are marked empty
        if (epochs_done < n_epochs && keep_traj)
            for (int k = epochs_done; k < n_epochs; ++k) traj[(size_t)ch * n_epochs + k].n_samples = 0;
        states[sidx] = st;
        if (states_copy) states_copy[ch] = st;   // (position in the launch's list: what the host reads back)
        if (epochs_done_out) epochs_done_out[ch] = epochs_done;
        if (n_bits) n_bits[ch] = sh->l_bits_run < max_bits ? sh->l_bits_run : max_bits;
        if (srv.done_words) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");       // (everything above is in the host's memory ...)
            __hip_atomic_store(&srv.done_words[ch], srv.done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // ... before this
        }
    }
}

}  // namespace

// track_dense.hip: the launch of the 256-thread form for more channels than CUs
hipError_t sdr_track_dense_launch(int fmt, int n_taps, int n_ch, size_t shmem, hipStream_t stream, void** args);
