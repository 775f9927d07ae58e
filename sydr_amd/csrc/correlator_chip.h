// Chip-aligned variant of the E/P/L correlator core (ci8 rings, code steps of 1/26 .. 1/16 chip per sample:
// GPS L1 C/A between ~16.4 and ~26.5 MHz, i.e. the 25 MHz of the headline configuration; BOC(1,1) half-chip codes
// at 50 MHz).
//
// The boundary variant of correlator.h gives a lane 16 consecutive SAMPLES: the chip switch of every tap falls
// somewhere inside, so all 16 running sums go through LDS (one 16-byte store per sample) and every tap pays its
// switch arithmetic per 16 samples.  Here a lane owns one whole CHIP of the centre ("anchor") tap -- the samples
// i with ceil(y_a(i)) == q, 24 or 25 of them at 25 MHz -- so
//   * the anchor tap sees no switch at all inside a lane's block;
//   * every other tap switches exactly once per block, and because all taps advance by the same step the switch
//     position is the same in every lane up to +1: split_t in {m_t, m_t + 1}, block length n in {M, M + 1}
//     with wave-uniform m_t, M;
//   * so only the running sums at those 2*NT positions are kept (a uniform branch around one LDS store at ~6 of
//     the 25 sample positions), and a tap's share of the block is
//          c(p+1) * P_n + (c(p) - c(p+1)) * P_split       p = the tap's chip at the block's first sample
//     with P_split read back from the lane's strip at a per-lane slot.
// Per sample that leaves the unavoidable part -- int8 -> fp64 (4 instructions) and the complex mix into the running
// sum (4 FMAs) -- plus ~5 instructions of amortised block overhead, against ~17.8 for the boundary variant.
//
// Exactness: a block boundary is "the first sample whose reference chip index exceeds q", with the reference's
// y(i) = fl(fl(i*step) + shift) (np.linspace).  It is PREDICTED as floor((q - shift)/step) + 1; the
// prediction can only be off when the crossing lies within ~1e-11 of a sample, and whenever any lane of the wave
// is within 2^-16 of one the wave re-derives the boundary from exact evaluations of y on both sides (rare branch).
// A lane that ever finds a split or a length outside its {m, m+1} pair (taps exactly aligned with the anchor whose
// rounding jitters, degenerate steps) raises a flag: the caller then redoes the whole epoch with the per-sample
// routine.  First and last (partial) chips of the epoch are edge samples (one per lane, per-sample arithmetic).
#pragma once

#include "correlator.h"

#pragma clang fp contract(off)

namespace sdr {

constexpr int kWaveThreads = 64;                  // one wave per channel-epoch: the ~5 us fixed latency of a workgroup is amortised over 4x more work
constexpr int kChipMax = 26;                      // samples a lane's block may hold (k = 0..25)
constexpr double kChipMinCodeStep = 1.0 / 25.9;   // blocks of at most 26 samples
constexpr double kChipMaxCodeStep = 1.0 / 15.5;   // (16.368 MHz is 16.0 samples per chip: Doppler must not decide the kernel; 31-32 MHz through the half-chip view)
constexpr int kChipRawDwords = 13;                // 52 bytes: 26 samples
// per WAVE, double2 slots of LDS behind the lanes' strips: the in-block rotations exp(-1j*k*dphi), k = 0..25, and (round 6, the
// forms with run-time positions) what the biased conversion's offset puts into a running sum of k samples, k = 0..26
constexpr int kChipRotSlots = 2 * kChipMax + 2;
template <int NT>
constexpr int chip_strip_slots() { return 2 * NT + 1; }   // double2 slots per lane (odd multiple of 16 B: conflict-free)

// Predicted first sample i with y(i) > thr on the line y = i*step + shift.
__host__ __device__ __forceinline__ int chip_first_above(double thr, double shift, double inv_step, bool& near) {
    const double u = (thr - shift) * inv_step;
    const double fl = floor(u);
    const double fr = u - fl;
    near = near || fr < kNearInteger || fr > 1.0 - kNearInteger;
    return (int)fl + 1;
}
// The same from exact evaluations of the reference expression around a prediction c.
__host__ __device__ __forceinline__ int chip_first_above_exact(int c, double thr, double step, double shift) {
    auto above = [&](int i) {
        double y = (double)i * step;   // reference arithmetic: separate multiply and add
        y = y + shift;
        return y > thr;
    };
    if (c >= 1 && above(c - 1)) return (c >= 2 && above(c - 2)) ? c - 2 : c - 1;
    if (c < 0) c = 0;
    if (above(c)) return c;
    return above(c + 1) ? c + 1 : c + 2;
}

// Compile-time loop: f(integral_constant<int, I>) for I in [B, E).
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

__device__ __forceinline__ int wave_min_i32(int x) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_xor(x, off, 64);
        x = o < x ? o : x;
    }
    return __builtin_amdgcn_readfirstlane(x);
}

// int8 -> fp64 in ONE instruction, with a known offset.  v_perm_b32 drops a sample byte (sign bit flipped: u = x + 128;
// a ci8 ring holds its bytes that way, ring_format.h kCi8Flip)
// into bits 8..15 of the high word 0x40B0_0000 of a double whose low word is zero: that double is 4096 + u = 4224 + x,
// exactly.  The straight-line kernels mix THESE into their running sums (against 2 instructions for
// v_bfe_i32 + v_cvt_f64_i32: the conversion was half of the 8-instruction floor per sample) and take the offset's share
// 4224 * (1 + 1j) * sum_k r_k out where a sum is read: the in-block rotations r_k are per-epoch constants, so that share
// is three complex scalars per epoch.  The running sums carry ~2^16 instead of ~2^9 while a half block is summed, i.e. their
// roundings are ~2^7 larger: ~1e-13 relative on an epoch's accumulators (measured; the bar is 1e-6).
#ifndef SDR_BIASED_CVT
#define SDR_BIASED_CVT 1
#endif
constexpr double kCvtBias = 4224.0;
#ifndef SDR_ALT_PAIRS
#define SDR_ALT_PAIRS 1      // (0: every sample on one set of register pairs, as before -- for A/B runs of the s_nop pads)
#endif
// The double lives in a register PAIR whose low word stays zero for the whole epoch: only the high word is rewritten
// (built from a fresh zero each time, the compiler spends a v_mov on every low word and nothing is gained).
typedef uint32_t sdr_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double biased_sample(sdr_u32x2& pair, uint32_t w_flipped, uint32_t selector, uint32_t hi_const) {
    pair.y = __builtin_amdgcn_perm(w_flipped, hi_const, selector);
    return __builtin_bit_cast(double, pair);
}
// selector of v_perm_b32 for byte `byte` of the sample dword: result = [0x40][0xB0][that byte][0x00]
constexpr uint32_t cvt_selector(int byte) { return 0x03020000u | ((uint32_t)(4 + byte) << 8) | 0x0Cu; }

// What the chip-aligned routine needs of an epoch besides its samples and its rotations: wave-uniform integers that
// follow from the taps' np.linspace constants alone.  The kernels with run-time positions derive them per epoch; for
// the straight-line ones the HOST does, when a plan is made (epl_plan.hip: sdr_epl_plan_create) -- the same function, the same
// IEEE operations -- and a wave reads them with scalar loads: ~300 vector and ~200 scalar instructions less per epoch
// (of ~5000: int64 conversions, the exact boundary evaluations of the first and last chip, a 64-bit modulo).
template <int NT>
struct ChipGeom {
    int64_t Tfx, Ufx;           // samples per chip and the anchor line's offset U = -shift/step, Q32.32
    uint64_t delta[NT];         // tap t's switch, in samples after the block start (Q32.32)
    int q0, F;                  // chips q0 + 1 .. q0 + F of the anchor tap are whole
    int head_end, tail_start;   // samples [0, head_end) and [tail_start, n) belong to the partial first and last chip
    int m[NT], J[NT];           // integer part of delta_t; the chip q + J_t tap t sits on at the start of anchor chip q
    int bad;                    // the uniform-position scheme does not cover this epoch
};

template <int NT, int KM, int KS, int KI>
__host__ __device__ __forceinline__ void chip_geometry(int n, const double* shift, const double* step, const double* inv_step,
                                                       ChipGeom<NT>& g) {
    constexpr int A = NT / 2;
    const double two32 = 4294967296.0;
    g.q0 = (int)ceil(shift[A]);
    double y_last = (double)(n - 1) * step[A];
    y_last = y_last + shift[A];
    const int q_last = (int)ceil(y_last);
    g.F = q_last - g.q0 - 1;
    g.head_end = n, g.tail_start = n;
    if (g.F > 0) {
        bool nr = false;
        g.head_end = chip_first_above_exact(chip_first_above((double)g.q0, shift[A], inv_step[A], nr), (double)g.q0, step[A], shift[A]);
        g.tail_start = chip_first_above_exact(chip_first_above((double)(q_last - 1), shift[A], inv_step[A], nr),
                                              (double)(q_last - 1), step[A], shift[A]);
    }
    g.Tfx = (int64_t)rint(inv_step[A] * two32);
    g.Ufx = (int64_t)floor(-shift[A] * inv_step[A] * two32);
    const int M = (int)(g.Tfx >> 32);                                   // block length M or M + 1
    bool bad = M < 1 || M + 1 > kChipMax || g.F > 16384 || (KM != 0 && M != KM);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        g.m[t] = M, g.J[t] = 0, g.delta[t] = 0;
        if (t == A) continue;
        // tap t sits on chip q + J_t at the block start of anchor chip q; its switch to q + J_t + 1 comes
        // delta_t >= 0 samples later (delta_t < T)
        const int64_t Ut = (int64_t)floor(-shift[t] * inv_step[t] * two32);
        int j = (int)ceil(shift[t] - shift[A]) - 1;
        int64_t d = (Ut - g.Ufx) + (int64_t)(1 + j) * g.Tfx;
        if (d < 0) {
            d += g.Tfx;
            ++j;
        } else if (d >= g.Tfx) {
            d -= g.Tfx;
            --j;
        }
        bad = bad || d < 0 || d >= g.Tfx;
        g.J[t] = j;
        g.delta[t] = (uint64_t)d;
        g.m[t] = (int)(d >> 32);
        bad = bad || (KS != 0 && (g.m[t] != KS || j != (t < A ? -1 : 0)));   // (KS: the tap sits on chip q - 1 / q at the block start)
        // (KI: on chip q + (t - A) - 1 and switching at the block's first sample, or on q + (t - A) until its end)
        bad = bad || (KI != 0 && !((j == (t - A) * KI - 1 && g.m[t] == 0) || (j == (t - A) * KI && g.m[t] >= M)));
    }
    g.bad = bad ? 1 : 0;
}

// The carrier rotations of a straight-line kernel's epoch: exp(-1j*k*dphi) inside a half block (k = 1 .. kStaticHalf),
// over the D / D + 1 samples between a lane's blocks, and the biased conversion's share of a sum of kStaticHalf - 2 / - 1 /
// - 0 samples (correlate_epoch_chip).  Evaluated by the host with the kernels' own sincos_reduced -- fused multiply-adds
// and exact roundings on both sides, i.e. the same bits a wave would get -- and the same order of additions as the
// wave's DPP prefix sum.
constexpr int kStaticHalf = 13;                 // the longest half block a straight-line kernel sums: KS + 1 = (KM + 2) / 2 for KM = 24, KS = 12
// The half block of a straight-line geometry -- samples 0 .. KS (taps switching inside the block) or (KM + 2) / 2 (whole-chip
// taps) -- and the shortest sum whose share of the conversion's offset is kept: KM - half samples (the second half up to
// the M-th sample), then + 1, + 2.
constexpr int chip_half(int KM, int KS, int KI) { return KI != 0 ? (KM + 2) / 2 : KS + 1; }
struct ChipRot {
    double urc[kStaticHalf + 1], urs[kStaticHalf + 1];
    double rd0c, rd0s, rd1c, rd1s;
    double biasc[3], biass[3];
};
// half: chip_half() of the kernel's geometry; cmin = KM - half.
__host__ __device__ inline void chip_rotations(double dphi, int Dmin, ChipRot& r, int half = kStaticHalf, int cmin = kStaticHalf - 2) {
    double cs[16], sn[16];
    for (int k = 0; k < 16; ++k) sincos_reduced(-(double)k * dphi, &sn[k], &cs[k]);
    for (int k = 1; k <= half; ++k) r.urc[k] = cs[k], r.urs[k] = sn[k];
    r.urc[0] = 1.0, r.urs[0] = 0.0;
    sincos_reduced(-(double)Dmin * dphi, &r.rd0s, &r.rd0c);
    sincos_reduced(-(double)(Dmin + 1) * dphi, &r.rd1s, &r.rd1c);
    for (int st = 1; st < 16; st <<= 1)          // inclusive prefix sums as a row of 16 lanes forms them (row_shr:1, 2, 4, 8)
        for (int l = 15; l >= st; --l) cs[l] += cs[l - st], sn[l] += sn[l - st];
    for (int i = 0; i < 3; ++i) {
        const int l = cmin + i - 1;                 // (a sum of cmin + i samples: rotations 0 .. l)
        const double re = cs[l] - sn[l], im = cs[l] + sn[l];
        r.biasc[i] = re * 4224.0, r.biass[i] = im * 4224.0;
    }
}

// ---- Half blocks summed as folded sample pairs.  A half block is summed against rotations that are the same in every
// lane; taken about the CENTRE of the run of samples that is always summed, the rotations of the samples d before and d
// after it are complex conjugates, so with a = x(-d), b = x(+d) and (c, s) = (cos, sin)(d * dphi)
//     a (c + 1j s) + b (c - 1j s) = c (a + b) + 1j s (a - b):      Re += c SI - s DQ,    Im += c SQ + s DI
// four FMAs for two samples.  S = a + b and D = a - b are sums of bytes: v_perm_b32 gathers G = [aI aQ bI bQ] from the two
// raw dwords, G2 = G ^ 0xFFFF0000 holds 255 - u for the b half, and v_dot4_u32_u8 with the byte weight 128 on two of the
// four bytes, added onto the high word 0x40C0_0000 of 8192.0 (one unit of that word is 2^-7), leaves the high words of
// the exact doubles 8192 + ua + ub = 8448 + (xa + xb) and 8192 + ua + 255 - ub = 8447 + (xa - xb).  Ten instructions per
// pair, four of them fp64, against twelve and eight.  The run's optional last sample -- the one a lane's flag masks, see
// chip_mask_shares() -- stays a single biased sample (4224 + x), and so does the centre sample of a run of odd length, which
// starts the sum.  Both halves are referred to their own centres: the lane's block phasor is evaluated at the first half's
// centre instead of the block's first sample, and the second half is turned by the distance of the two centres.
#ifndef SDR_FOLD_PAIRS
#define SDR_FOLD_PAIRS 1     // (0: the direct sum of every form, the text of the kernels before folding -- for A/B runs)
#endif
#ifndef SDR_TURN_ONCE
#define SDR_TURN_ONCE 1      // (0: every tap's share of a block turned by the block phasor on its own, as before -- for A/B runs)
#endif
constexpr int kFoldPairsMax = kStaticHalf / 2;  // pairs of the longest run
constexpr double kFoldSumBias = 8192.0 + 256.0, kFoldDiffBias = 8192.0 + 255.0;
// The runs of a geometry: half h (0: samples from 0, 1: samples from chip_half()) always sums `count` samples from `first`;
// its optional last sample is first + count (the first half has one only where taps switch inside the block: KS).
constexpr int chip_fold_first(int half, int h) { return h == 0 ? 0 : half; }
constexpr int chip_fold_count(int KM, int half, bool ks, int h) { return h == 0 ? (ks ? half - 1 : half) : KM - half; }
struct ChipFold {
    double pc[2][kFoldPairsMax], ps[2][kFoldPairsMax];   // (cos, sin)(d * dphi) of pair i of half h, from the outside in: d = (count - 1) / 2 - i
    double sc[2], ss[2];                                 // the optional last sample's rotation about its half's centre: (cos, sin)(-(count + 1) / 2 * dphi)
    double tc, ts;                                       // second half onto the first half's centre: (cos, sin)(-(centre1 - centre0) * dphi)
    double shc[4], shs[4];                               // the offsets' share of: first half, first half with its last sample, second half, ... with its last sample
};
__host__ __device__ inline void chip_fold_constants(double dphi, int KM, int half, bool ks, ChipFold& f) {
    f = ChipFold{};
    for (int h = 0; h < 2; ++h) {
        const int count = chip_fold_count(KM, half, ks, h);
        double re = (count & 1) ? kCvtBias : 0.0, im = re;      // (the centre sample of an odd run: rotation 1)
        for (int i = 0; i < count / 2; ++i) {
            const double d = 0.5 * (double)(count - 1 - 2 * i);  // (half-integers are exact)
            sincos_reduced(d * dphi, &f.ps[h][i], &f.pc[h][i]);
            re += f.pc[h][i] * kFoldSumBias - f.ps[h][i] * kFoldDiffBias;
            im += f.pc[h][i] * kFoldSumBias + f.ps[h][i] * kFoldDiffBias;
        }
        sincos_reduced(-0.5 * (double)(count + 1) * dphi, &f.ss[h], &f.sc[h]);
        f.shc[2 * h] = re, f.shs[2 * h] = im;
        f.shc[2 * h + 1] = re + (f.sc[h] - f.ss[h]) * kCvtBias, f.shs[2 * h + 1] = im + (f.sc[h] + f.ss[h]) * kCvtBias;
    }
    const double turn = (double)chip_fold_first(half, 1) + 0.5 * (double)(chip_fold_count(KM, half, ks, 1) - 1) -
                        0.5 * (double)(chip_fold_count(KM, half, ks, 0) - 1);
    sincos_reduced(-turn * dphi, &f.ts, &f.tc);
}
// Which forms fold (per-form guard): a form that would lose a wave per SIMD or gain scratch by it keeps the direct sum.
// Folding holds eight register pairs for the doubles where the direct sum holds four, + 9 .. 17 vector registers by the
// compiler's count: the three-tap forms that run four waves per SIMD on at most 128 registers -- taps switching inside blocks
// of up to 19 samples (126 - 128 registers direct, 135 - 137 folded), whole-chip taps on blocks of 18 and more (117 - 124
// direct, 131 - 138 folded) -- would drop to three.  The other forms run three waves either way (docs/notes/K1.md).
constexpr bool chip_folds(int NT, int KM, int KS, int KI) {
    return SDR_FOLD_PAIRS != 0 && SDR_BIASED_CVT != 0 && KM != 0 && (KS != 0 || KI != 0) &&
           (NT > 3 || (KS != 0 ? KM >= 20 : KM <= 17));
}

// ---- Optional samples are masked, not selected.  Each half block has one or two samples that only some lanes sum: the
// block's sample KM where the block is M + 1 long, and (taps switching inside the block, KS) sample KS, which belongs to the
// first half where the lane's taps switch a sample late and to the second half otherwise.  A lane takes such a sample's raw
// dword or 0x80808080 (x = 0) by its flag, so every lane sums the conversion's offset in that place and a half's sum can
// START from minus the offsets' share of all its samples: c1 / s1 for the first half, c2 / s2 for the second.  From the
// plan's constants: the folded forms pair samples KS and KM about the second half's centre (rotations (sc, -+ss)[1]); the
// direct ones meet sample KS one step in front of the second half's rotation 0.
struct ChipShares {
    double c1, s1, c2, s2;
};
__host__ __device__ __forceinline__ ChipShares chip_mask_shares(const ChipFold& f, bool ks) {
    if (!ks) return ChipShares{f.shc[0], f.shs[0], f.shc[3], f.shs[3]};
    return ChipShares{f.shc[1], f.shs[1], f.shc[2] + (f.sc[1] * kFoldSumBias + f.ss[1] * kFoldDiffBias),
                      f.shs[2] + (f.sc[1] * kFoldSumBias - f.ss[1] * kFoldDiffBias)};
}
__host__ __device__ __forceinline__ ChipShares chip_mask_shares(const ChipRot& r, int KM, int half, bool ks) {
    const int i_first = 2 * half - KM;              // (biasc[i]: a sum of KM - half + i samples)
    ChipShares sh{r.biasc[i_first], r.biass[i_first], r.biasc[1], r.biass[1]};
    if (ks) {
        sh.c2 = sh.c2 + (r.urc[1] + r.urs[1]) * kCvtBias;
        sh.s2 = sh.s2 + (r.urc[1] - r.urs[1]) * kCvtBias;
    }
    return sh;
}

// One epoch of a plan as the straight-line kernels read it (device memory, one per item).
template <int NT>
struct ChipSetup {
    double dphi;                                // carrier_step(carrier_hz, fs)
    double shift[NT], step[NT], inv_step[NT];   // the taps' np.linspace constants (compute_tap_constants)
    int64_t base;                               // start_sample % capacity; < 0: the chip-aligned routine does not apply (chip_variant_applies)
    ChipGeom<NT> g;
    ChipRot r;
#if SDR_FOLD_PAIRS
    ChipFold f;                                 // (the folded forms read these in the place of r's in-block rotations and shares)
#endif
};

// ... and how one is made (one THREAD per item of a plan: epl_plan.hip's chip_setup_kernel; the host builds of the tests).
// stride: the lanes that share an epoch (a lane's blocks are that many chips apart).
template <int NT, int KM, int KS, int KI>
__host__ __device__ inline void chip_setup(int n, int64_t start_sample, int64_t capacity, double carrier_hz, double rem_code,
                                           double code_step, const double* spacing, double fs, int stride, ChipSetup<NT>& S) {
    S = ChipSetup<NT>{};
    S.dphi = carrier_step(carrier_hz, fs);
    const double nd = (double)n;
    for (int t = 0; t < NT; ++t) {             // compute_tap_constants(): np.linspace(shift, code_step*n + shift, n, endpoint=False)
        const double shift = rem_code + spacing[t];
        double stop = code_step * nd;
        stop = stop + shift;
        const double delta = stop - shift;
        S.shift[t] = shift;
        S.step[t] = delta / nd;
        S.inv_step[t] = 1.0 / S.step[t];       // (only ever predicts positions that are re-checked exactly near a sample)
    }
    const int64_t base = start_sample % capacity;
    const bool applies = code_step >= kChipMinCodeStep && code_step <= kChipMaxCodeStep && base + n + 32 <= capacity;   // chip_variant_applies()
    S.base = applies ? base : -1;
    if (applies) {
        chip_geometry<NT, KM, KS, KI>(n, S.shift, S.step, S.inv_step, S.g);
        chip_rotations(S.dphi, (int)(((int64_t)stride * S.g.Tfx) >> 32), S.r, chip_half(KM, KS, KI), KM - chip_half(KM, KS, KI));
#if SDR_FOLD_PAIRS
        if constexpr (chip_folds(NT, KM, KS, KI)) chip_fold_constants(S.dphi, KM, chip_half(KM, KS, KI), KS != 0, S.f);
#endif
    }
}

// ---- The block walk of the straight-line forms (KS / KI).  A lane carries the first sample S of its block and the 32-bit
// fraction f of that boundary on the Q32.32 line (u = S * 2^32 + f), nothing wider.  Everything a block needs beyond S is
// the CARRY of a 32-bit add onto f: the block is M + 1 samples long iff f + lo(T) carries (hi(u + T) - hi(u) - M), tap t
// switches at m_t + 1 iff f + lo(delta_t) carries, and the lane's next block starts Dmin + 1 samples on iff f + lo(stride * T)
// carries.  A carry is 0 or 1: none of the range checks of the integer formulation can fire here.  The sums f + lo(T),
// f + lo(delta_t) are also the fractions of those boundaries, which the 2^-16 window looks at: the same blocks as before go
// through the exact re-evaluation.  __host__ __device__: tests/csrc/chip_walk_dump.hip walks epochs with these on the CPU.
struct ChipWalk {
    int S;
    uint32_t f;
};
__host__ __device__ __forceinline__ ChipWalk chip_walk_at(uint64_t u) { return ChipWalk{(int)(u >> 32), (uint32_t)u}; }
__host__ __device__ __forceinline__ bool chip_carry(uint32_t a, uint32_t b, uint32_t& sum) { return __builtin_add_overflow(a, b, &sum); }
__host__ __device__ __forceinline__ bool chip_near_sample(uint32_t fr) { return fr + 0x10000u < 0x20000u; }
// The lane's next block, `stride` chips on (stride_lo = lo(stride * T), Dmin = hi(stride * T)); returns dd.
__host__ __device__ __forceinline__ bool chip_walk_step(ChipWalk& w, uint32_t stride_lo, int Dmin) {
    const bool dd = chip_carry(w.f, stride_lo, w.f);
    w.S = w.S + Dmin + (dd ? 1 : 0);
    return dd;
}
// The last round of an epoch: a lane beyond the last whole chip re-does that chip (w_last), it does not walk on.
__host__ __device__ __forceinline__ ChipWalk chip_walk_clamp(const ChipWalk& w, bool inside, const ChipWalk& w_last) {
    return ChipWalk{inside ? w.S : w_last.S, inside ? w.f : w_last.f};
}
// The flags of the block that starts at fraction f: dn, ds[t] (t != A; whole-chip taps, KI: none) and whether one of its
// boundaries lies within 2^-16 of a sample.
template <int NT, int KI>
__host__ __device__ __forceinline__ void chip_walk_flags(uint32_t f, uint32_t T_lo, const uint32_t* delta_lo, bool& dn, bool* ds, bool& near) {
    uint32_t fE;
    dn = chip_carry(f, T_lo, fE);
    near = chip_near_sample(f) || chip_near_sample(fE);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        ds[t] = false;
        if (t == NT / 2 || KI != 0) continue;
        uint32_t fT;
        ds[t] = chip_carry(f, delta_lo[t], fT);
        near = near || chip_near_sample(fT);
    }
}

// One lane's block, prepared one round ahead of its use (its loads are in flight while the previous block computes).
template <int NT>
struct ChipBlock {
    uint32_t raw[kChipRawDwords];
    int S;             // first sample of the block (epoch-relative)
    int dn;            // block length - M            (0 or 1)
    int ds[NT];        // per tap: switch position - m_t (0 or 1; anchor: unused)
    // (straight-line forms: dn / ds are the carries of the block's fraction f, taken where they are used; the integers above
    // are set only in a block that went through the exact re-evaluation -- slow != 0 -- which then speaks for the carries)
    uint32_t f;
    int slow;
    int adj;           // (slow != 0) S - the walk's S: where the exact re-evaluation moved the block's start
};

// Returns false when a lane met a configuration the uniform-position scheme does not cover: the caller redoes the
// epoch with correlate_epoch().  strip: this wave-group's [stride][chip_strip_slots<NT>()] double2; rot: kChipRotSlots double2
// private to the WAVE.
//
// Block boundaries come from a fixed-point line (Q32.32 samples): with T = 1/step samples per chip and
// U = -shift/step, the first sample whose reference y exceeds thr is floor(U + thr*T) + 1.  One 64-bit add per
// boundary per lane; a boundary whose fraction lies within 2^-16 of an integer (where fixed point, the real line
// and the reference's rounded y might disagree) sends the wave through exact evaluations of the reference
// expression instead.  Because every tap advances by the same T, the switch of tap t sits delta_t = const samples
// after the block start on the real line, so its sample position is floor(delta_t) or floor(delta_t) + 1 in every
// lane (floor(a + b) - floor(a) for b >= 0): the two LDS slots per tap are known for the whole epoch.
// KM > 0: the block length M is known when the kernel is compiled (the host checked that every epoch of the launch
// has floor(samples per chip) == KM, e.g. 24 at 25 MHz): the sample loop then has a fixed trip count and the stores
// of P_M and P_(M+1) are unconditional -- two scalar instructions per sample (bit test + branch for a tap position)
// instead of six with two branches (measured: 0.436 -> 0.40 ms per launch; testing two samples per branch with
// both bodies duplicated was slower again: 0.415).
// KS > 0 (with KM > 0): every other tap's switch position m_t is known too (KS = 12: taps half a chip either side of
// the anchor at 24.4 samples per chip -- the reference's default correlator spacing at 25 MHz; the host checked it for
// every epoch of the launch, and an epoch that disagrees is flagged and redone per sample).  All four positions
// somebody reads -- P_KS, P_(KS+1), P_KM, P_(KM+1) -- are then compile-time: they stay in registers, the sample loop
// is one straight line (no strip stores, no bit tests, no branches) and a lane masks the two samples it may not own
// (chip_mask_shares()).
// KI = 1 (with KM > 0): the taps sit whole chips apart -- tap t on chip q + (t - A) for ALL of the anchor's block of
// chip q (the five taps VE/E/P/L/VL at -1, -0.5, 0, +0.5, +1 chip of BASELINE configs 4-5 on the half-chip view of
// their replicas: -2 .. +2 half-chips at 24.4 samples per half-chip).  No tap switches inside a block, so the block
// needs ONE sum (P_M or P_(M+1)), turned by the block-start phasor once and added into every tap with that tap's
// replica value: two FMAs per tap and block, no strip, no per-tap fixed-point arithmetic.  The host checks the spacing;
// a block in which the reference's rounding lets a tap switch a sample early or late (only possible within 2^-16 of
// a sample, where the wave evaluates the reference expression exactly anyway) flags the epoch, which is redone per
// sample.
// G: chip_geometry() of the epoch, computed by the caller or read from the plan's ChipSetup; base = start_sample % capacity;
// R (straight-line forms only): the plan's chip_rotations() of the epoch; RF (the forms that fold, chip_folds()): its
// chip_fold_constants().
template <int NT, bool SINGLE_WAVE, int KM = 0, int KS = 0, int KI = 0>
__device__ __forceinline__ bool correlate_epoch_chip(const void* __restrict__ ring, const void* __restrict__ ring_flipped, int64_t capacity,
                                                     const EpochParams& ep, double dphi, const EpochConsts<NT>& K,
                                                     const ChipGeom<NT>& G, int64_t base, const ChipRot* R,
                                                     const uint32_t* lut, double2* strip_lds, double2* rot, int tid,
                                                     int lane, int stride, int edge_lane, double* accr, double* acci,
                                                     const ChipFold* RF = nullptr) {
    constexpr int A = NT / 2;                       // anchor tap: the centre one (prompt)
    constexpr int kSlots = chip_strip_slots<NT>();
    const int n = ep.n;
    const double* shift = K.shift;
    const double* step = K.step;
    double2* strip = strip_lds + tid * kSlots;
    const int wlane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < NT; ++t) accr[t] = acci[t] = 0.0;

    // ---- epoch geometry (wave-uniform): chips q0 .. q_last of the anchor tap; q0+1 .. q_last-1 are whole
    const double dphi_u = uniform(dphi), rem_carrier_u = uniform(ep.rem_carrier);
    const int q0 = __builtin_amdgcn_readfirstlane(G.q0);
    const int F = __builtin_amdgcn_readfirstlane(G.F);                  // whole chips
    const int head_end = __builtin_amdgcn_readfirstlane(G.head_end);
    const int tail_start = __builtin_amdgcn_readfirstlane(G.tail_start);
    // (the caller guarantees base + n + 32 <= capacity)
    // (the straight-line forms build their samples from the sign-flipped image of the ring: see biased_sample())
    // (round 6: the ring itself holds the sign-flipped bytes -- `ring_flipped` is the same pointer, kept in the signature)
    (void)ring_flipped;
    const char* ring_base = static_cast<const char*>(ring) + base * 2;

    // in-block rotations exp(-1j*k*dphi), k = 0..25: one per lane, parked in LDS, read back as broadcasts
    // (KS: the block is summed in two halves of KS + 1 and KM - KS samples that both start at rotation 0, so only
    // k = 1 .. KS + 1 are needed and they fit in scalar registers -- no LDS reads in the sample loop at all)
    static_assert(!(KS != 0 && KI != 0), "either the taps switch inside the block (KS) or with it (KI)");
    constexpr bool kStatic = KM != 0 && (KS != 0 || KI != 0);
    // ... of which the forms short of scalar registers -- taps switching inside the block, or five taps -- walk their blocks by
    // the fraction (ChipWalk); the three-tap whole-chip forms have registers of both kinds to spare for a fourth wave per SIMD,
    // which the walk's vector registers would cost them, and keep the 64-bit line
    constexpr bool kWalk = kStatic && (KS != 0 || NT > 3);
    constexpr int kHalf = chip_half(KM, KS, KI);
    // ... and of those, the forms that sum their half blocks as folded sample pairs (ChipFold)
    constexpr bool kFold = kStatic && chip_folds(NT, KM, KS, KI);
    constexpr int kFoldN0 = chip_fold_count(KM, kHalf, KS != 0, 0), kFoldN1 = chip_fold_count(KM, kHalf, KS != 0, 1);
    // ... and the three-tap forms whose taps switch inside the block turn a block's two sums by its phasor once and add them
    // into P, E - P and L - P (see process())
    constexpr bool kTurnOnce = SDR_TURN_ONCE != 0 && kStatic && KS != 0 && NT == 3;
    double fpc[2][kFoldPairsMax], fps[2][kFoldPairsMax], fsc[2] = {1.0, 1.0}, fss[2] = {0.0, 0.0};   // (kFold) pair and last-sample rotations
    double urc[kStatic ? kHalf + 1 : 1], urs[kStatic ? kHalf + 1 : 1];
    // (straight-line forms, biased conversion) the offsets' share of each half's sum WITH its optional samples: a half starts
    // from minus its share, and a lane without an optional sample sums the offset alone in its place (see process())
    double sh1c = 0.0, sh1s = 0.0, sh2c = 0.0, sh2s = 0.0;
    // samples per chip as Q32.32, and the distance to a lane's next block: D or D + 1 samples
    const double two32 = 4294967296.0;
    int64_t Tfx = G.Tfx;
    int64_t stride_fx = (int64_t)stride * Tfx;
    const int Dmin = (int)(stride_fx >> 32);
    // (read from the plan these arrive in scalar registers, which the rotations of the sample loop need: the per-lane
    // 64-bit arithmetic of the block boundaries takes them from vector registers, as when a wave derives them itself)
    if constexpr (kStatic) asm volatile("" : "+v"(Tfx), "+v"(stride_fx));
    double rd0c = 1.0, rd0s = 0.0, rd1c = 1.0, rd1s = 0.0;  // the carrier rotations over D and D + 1 samples
    {
        double sn = 0.0, cs = 0.0;
        if constexpr (kStatic) {
            // (worked out by the host with the plan: chip_rotations())
            static_assert(kHalf <= kStaticHalf, "the plan's rotations are laid out for half blocks of up to 13 samples");
            if constexpr (kFold) {
                static_assert(kFoldN0 / 2 <= kFoldPairsMax && kFoldN1 / 2 <= kFoldPairsMax, "the plan's pair rotations are laid out for runs of up to 13 samples");
#pragma unroll
                for (int h = 0; h < 2; ++h) {
#pragma unroll
                    for (int i = 0; i < (h == 0 ? kFoldN0 : kFoldN1) / 2; ++i) fpc[h][i] = RF->pc[h][i], fps[h][i] = RF->ps[h][i];
                    if (h == 1 || KS != 0) fsc[h] = RF->sc[h], fss[h] = RF->ss[h];
                }
                urc[kHalf] = RF->tc, urs[kHalf] = RF->ts;       // (the second half onto the first half's centre)
                const ChipShares sh = chip_mask_shares(*RF, KS != 0);
                sh1c = sh.c1, sh1s = sh.s1, sh2c = sh.c2, sh2s = sh.s2;
            } else {
#pragma unroll
                for (int k = 1; k <= kHalf; ++k) urc[k] = R->urc[k], urs[k] = R->urs[k];
                if constexpr (SDR_BIASED_CVT) {
                    const ChipShares sh = chip_mask_shares(*R, KM, kHalf, KS != 0);
                    sh1c = sh.c1, sh1s = sh.s1, sh2c = sh.c2, sh2s = sh.s2;
                }
            }
            rd0c = R->rd0c, rd0s = R->rd0s, rd1c = R->rd1c, rd1s = R->rd1s;
            // (the shares start fused multiply-adds and additions, which take them from vector registers as well: scalar
            // registers less beside the 48 - 52 of the in-block rotations of the long blocks' forms that are short of them; the
            // forms that are not keep their vector registers, some of them for a fourth wave per SIMD)
            if constexpr (SDR_BIASED_CVT && kWalk && (kHalf >= 12 || NT > 3)) asm volatile("" : "+v"(sh1c), "+v"(sh1s), "+v"(sh2c), "+v"(sh2s));
            // (the three-tap whole-chip form of 24 samples holds 52 scalar registers of rotations and runs four waves on 120 - 122
            // vector ones: one share fits there, and with both in scalar registers a spill slot stays in the frame)
            if constexpr (SDR_BIASED_CVT && !kWalk && !kFold && KM == 24) asm volatile("" : "+v"(sh2c), "+v"(sh2s));
        } else {
            if (wlane < kChipMax) {
                sincos_reduced(-(double)wlane * dphi_u, &sn, &cs);
                rot[wlane] = make_double2(cs, sn);
            }
            if constexpr (SDR_BIASED_CVT) {
                // Round 6: the ring holds sign-flipped bytes, so these forms take the one-instruction conversion too (a
                // sample arrives as 4224 + x: two v_perm_b32 instead of an exclusive or, two bit-field extracts and two
                // converts per sample).  A running sum P_k then carries 4224 (1 + 1j) sum_{i<k} r_i: btab[k], an inclusive
                // scan of the lanes' rotations, taken out where a parked sum is read.
                double br = (cs - sn) * kCvtBias, bi = (cs + sn) * kCvtBias;       // (lanes >= 26 hold zeros)
#pragma unroll
                for (int off = 1; off < 32; off <<= 1) {
                    const double o_r = __shfl_up(br, off, 64), o_i = __shfl_up(bi, off, 64);
                    br = wlane >= off ? br + o_r : br;
                    bi = wlane >= off ? bi + o_i : bi;
                }
                double2* const btab = rot + kChipMax;
                if (wlane < kChipMax) btab[wlane + 1] = make_double2(br, bi);
                if (wlane == 0) btab[0] = make_double2(0.0, 0.0);
            }
        }
    }

    bool bad = false;
    const int rounds = F > 0 ? (F + stride - 1) / stride : 0;
    if (rounds > 0) {
        // ---- the fixed-point line of the anchor tap, and each tap's constant offset on it
        int64_t Ufx = G.Ufx;
        const int M = (int)(G.Tfx >> 32);                                 // block length M or M + 1
        if constexpr (kStatic) asm volatile("" : "+v"(Ufx));
        bad = bad || G.bad != 0;
        int m[NT], J[NT];
        uint64_t delta[NT];
        unsigned evmask = (1u << M) | (2u << M);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            m[t] = G.m[t], J[t] = G.J[t], delta[t] = G.delta[t];
            if constexpr (kStatic) asm volatile("" : "+v"(m[t]), "+v"(J[t]), "+v"(delta[t]));
            if (t != A) evmask |= (1u << m[t]) | (2u << m[t]);
        }
        const int k_last = M + 1;                       // no prefix beyond P_(M+1) is ever read
        int rank[NT];                                   // strip slot of position m_t (m_t + 1 sits in the next one)
#pragma unroll
        for (int t = 0; t < NT; ++t) rank[t] = __builtin_popcount(evmask & ((1u << m[t]) - 1u));
        if constexpr (!kStatic) {
            double sn, cs;
            sincos_reduced(-(double)(Dmin + (wlane & 1)) * dphi_u, &sn, &cs);   // lane 0: Dmin, lane 1: Dmin + 1
            rd0c = lane_value(cs, 0), rd0s = lane_value(sn, 0);
            rd1c = lane_value(cs, 1), rd1s = lane_value(sn, 1);
        }
        asm volatile("" : "+v"(rd0c), "+v"(rd0s), "+v"(rd1c), "+v"(rd1s));   // (selected per lane: keep them in vector registers)
        const uint64_t lane_fx = (uint64_t)((int64_t)lane * Tfx);
        // u of the lane's block start in round 0, "+1 sample" folded in: S = u >> 32
        uint64_t u_cur = (uint64_t)(Ufx + (int64_t)q0 * Tfx + (int64_t)two32) + lane_fx;
        const int last_idx = F - 1;

        auto prepare = [&](int round, uint64_t u0, ChipBlock<NT>& b) {
            // (a lane beyond the last whole chip re-does the last one with a zero carrier phasor)
            const int idx = round * stride + lane;
            const bool inside = idx <= last_idx;
            const uint64_t uS = inside ? u0 : (uint64_t)(Ufx + (int64_t)(q0 + last_idx) * Tfx + (int64_t)two32);
            const uint64_t uE = uS + (uint64_t)Tfx;
            int S = (int)(uS >> 32);
            int E = (int)(uE >> 32);
            bool near = (uint32_t)uS + 0x10000u < 0x20000u || (uint32_t)uE + 0x10000u < 0x20000u;
            int split[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                split[t] = 0;
                if (t == A) continue;
                if constexpr (KI != 0) {
                    // (the tap's switch IS the block's boundary up to a few units of 2^-32 sample: away from `near` it
                    // falls on the same sample, so there is nothing to compute)
                    split[t] = J[t] == (t - A) * KI ? E - S : 0;
                    continue;
                }
                const uint64_t uT = uS + delta[t];
                near = near || (uint32_t)uT + 0x10000u < 0x20000u;
                split[t] = (int)(uT >> 32) - S;
            }
            if (__builtin_expect(__any(near), 0)) {
                const int q = q0 + 1 + (inside ? idx : last_idx);
                S = chip_first_above_exact(S, (double)(q - 1), step[A], shift[A]);
                E = chip_first_above_exact(E, (double)q, step[A], shift[A]);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (t == A) continue;
                    const int p0 = q + J[t];
                    // the tap must sit on p0 or p0 + 1 at S and switch to p0 + 1 at most once inside the block
                    const int bt = chip_first_above_exact(S + split[t], (double)p0, step[t], shift[t]);
                    double y = (double)S * step[t];
                    y = y + shift[t];
                    const int at_s = (int)ceil(y);
                    bad = bad || (at_s != p0 && at_s != p0 + 1) || (at_s == p0 + 1 && bt > S);
                    split[t] = bt < S ? 0 : bt - S;
                }
            }
            b.S = S;
            const int nn = E - S;
            b.dn = nn - M;
            bad = bad || (unsigned)b.dn > 1u;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                b.ds[t] = 0;
                if (t == A) continue;
                const int sp = split[t] > nn ? nn : split[t];
                if constexpr (KI != 0) {
                    bad = bad || !(J[t] == (t - A) * KI ? sp == nn : sp == 0);   // on chip q + (t - A) for the whole block
                    continue;
                }
                b.ds[t] = sp - m[t];
                bad = bad || (unsigned)b.ds[t] > 1u;
            }
            // (KS, three taps: E and L switch half a chip into the block, on the same sample away from a `near` one -- one
            // select serves both; a block where they differ flags the epoch)
            if constexpr (KS != 0 && NT == 3) bad = bad || b.ds[0] != b.ds[2];
            // 13 dwords = 26 samples from the (2-byte aligned) address of sample S: gfx950 serves unaligned dword loads
            const char* src = ring_base + (int64_t)S * 2;
            const uint4 w0 = *reinterpret_cast<const uint4*>(src);
            const uint4 w1 = *reinterpret_cast<const uint4*>(src + 16);
            const uint4 w2 = *reinterpret_cast<const uint4*>(src + 32);
            const uint32_t w3 = *reinterpret_cast<const uint32_t*>(src + 48);
            b.raw[0] = w0.x, b.raw[1] = w0.y, b.raw[2] = w0.z, b.raw[3] = w0.w;
            b.raw[4] = w1.x, b.raw[5] = w1.y, b.raw[6] = w1.z, b.raw[7] = w1.w;
            b.raw[8] = w2.x, b.raw[9] = w2.y, b.raw[10] = w2.z, b.raw[11] = w2.w;
            b.raw[12] = w3;
        };

        // ---- straight-line forms: the same block from the walk (ChipWalk): flags from carries, no integers on the fast path.
        // clampc: the round may be the epoch's last one, where a lane beyond the last whole chip re-does that chip.
        const uint32_t T_lo = (uint32_t)Tfx, stride_lo = (uint32_t)stride_fx;
        uint32_t delta_lo[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) delta_lo[t] = (uint32_t)delta[t];
        // (what the rare paths find wrong, as a vector register: a lane mask would be merged behind every uniform branch)
        int bad_v = 0;
        int Dmin_v = Dmin;                              // (the step's add-with-carry takes its carry from a scalar pair already)
        if constexpr (kWalk) asm volatile("" : "+v"(bad_v), "+v"(Dmin_v));
        auto prepare_walk = [&](auto clampc, int round, const ChipWalk& w_in, ChipBlock<NT>& b) {
            constexpr bool kClamp = decltype(clampc)::value;
            const int idx = round * stride + lane;
            bool inside = true;
            ChipWalk w = w_in;
            if constexpr (kClamp) {
                inside = idx <= last_idx;
                w = chip_walk_clamp(w_in, inside, chip_walk_at((uint64_t)(Ufx + (int64_t)(q0 + last_idx) * Tfx + (int64_t)two32)));
            }
            bool dn, ds[NT], near;
            chip_walk_flags<NT, KI>(w.f, T_lo, delta_lo, dn, ds, near);
            // (KS, three taps: one select serves E and L, and a block where they switch on different samples flags the epoch.
            // Their carries are two masks and the difference a scalar instruction: such a block takes the exact path, which
            // finds the same and says so)
            if constexpr (KS != 0 && NT == 3) near = near || ds[0] != ds[2];
            b.f = w.f;
            b.slow = 0;
            uint32_t off;                               // of the block's first sample in the epoch, bytes
            if (__builtin_expect(__any(near), 0)) {
                // (the run-time-position forms' exact path, entered with the same predictions: E = hi(u + T), split = hi(u + delta) - S)
                int S = w.S;
                int E = S + M + (dn ? 1 : 0);
                int split[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    split[t] = 0;
                    if (t == A) continue;
                    if constexpr (KI != 0)
                        split[t] = J[t] == (t - A) * KI ? E - S : 0;
                    else
                        split[t] = m[t] + (ds[t] ? 1 : 0);
                }
                bool wrong = false;
                const int q = q0 + 1 + (inside ? idx : last_idx);
                S = chip_first_above_exact(S, (double)(q - 1), step[A], shift[A]);
                E = chip_first_above_exact(E, (double)q, step[A], shift[A]);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    if (t == A) continue;
                    const int p0 = q + J[t];
                    const int bt = chip_first_above_exact(S + split[t], (double)p0, step[t], shift[t]);
                    double y = (double)S * step[t];
                    y = y + shift[t];
                    const int at_s = (int)ceil(y);
                    wrong = wrong || (at_s != p0 && at_s != p0 + 1) || (at_s == p0 + 1 && bt > S);
                    split[t] = bt < S ? 0 : bt - S;
                }
                const int nn = E - S;
                b.dn = nn - M;
                wrong = wrong || (unsigned)b.dn > 1u;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    b.ds[t] = 0;
                    if (t == A) continue;
                    const int sp = split[t] > nn ? nn : split[t];
                    if constexpr (KI != 0) {
                        wrong = wrong || !(J[t] == (t - A) * KI ? sp == nn : sp == 0);
                        continue;
                    }
                    b.ds[t] = sp - m[t];
                    wrong = wrong || (unsigned)b.ds[t] > 1u;
                }
                if constexpr (KS != 0 && NT == 3) wrong = wrong || b.ds[0] != b.ds[2];
                bad_v |= wrong ? 1 : 0;
                b.adj = S - w.S;
                b.slow = 1;
                off = (uint32_t)S << 1;
            } else {
                off = (uint32_t)w.S << 1;               // (the shift is the copy: S itself stays with the walk)
            }
            // (opaque: knowing it zero on one side, the compiler lays out a second copy of everything that asks for it)
            asm volatile("" : "+s"(b.slow));
            // 13 dwords = 26 samples from the (2-byte aligned) address of sample S: gfx950 serves unaligned dword loads.  A
            // 32-bit offset on the epoch's scalar base address: S >= 0, and an epoch is far shorter than 2^31 bytes.
            const char* src = ring_base + off;
            const uint4 w0 = *reinterpret_cast<const uint4*>(src);
            const uint4 w1 = *reinterpret_cast<const uint4*>(src + 16);
            const uint4 w2 = *reinterpret_cast<const uint4*>(src + 32);
            const uint32_t w3 = *reinterpret_cast<const uint32_t*>(src + 48);
            b.raw[0] = w0.x, b.raw[1] = w0.y, b.raw[2] = w0.z, b.raw[3] = w0.w;
            b.raw[4] = w1.x, b.raw[5] = w1.y, b.raw[6] = w1.z, b.raw[7] = w1.w;
            b.raw[8] = w2.x, b.raw[9] = w2.y, b.raw[10] = w2.z, b.raw[11] = w2.w;
            b.raw[12] = w3;
        };

        ChipBlock<NT> blk_a, blk_b;
        ChipWalk walk = chip_walk_at(u_cur);
        if constexpr (kWalk) {
            prepare_walk(std::true_type{}, 0, walk, blk_a);
            const ChipWalk w0 = chip_walk_clamp(walk, lane <= last_idx, chip_walk_at((uint64_t)(Ufx + (int64_t)(q0 + last_idx) * Tfx + (int64_t)two32)));
            blk_a.S = w0.S + (blk_a.slow ? blk_a.adj : 0);
        } else {
            prepare(0, u_cur, blk_a);
        }
        // carrier phase at the lane's first block: one exact evaluation; later blocks by a fixed rotation
        double sb, cb;
        // (folded forms: at the centre of the first half's run, which the block's sums are referred to)
        constexpr double kRefSample = kFold ? 0.5 * (double)(kFoldN0 - 1) : 0.0;
        if constexpr (kFold)
            sincos_reduced(__builtin_fma(-((double)blk_a.S + kRefSample), dphi_u, rem_carrier_u), &sb, &cb);
        else
            sincos_reduced(__builtin_fma(-(double)blk_a.S, dphi_u, rem_carrier_u), &sb, &cb);
        if constexpr (!kStatic) {
            sb = lane <= last_idx ? sb : 0.0;
            cb = lane <= last_idx ? cb : 0.0;
        }
        // per-lane LDS addresses: the strip slots of each tap's position m_t, and the lane's replica entry
        const int q_lane = q0 + 1 + lane + SDR_LUT_PAD;
        // (KS / KI) the lane's own strip slots are not used for running sums: eight zero words stand in for the replica of a
        // lane that has no block in a round (the last one)
        const uint32_t* zero_lq = reinterpret_cast<const uint32_t*>(strip) + 3;   // (words 1 .. 5 serve entries -2 .. +2)
        if constexpr (kStatic) strip[0] = strip[1] = make_double2(0.0, 0.0);

        sdr_u32x2 zI = {0u, 0u}, zQ = {0u, 0u};     // (biased conversion) the two register pairs the samples are built in
        asm volatile("" : "+v"(zI), "+v"(zQ));
        // (straight-line forms: a second set, for the odd samples.  v_perm_b32 rewrites the high word of a pair the v_fmac_f64
        // just in front of it has read, and the hazard recognizer puts an s_nop between the two -- one per sample; with the
        // pairs alternating, the pair that is rewritten was last read two samples ago and the pads are gone)
        sdr_u32x2 zI2 = {0u, 0u}, zQ2 = {0u, 0u};
        if constexpr (kWalk || kFold) asm volatile("" : "+v"(zI2), "+v"(zQ2));
        // (folded forms: the differences of a pair beside its sums -- zI / zQ and zI2 / zQ2 hold the sums, and the single
        // samples in between -- and the high word of 8192.0 the byte sums are added onto)
        sdr_u32x2 zDI = {0u, 0u}, zDQ = {0u, 0u}, zDI2 = {0u, 0u}, zDQ2 = {0u, 0u};
        uint32_t hi_fold = 0x40C00000u;
        if constexpr (kFold) asm volatile("" : "+v"(zDI), "+v"(zDQ), "+v"(zDI2), "+v"(zDQ2), "+v"(hi_fold));

        // (straight-line forms: the biased conversion's high-word constant, a vector register for the whole epoch -- v_perm_b32
        // takes one scalar operand, the selector; made opaque per block it was a move per block)
        uint32_t hi_epoch = 0x40B00000u;
        if constexpr ((kWalk || kFold) && SDR_BIASED_CVT) asm volatile("" : "+v"(hi_epoch));
        auto process = [&](const ChipBlock<NT>& b, int round, double sbk, double cbk, auto clampc) {
            constexpr bool kClamp = decltype(clampc)::value;   // (straight-line forms) the round may be the epoch's last one
            double pr = 0.0, pi = 0.0;
            double2* wp = strip;
            // the event positions as ONE scalar register, re-read per block: left to itself the compiler hoists the 27
            // bit tests out of the round loop as 27 lane masks and spills them through v_writelane / v_readlane
            unsigned evm = evmask;
            int klast = k_last;
            if constexpr (!kStatic) asm volatile("" : "+s"(evm), "+s"(klast));
            // the in-block rotations come from LDS as broadcasts, fetched a few samples ahead of their use (the
            // uniform branches below end a basic block: nothing is hoisted across them for us)
            constexpr int kAhead = 4;
            double2 rr[kChipMax + kAhead];
            if constexpr (!kStatic) {
#pragma unroll
                for (int k = 0; k < kAhead; ++k) rr[k] = rot[k];
            }
            auto park = [&]() {                         // P_k -> the lane's next strip slot
                *wp = make_double2(pr, pi);
                ++wp;
                asm volatile("" ::: "memory");
            };
            uint32_t hi_rt = 0x40B00000u;                 // (run-time-position forms: the biased conversion's high-word constant)
            // ... and its four byte selectors as scalar registers for the whole block: left as literals each costs the scalar
            // pipe a move in front of EVERY v_perm_b32 (two per sample: measured, + 41 % scalar instructions in the dense
            // closed-loop kernel and no gain from 6 % fewer vector ones)
            uint32_t sel_rt[4] = {cvt_selector(0), cvt_selector(1), cvt_selector(2), cvt_selector(3)};
            if constexpr (!kStatic && SDR_BIASED_CVT) {
                asm volatile("" : "+v"(hi_rt));
                asm volatile("" : "+s"(sel_rt[0]), "+s"(sel_rt[1]), "+s"(sel_rt[2]), "+s"(sel_rt[3]));
            }
            auto sample = [&](auto kc) {
                constexpr int k = decltype(kc)::value;
                double ar, ai;
                if constexpr (SDR_BIASED_CVT) {
                    ar = biased_sample(zI, b.raw[k >> 1], sel_rt[(k & 1) ? 2 : 0], hi_rt);
                    ai = biased_sample(zQ, b.raw[k >> 1], sel_rt[(k & 1) ? 3 : 1], hi_rt);
                } else {
                    const int w = ci8_native((int)b.raw[k >> 1]);
                    ar = (k & 1) ? (double)(int)(int8_t)(w >> 16) : (double)(int)(int8_t)w;
                    ai = (k & 1) ? (double)(w >> 24) : (double)(int)(int8_t)(w >> 8);
                }
                if (k + kAhead < kChipMax) rr[k + kAhead] = rot[k + kAhead];
                const double2 r = rr[k];
                pr = __builtin_fma(-ai, r.y, __builtin_fma(ar, r.x, pr));
                pi = __builtin_fma(ai, r.x, __builtin_fma(ar, r.y, pi));
                if constexpr (SDR_BIASED_CVT) asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI), "+v"(zQ));   // (see the straight-line loop below)
            };
            double hr = 0.0, hi = 0.0;                    // (straight-line forms) the first half's sum
            if constexpr (kStatic) {
                static_assert(2 * kHalf >= KM + 1 && kHalf < KM, "two halves of at most KS + 1 samples cover the block");
                // The block is summed in two halves, each from rotation 0 (folded forms: about its own centre); the second one is
                // turned onto the first where the block's sum is formed.  KS: the first half is the tap's part of the block in
                // front of its switch -- samples 0 .. KS - 1 and, where the lane's switch comes a sample late, KS -- and the second
                // half everything behind it: sample KS where the first half left it, KS + 1 .. KM - 1, and KM where the lane's block
                // is M + 1 long.  KI: samples 0 .. kHalf - 1, then kHalf .. KM - 1 and KM likewise.  An optional sample is MASKED,
                // not selected: the lane's flag picks the sample's raw dword or 0x80808080 (x = 0), so a lane without the sample
                // sums the conversion's offset times the sample's rotation, the same amount in every lane -- and each half starts
                // from minus the offsets' share of ALL its samples (sh1 / sh2).  Two sums per block, no captures, no 64-bit selects.
                static_assert(!SDR_BIASED_CVT || (2 * kHalf - KM >= 1 && 2 * kHalf - KM <= 2 && (KS == 0 || KS == kHalf - 1)),
                              "the offset's shares are kept for sums of KM - kHalf, + 1 and + 2 samples: kHalf must be one of the last two");
                static_assert(KS == 0 || NT == 3, "one switch flag serves the taps either side of the anchor");
                uint32_t flipped[kChipRawDwords];
                uint32_t hi_const = hi_epoch;
                if constexpr (SDR_BIASED_CVT) {
                    if constexpr (!kWalk && !kFold) asm volatile("" : "+v"(hi_const));   // (v_perm_b32 takes one scalar operand: the selector)
                }
#pragma unroll
                for (int i = 0; i < kChipRawDwords; ++i) flipped[i] = b.raw[i];   // (the ring holds the flipped bytes)
                // The masked copies (copies: a dword's other sample belongs to the other half).  The flags are the carries of the
                // block's fraction, taken HERE: a flag made when the block was prepared is a lane mask in a scalar register pair
                // for the length of a block, two blocks in flight, beside the 52 scalar registers of the rotations -- which then
                // spill through v_readlane.  A block that went through the exact re-evaluation brings its flags as integers.
                constexpr uint32_t kNoSample = kCi8Flip;   // (two samples of 0 + 0j as the ring holds them)
                constexpr int kWordS = (kHalf - 1) >> 1, kWordM = KM >> 1;
                bool dnf = false, swf = false;
                if constexpr (kWalk) {
                    if (__builtin_expect(b.slow != 0, 0)) {
                        dnf = b.dn != 0;
                        if constexpr (KS != 0) swf = b.ds[0] != 0;
                        asm volatile("");                       // (stays a branch: as selects, both sides would be paid in every block)
                    } else {
                        uint32_t f = b.f, fsum;
                        asm volatile("" : "+v"(f));
                        dnf = chip_carry(f, T_lo, fsum);
                        if constexpr (KS != 0) swf = chip_carry(f, delta_lo[0], fsum);
                    }
                } else {
                    dnf = b.dn != 0;
                }
                // sample KM, and sample KS for the first half / for the second
                const uint32_t w_last = dnf ? flipped[kWordM] : kNoSample;
                const uint32_t w_first = swf ? flipped[kWordS] : kNoSample, w_rest = swf ? kNoSample : flipped[kWordS];
                if constexpr (kFold) {
                    // Each half: the centre sample of an odd run starts the sum, then the pairs from the outside in, then the
                    // optional samples.  `seq` counts these steps through the block: odd steps build their doubles in the
                    // second register set (see SDR_ALT_PAIRS: a high word is rewritten two steps after it was last read).
                    auto single = [&](auto highc, auto seqc, uint32_t w, bool start, double rc, double rs, double shr, double shi) {
                        constexpr bool high = decltype(highc)::value != 0;     // the dword's second sample
                        constexpr bool alt = SDR_ALT_PAIRS && (decltype(seqc)::value & 1);
                        const double ar = biased_sample(alt ? zI2 : zI, w, cvt_selector(high ? 2 : 0), hi_const);
                        const double ai = biased_sample(alt ? zQ2 : zQ, w, cvt_selector(high ? 3 : 1), hi_const);
                        if (start) {
                            pr = ar - shr, pi = ai - shi;
                        } else {
                            pr = __builtin_fma(-ai, rs, __builtin_fma(ar, rc, pr));
                            pi = __builtin_fma(ai, rc, __builtin_fma(ar, rs, pi));
                        }
                        if constexpr (alt) asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI2), "+v"(zQ2));
                        else asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI), "+v"(zQ));
                    };
                    auto pair = [&](auto highac, auto highbc, auto seqc, uint32_t wa, uint32_t wb, bool start, double c, double sn, double shr, double shi) {
                        constexpr bool alt = SDR_ALT_PAIRS && (decltype(seqc)::value & 1);
                        // G = [aI aQ bI bQ], lowest byte first (selector bytes 4 .. 7: the first operand, 0 .. 3: the second)
                        constexpr uint32_t ia = 4u + 2u * (decltype(highac)::value & 1), ib = 2u * (decltype(highbc)::value & 1);
                        const uint32_t g = __builtin_amdgcn_perm(wa, wb, ((ib + 1u) << 24) | (ib << 16) | ((ia + 1u) << 8) | ia);
                        const uint32_t g2 = g ^ 0xFFFF0000u;
                        sdr_u32x2& SI = alt ? zI2 : zI;
                        sdr_u32x2& SQ = alt ? zQ2 : zQ;
                        sdr_u32x2& DI = alt ? zDI2 : zDI;
                        sdr_u32x2& DQ = alt ? zDQ2 : zDQ;
                        SI.y = __builtin_amdgcn_udot4(g, 0x00800080u, hi_fold, false);
                        SQ.y = __builtin_amdgcn_udot4(g, 0x80008000u, hi_fold, false);
                        DI.y = __builtin_amdgcn_udot4(g2, 0x00800080u, hi_fold, false);
                        DQ.y = __builtin_amdgcn_udot4(g2, 0x80008000u, hi_fold, false);
                        const double si = __builtin_bit_cast(double, SI), sq = __builtin_bit_cast(double, SQ);
                        const double di = __builtin_bit_cast(double, DI), dq = __builtin_bit_cast(double, DQ);
                        if (start) {
                            pr = __builtin_fma(-sn, dq, __builtin_fma(c, si, -shr));
                            pi = __builtin_fma(sn, di, __builtin_fma(c, sq, -shi));
                        } else {
                            pr = __builtin_fma(-sn, dq, __builtin_fma(c, si, pr));
                            pi = __builtin_fma(sn, di, __builtin_fma(c, sq, pi));
                        }
                        if constexpr (alt) asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI2), "+v"(zQ2), "+v"(zDI2), "+v"(zDQ2));
                        else asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI), "+v"(zQ), "+v"(zDI), "+v"(zDQ));
                    };
                    static_for<0, 2>([&](auto hc) {
                        constexpr int h = decltype(hc)::value;
                        constexpr int first = chip_fold_first(kHalf, h), count = h == 0 ? kFoldN0 : kFoldN1;
                        constexpr int odd = count & 1;
                        constexpr int seq0 = h == 0 ? 0 : (kFoldN0 & 1) + kFoldN0 / 2 + (KS != 0 ? 1 : 0);
                        constexpr int last = first + count;                            // the half's optional last sample
                        const double shr = h == 0 ? sh1c : sh2c, shi = h == 0 ? sh1s : sh2s;
                        if constexpr (odd)
                            single(std::integral_constant<int, (first + count / 2) & 1>{}, std::integral_constant<int, seq0>{},
                                   flipped[(first + count / 2) >> 1], true, 1.0, 0.0, shr, shi);
                        static_for<0, count / 2>([&](auto ic) {
                            constexpr int i = decltype(ic)::value;
                            constexpr int ka = first + i, kb = first + count - 1 - i;
                            pair(std::integral_constant<int, ka & 1>{}, std::integral_constant<int, kb & 1>{}, std::integral_constant<int, seq0 + odd + i>{},
                                 flipped[ka >> 1], flipped[kb >> 1], !odd && i == 0, fpc[h][i], fps[h][i], shr, shi);
                        });
                        constexpr auto seql = std::integral_constant<int, seq0 + odd + count / 2>{};
                        if constexpr (h == 0) {
                            if constexpr (KS != 0) single(std::integral_constant<int, last & 1>{}, seql, w_first, false, fsc[0], fss[0], 0.0, 0.0);
                            hr = pr, hi = pi;
                        } else if constexpr (KS != 0) {
                            // (samples KS and KM lie (count + 1) / 2 either side of the second half's centre: one more pair)
                            pair(std::integral_constant<int, (kHalf - 1) & 1>{}, std::integral_constant<int, last & 1>{}, seql, w_rest, w_last, false,
                                 fsc[1], -fss[1], 0.0, 0.0);
                        } else {
                            single(std::integral_constant<int, last & 1>{}, seql, w_last, false, fsc[1], fss[1], 0.0, 0.0);
                        }
                    });
                } else {
                    // mode 0: the sum starts from this sample (rotation 1) and minus the share; 1: rotation 1; 2: rotation (rc, rs)
                    auto direct = [&](auto highc, auto seqc, uint32_t w, auto modec, double rc, double rs, double shr, double shi) {
                        constexpr bool high = decltype(highc)::value != 0;
                        constexpr int mode = decltype(modec)::value;
                        constexpr bool alt = kWalk && SDR_ALT_PAIRS && (decltype(seqc)::value & 1);
                        double ar, ai;
                        if constexpr (SDR_BIASED_CVT) {
                            ar = biased_sample(alt ? zI2 : zI, w, cvt_selector(high ? 2 : 0), hi_const);
                            ai = biased_sample(alt ? zQ2 : zQ, w, cvt_selector(high ? 3 : 1), hi_const);
                        } else {
                            const int wn = ci8_native((int)w);
                            ar = high ? (double)(int)(int8_t)(wn >> 16) : (double)(int)(int8_t)wn;
                            ai = high ? (double)(wn >> 24) : (double)(int)(int8_t)(wn >> 8);
                        }
                        if constexpr (mode == 0) {
                            pr = ar - shr, pi = ai - shi;
                        } else if constexpr (mode == 1) {
                            pr = pr + ar, pi = pi + ai;
                        } else {
                            pr = __builtin_fma(-ai, rs, __builtin_fma(ar, rc, pr));
                            pi = __builtin_fma(ai, rc, __builtin_fma(ar, rs, pi));
                        }
                        // (an opaque point per sample: the sums must have read the pairs before their high words are written
                        // again, and the next sample must be built on THESE registers -- seen through, every sample would be
                        // rebuilt from the original pair, i.e. from a copy of its low word)
                        if constexpr (SDR_BIASED_CVT) {
                            if constexpr (alt) asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI2), "+v"(zQ2));
                            else asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI), "+v"(zQ));
                        }
                    };
                    constexpr int kExtra = KS != 0 ? 1 : 0;       // (KS: sample KS is summed once per half)
                    static_for<0, kHalf>([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        const uint32_t w = KS != 0 && k == kHalf - 1 ? w_first : flipped[k >> 1];
                        direct(std::integral_constant<int, k & 1>{}, kc, w, std::integral_constant<int, k == 0 ? 0 : 2>{}, k == 0 ? 1.0 : urc[k], k == 0 ? 0.0 : urs[k], sh1c, sh1s);
                    });
                    hr = pr, hi = pi;
                    if constexpr (KS != 0) {
                        // (one sample in front of the second half's rotation 0: the conjugate of one sample behind it)
                        pr = -sh2c, pi = -sh2s;
                        direct(std::integral_constant<int, (kHalf - 1) & 1>{}, std::integral_constant<int, kHalf>{}, w_rest, std::integral_constant<int, 2>{},
                               urc[1], -urs[1], 0.0, 0.0);
                    }
                    static_for<kHalf, KM + 1>([&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        constexpr int j = k - kHalf;
                        const uint32_t w = k == KM ? w_last : flipped[k >> 1];
                        direct(std::integral_constant<int, k & 1>{}, std::integral_constant<int, k + kExtra>{}, w,
                               std::integral_constant<int, j == 0 ? (KS != 0 ? 1 : 0) : 2>{}, j == 0 ? 1.0 : urc[j], j == 0 ? 0.0 : urs[j], sh2c, sh2s);
                    });
                }
            } else if constexpr (KM != 0) {
                // positions KM and KM + 1 are always events; the others (the taps' m_t, m_t + 1 < KM) are looked for
                // two samples at a time
                static_for<0, KM>([&](auto kc) {         // samples below KM: a tap's position may sit in front of any of them
                    constexpr int k = decltype(kc)::value;
                    if (evm & (1u << k)) park();
                    sample(kc);
                });
                park();                                  // P_KM
                sample(std::integral_constant<int, KM>{});
                park();                                  // P_(KM+1)
            } else {
#pragma unroll
                for (int k = 0; k <= kChipMax; ++k) {
                    if (evm & (1u << k)) {              // (wave-uniform) one of the positions somebody reads: park P_k
                        park();
                        if (k == klast) break;
                    }
                    if (k < kChipMax) {
                        double ar, ai;
                        if constexpr (SDR_BIASED_CVT) {
                            ar = biased_sample(zI, b.raw[k >> 1], sel_rt[(k & 1) ? 2 : 0], hi_rt);
                            ai = biased_sample(zQ, b.raw[k >> 1], sel_rt[(k & 1) ? 3 : 1], hi_rt);
                        } else {
                            const int w = ci8_native((int)b.raw[k >> 1]);
                            ar = (k & 1) ? (double)(int)(int8_t)(w >> 16) : (double)(int)(int8_t)w;
                            ai = (k & 1) ? (double)(w >> 24) : (double)(int)(int8_t)(w >> 8);
                        }
                        if (k + kAhead < kChipMax) rr[k + kAhead] = rot[k + kAhead];
                        const double2 r = rr[k];
                        pr = __builtin_fma(-ai, r.y, __builtin_fma(ar, r.x, pr));
                        pi = __builtin_fma(ai, r.x, __builtin_fma(ar, r.y, pi));
                        if constexpr (SDR_BIASED_CVT) asm volatile("" : "+v"(pr), "+v"(pi), "+v"(zI), "+v"(zQ));
                    }
                }
            }
            double2 ptot;
            if constexpr (kStatic) {
                // (the second half -- pr, pi -- onto the first)
                ptot.x = __builtin_fma(-pi, urs[kHalf], __builtin_fma(pr, urc[kHalf], hr));
                ptot.y = __builtin_fma(pi, urc[kHalf], __builtin_fma(pr, urs[kHalf], hi));
            } else {
                ptot = strip[rank[A] + b.dn];
                if constexpr (SDR_BIASED_CVT) {             // (P_M or P_(M+1): the offset's share of that many samples out)
                    const double2 bb = (rot + kChipMax)[M + b.dn];
                    ptot.x -= bb.x, ptot.y -= bb.y;
                }
            }
            const int first = round * stride;           // (a lane beyond the last whole chip re-does the last one)
            const uint32_t* lq;                         // replica entry of the block's anchor chip
            if constexpr (kStatic)                      // (... against three zero words: it adds nothing, whatever its phasor)
                lq = !kClamp || first + lane <= last_idx ? lut + q_lane + first : zero_lq;
            else
                lq = lut + q_lane + (first + lane <= last_idx ? first : last_idx - lane);
            if constexpr (KI != 0) {
                // every tap sees the whole block on one chip: turn the block's sum once, add it per tap
                const double xr = __builtin_fma(-sbk, ptot.y, cbk * ptot.x);
                const double xi = __builtin_fma(sbk, ptot.x, cbk * ptot.y);
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const double c = __hiloint2double((int)lq[(t - A) * KI], 0);
                    accr[t] = __builtin_fma(c, xr, accr[t]);
                    acci[t] = __builtin_fma(c, xi, acci[t]);
                }
                return;
            }
            if constexpr (kTurnOnce) {
                // E = c(q-1) ps + c(q) (ptot - ps), L = c(q) ps + c(q+1) (ptot - ps): with X = ph ptot, Y = ph ps
                //     P += c(q) X,    E' += (c(q-1) - c(q)) Y,    L' += (c(q) - c(q+1)) (Y - X),    E = E' + P,  L = L' + P
                // the block phasor turns two sums once instead of three tap shares (E' and L' are made whole behind the rounds)
                const double xr = __builtin_fma(-sbk, ptot.y, cbk * ptot.x), xi = __builtin_fma(sbk, ptot.x, cbk * ptot.y);
                const double yr = __builtin_fma(-sbk, hi, cbk * hr), yi = __builtin_fma(sbk, hr, cbk * hi);
                const double zr = yr - xr, zi = yi - xi;
                const double ce = __hiloint2double((int)lq[-1], 0), cp = __hiloint2double((int)lq[0], 0), cl = __hiloint2double((int)lq[1], 0);
                const double de = ce - cp, dl = cp - cl;
                accr[A] = __builtin_fma(cp, xr, accr[A]), acci[A] = __builtin_fma(cp, xi, acci[A]);
                accr[0] = __builtin_fma(de, yr, accr[0]), acci[0] = __builtin_fma(de, yi, acci[0]);
                accr[2] = __builtin_fma(dl, zr, accr[2]), acci[2] = __builtin_fma(dl, zi, acci[2]);
                return;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                double gr, gi;
                if (t == A) {
                    const double c = __hiloint2double((int)lq[0], 0);
                    gr = c * ptot.x;
                    gi = c * ptot.y;
                } else {
                    double2 ps;
                    if constexpr (kStatic)
                        ps = make_double2(hr, hi);          // (KS: the first half ends where the lane's taps switch)
                    else {
                        ps = strip[rank[t] + b.ds[t]];
                        if constexpr (SDR_BIASED_CVT) {
                            const double2 bb = (rot + kChipMax)[m[t] + b.ds[t]];
                            ps.x -= bb.x, ps.y -= bb.y;
                        }
                    }
                    const int jt = kStatic ? (t < A ? -1 : 0) : J[t];      // (KS: checked when the epoch was set up)
                    const double ca = __hiloint2double((int)lq[jt], 0);
                    const double cbn = __hiloint2double((int)lq[jt + 1], 0);
                    const double diff = ca - cbn;
                    gr = __builtin_fma(diff, ps.x, cbn * ptot.x);
                    gi = __builtin_fma(diff, ps.y, cbn * ptot.y);
                }
                accr[t] = __builtin_fma(-sbk, gi, __builtin_fma(cbk, gr, accr[t]));
                acci[t] = __builtin_fma(sbk, gr, __builtin_fma(cbk, gi, acci[t]));
            }
        };

        auto wave_has_work = [&](int round) { return SINGLE_WAVE || round * stride + (lane - wlane) <= last_idx; };
        // rotation to the next block of this lane
        auto advance = [&](const ChipBlock<NT>& from, const ChipBlock<NT>& to, int to_round) {
            const unsigned dd = (unsigned)(to.S - from.S - Dmin);
            const bool alive = to_round * stride + lane <= last_idx;
            bad = bad || (alive && dd > 1u);
            const double rc_ = dd ? rd1c : rd0c, rs_ = dd ? rd1s : rd0s;
            const double cbn = __builtin_fma(cb, rc_, -sb * rs_);
            const double sbn = __builtin_fma(sb, rc_, cb * rs_);
            if constexpr (kStatic) {
                cb = cbn, sb = sbn;                     // (a lane without a block correlates against zero replica words)
            } else {
                cb = alive ? cbn : 0.0;
                sb = alive ? sbn : 0.0;
            }
        };

        static_assert(SINGLE_WAVE || !kWalk, "the straight-line forms give a wave an epoch of its own");
        if constexpr (kWalk) {
            // The lane's next block and the rotation to it: dd is the carry of the walk's step.  A block that went through the
            // exact re-evaluation may start a sample off the line: next to one, dd comes from the integers as before.
            auto next_block = [&](auto clampc, const ChipBlock<NT>& from, ChipBlock<NT>& to, int to_round) {
                constexpr bool kClamp = decltype(clampc)::value;
                bool dd = chip_walk_step(walk, stride_lo, Dmin_v);
                prepare_walk(clampc, to_round, walk, to);
                if (__builtin_expect((from.slow | to.slow) != 0, 0)) {
                    bool alive = true;
                    // to.S - from.S - Dmin.  (Read back from the carry's lane mask: `dd ? 1 : 0` is the integer the walk's step adds,
                    // and the compiler forms it in front of the branch, one instruction in every block)
                    int d = (int)((__builtin_amdgcn_ballot_w64(dd) >> wlane) & 1u);
                    if constexpr (kClamp) {
                        // (a lane beyond the last whole chip: its block is the last chip's, wherever the walk went)
                        alive = to_round * stride + lane <= last_idx;
                        const int S_last = (int)((uint64_t)(Ufx + (int64_t)(q0 + last_idx) * Tfx + (int64_t)two32) >> 32);
                        d = alive ? d : S_last - (walk.S - d - Dmin_v) - Dmin_v;
                    }
                    if (to.slow) d += to.adj;
                    if (from.slow) d -= from.adj;
                    bad_v |= alive && (unsigned)d > 1u ? 1 : 0;
                    dd = d != 0;
                    asm volatile("");
                }
                const double rc_ = dd ? rd1c : rd0c, rs_ = dd ? rd1s : rd0s;
                const double cbn = __builtin_fma(cb, rc_, -sb * rs_);
                const double sbn = __builtin_fma(sb, rc_, cb * rs_);
                cb = cbn, sb = sbn;                     // (a lane without a block correlates against zero replica words)
                // (... done before the samples of the block at hand: floating down, the selects keep dd's mask for a block)
                asm volatile("" : "+v"(cb), "+v"(sb));
            };
            // (a block's taps are combined before the next block's samples begin: left to float behind them, the
            // combination holds the block's flags and four sums for the length of a block)
            auto settle = [&]() {
#pragma unroll
                for (int t = 0; t < NT; ++t) asm volatile("" : "+v"(accr[t]), "+v"(acci[t]));
            };
            auto round_pair = [&](auto clampc, int it) {
                const double sb0 = sb, cb0 = cb;
                next_block(clampc, blk_a, blk_b, 2 * it + 1);
                process(blk_a, 2 * it, sb0, cb0, clampc);
                settle();
                const double sb1 = sb, cb1 = cb;
                if (!decltype(clampc)::value || 2 * it + 2 < rounds) next_block(clampc, blk_b, blk_a, 2 * it + 2);
                process(blk_b, 2 * it + 1, sb1, cb1, clampc);
                settle();
            };
            // Rounds 0 .. rounds - 2 hold a block for every lane (r * stride + lane <= last_idx by construction): the pairs
            // that neither work on nor prepare the last round run without the clamp, `alive` and the zero replica words.
            const int plain = rounds >= 2 ? (rounds - 2) / 2 : 0;
            for (int it = 0; it < plain; ++it) round_pair(std::false_type{}, it);
            for (int it = plain; it < rounds / 2; ++it) round_pair(std::true_type{}, it);
            if (rounds & 1) process(blk_a, rounds - 1, sb, cb, std::true_type{});
            if constexpr (kTurnOnce) {              // E = E' + P, L = L' + P
                accr[0] += accr[A], acci[0] += acci[A];
                accr[2] += accr[A], acci[2] += acci[A];
            }
        } else {
            for (int it = 0; it < rounds / 2; ++it) {
                const double sb0 = sb, cb0 = cb;
                u_cur += (uint64_t)stride_fx;
                prepare(2 * it + 1, u_cur, blk_b);
                advance(blk_a, blk_b, 2 * it + 1);
                if (wave_has_work(2 * it)) process(blk_a, 2 * it, sb0, cb0, std::true_type{});
                const double sb1 = sb, cb1 = cb;
                if (2 * it + 2 < rounds) {
                    u_cur += (uint64_t)stride_fx;
                    prepare(2 * it + 2, u_cur, blk_a);
                    advance(blk_b, blk_a, 2 * it + 2);
                }
                if (wave_has_work(2 * it + 1)) process(blk_b, 2 * it + 1, sb1, cb1, std::true_type{});
            }
            if ((rounds & 1) && wave_has_work(rounds - 1)) process(blk_a, rounds - 1, sb, cb, std::true_type{});
        }
        bad = bad || bad_v != 0;
    }

    if (__any(bad)) return false;
    if (edge_lane >= 0) {
        if (head_end + (n - tail_start) > 64) {
            for (int off = 0; off < head_end + (n - tail_start); off += 64)
                edge_samples<SDR_FMT_CI8, NT>(ring, capacity, ep, dphi, shift, step, lut, edge_lane + off, head_end, tail_start, accr, acci, base);
        } else {
            edge_samples<SDR_FMT_CI8, NT>(ring, capacity, ep, dphi, shift, step, lut, edge_lane, head_end, tail_start, accr, acci, base);
        }
    }
    return true;
}

// True when the epoch can go through the chip-aligned routine: the code step in its range and no ring wrap within
// the epoch plus the slack the 56-byte windows may touch.
__device__ __forceinline__ bool chip_variant_applies(const EpochParams& ep, int64_t capacity) {
    return ep.code_step >= kChipMinCodeStep && ep.code_step <= kChipMaxCodeStep &&
           ep.start_sample % capacity + ep.n + 32 <= capacity;
}

}  // namespace sdr
