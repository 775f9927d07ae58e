// Host-side dump of the half-block sums of the straight-line correlators with their optional samples MASKED
// (correlator_chip.h: chip_mask_shares and the kStatic sample loop of correlate_epoch_chip) for tests/test_chip_mask.py:
// blocks of sample bytes summed in the kernels' own order -- the lane's flag picks an optional sample's raw dword or
// 0x80808080, each half starts from minus the offsets' share of all its samples, nothing is captured on the way, the second
// half is turned onto the first -- with the instructions written out as integer arithmetic.  Folded forms: sample KS (taps
// switching inside the block) ends the first half as a single sample or joins sample KM in one more pair of the second
// half; direct forms: it is summed one step in front of the second half's rotation 0.
// Built with `hipcc --cuda-host-only`: no device code, no GPU.
//   usage: chip_mask_dump <KM> <half> <ks 0|1> <fold 0|1> <carrier_hz> <fs> <random|rail> <n_blocks> <seed>
//     -> "const dphi=.. ref=.. c1=.. s1=.. c2=.. s2=.."      (ref: the sample position the sums are referred to)
//        then per block "b <hex of the 2 * (KM + 1) ring bytes>" and, for sw in (0, 1) [ks only] and dn in (0, 1), in that
//        order, "<first half re im> <block re im>" (%.17g)
//   or: chip_mask_dump turn <n_blocks> <carrier_hz> <fs> <seed>
//     -> "direct <E re im> <P re im> <L re im>" and "turned <...>": n_blocks folded blocks of 24 / 25 samples with random
//        flags, random +-1 chips and a block phasor advanced by 64 chips per block, combined per tap (three phasor turns per
//        block) and as the three-tap forms do it (X = ph ptot, Y = ph ps: P += c(q) X, E' += (c(q-1) - c(q)) Y,
//        L' += (c(q) - c(q+1)) (Y - X), E = E' + P, L = L' + P)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sydr_amd/csrc/engine_internal.h"
#include "../../sydr_amd/csrc/correlator.h"
#include "../../sydr_amd/csrc/correlator_chip.h"

using namespace sdr;

// v_perm_b32: selector bytes 0 .. 3 take the second operand's bytes, 4 .. 7 the first's, 0x0C is a zero byte
static uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t both = ((uint64_t)s0 << 32) | s1;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = (sel >> (8 * i)) & 0xFFu;
        if (c > 7u && c != 0x0Cu) abort();
        const uint32_t byte = c == 0x0Cu ? 0u : (uint32_t)((both >> (8 * c)) & 0xFFu);
        out |= byte << (8 * i);
    }
    return out;
}
// v_dot4_u32_u8
static uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) {
    for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
    return c;
}
static double from_high_word(uint32_t hi) {
    const uint64_t bits = (uint64_t)hi << 32;
    double d;
    memcpy(&d, &bits, 8);
    return d;
}

constexpr uint32_t kNoSample = 0x80808080u;

struct Acc {
    double pr = 0.0, pi = 0.0;
    // mode 0: the sum starts from this sample and minus the share; 1: rotation 1; 2: rotation (rc, rs)
    void single(uint32_t w, int high, int mode, double rc, double rs, double shr, double shi) {
        const double ar = from_high_word(perm(w, 0x40B00000u, cvt_selector(high ? 2 : 0)));
        const double ai = from_high_word(perm(w, 0x40B00000u, cvt_selector(high ? 3 : 1)));
        if (mode == 0) {
            pr = ar - shr, pi = ai - shi;
        } else if (mode == 1) {
            pr = pr + ar, pi = pi + ai;
        } else {
            pr = fma(-ai, rs, fma(ar, rc, pr));
            pi = fma(ai, rc, fma(ar, rs, pi));
        }
    }
    void pair(uint32_t wa, int high_a, uint32_t wb, int high_b, bool start, double c, double sn, double shr, double shi) {
        const uint32_t ia = 4u + 2u * (uint32_t)high_a, ib = 2u * (uint32_t)high_b;
        const uint32_t g = perm(wa, wb, ((ib + 1u) << 24) | (ib << 16) | ((ia + 1u) << 8) | ia);
        const uint32_t g2 = g ^ 0xFFFF0000u;
        const double si = from_high_word(dot4(g, 0x00800080u, 0x40C00000u)), sq = from_high_word(dot4(g, 0x80008000u, 0x40C00000u));
        const double di = from_high_word(dot4(g2, 0x00800080u, 0x40C00000u)), dq = from_high_word(dot4(g2, 0x80008000u, 0x40C00000u));
        pr = fma(-sn, dq, fma(c, si, start ? -shr : pr));
        pi = fma(sn, di, fma(c, sq, start ? -shi : pi));
    }
};

struct Sums {
    double hr, hi, tr, ti;   // the first half, the block
};

static void masked_words(const uint32_t* raw, int KM, int half, bool ks, bool sw, bool dn, uint32_t& w_first, uint32_t& w_rest, uint32_t& w_last) {
    w_last = dn ? raw[KM >> 1] : kNoSample;
    w_first = ks && sw ? raw[(half - 1) >> 1] : kNoSample;
    w_rest = ks && !sw ? raw[(half - 1) >> 1] : kNoSample;
}

static Sums fold_block(const uint32_t* raw, int KM, int half, bool ks, bool sw, bool dn, const ChipFold& f, const ChipShares& sh) {
    uint32_t w_first, w_rest, w_last;
    masked_words(raw, KM, half, ks, sw, dn, w_first, w_rest, w_last);
    Acc a;
    Sums out{};
    for (int h = 0; h < 2; ++h) {
        const int first = chip_fold_first(half, h), count = chip_fold_count(KM, half, ks, h), odd = count & 1, last = first + count;
        const double shr = h == 0 ? sh.c1 : sh.c2, shi = h == 0 ? sh.s1 : sh.s2;
        if (odd) a.single(raw[(first + count / 2) >> 1], (first + count / 2) & 1, 0, 1.0, 0.0, shr, shi);
        for (int i = 0; i < count / 2; ++i) {
            const int ka = first + i, kb = first + count - 1 - i;
            a.pair(raw[ka >> 1], ka & 1, raw[kb >> 1], kb & 1, !odd && i == 0, f.pc[h][i], f.ps[h][i], shr, shi);
        }
        if (h == 0) {
            if (ks) a.single(w_first, last & 1, 2, f.sc[0], f.ss[0], 0.0, 0.0);
            out.hr = a.pr, out.hi = a.pi;
        } else if (ks) {
            a.pair(w_rest, (half - 1) & 1, w_last, last & 1, false, f.sc[1], -f.ss[1], 0.0, 0.0);
        } else {
            a.single(w_last, last & 1, 2, f.sc[1], f.ss[1], 0.0, 0.0);
        }
    }
    out.tr = fma(-a.pi, f.ts, fma(a.pr, f.tc, out.hr));
    out.ti = fma(a.pi, f.tc, fma(a.pr, f.ts, out.hi));
    return out;
}

static Sums direct_block(const uint32_t* raw, int KM, int half, bool ks, bool sw, bool dn, const ChipRot& r, const ChipShares& sh) {
    uint32_t w_first, w_rest, w_last;
    masked_words(raw, KM, half, ks, sw, dn, w_first, w_rest, w_last);
    Acc a;
    Sums out{};
    for (int k = 0; k < half; ++k)
        a.single(ks && k == half - 1 ? w_first : raw[k >> 1], k & 1, k == 0 ? 0 : 2, r.urc[k], r.urs[k], sh.c1, sh.s1);
    out.hr = a.pr, out.hi = a.pi;
    if (ks) {
        a.pr = -sh.c2, a.pi = -sh.s2;
        a.single(w_rest, (half - 1) & 1, 2, r.urc[1], -r.urs[1], 0.0, 0.0);
    }
    for (int k = half; k <= KM; ++k) {
        const int j = k - half;
        a.single(k == KM ? w_last : raw[k >> 1], k & 1, j == 0 ? (ks ? 1 : 0) : 2, r.urc[j], r.urs[j], sh.c2, sh.s2);
    }
    out.tr = fma(-a.pi, r.urs[half], fma(a.pr, r.urc[half], out.hr));
    out.ti = fma(a.pi, r.urc[half], fma(a.pr, r.urs[half], out.hi));
    return out;
}

static int turn_mode(int argc, char** argv) {
    if (argc != 6) return 2;
    const int n_blocks = atoi(argv[2]), KM = 24, half = 13;
    const double dphi = carrier_step(atof(argv[3]), atof(argv[4]));
    uint64_t state = strtoull(argv[5], nullptr, 10) * 6364136223846793005ull + 1442695040888963407ull;
    auto next = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(state >> 33);
    };
    ChipFold f{};
    chip_fold_constants(dphi, KM, half, true, f);
    const ChipShares sh = chip_mask_shares(f, true);
    double dr[3] = {0, 0, 0}, di[3] = {0, 0, 0}, tr[3] = {0, 0, 0}, ti[3] = {0, 0, 0};
    for (int b = 0; b < n_blocks; ++b) {
        uint8_t bytes[4 * kChipRawDwords] = {0};
        for (int i = 0; i < 2 * (KM + 1); ++i) bytes[i] = (uint8_t)(next() & 0xFFu);
        uint32_t raw[kChipRawDwords];
        memcpy(raw, bytes, sizeof raw);
        const Sums s = fold_block(raw, KM, half, true, (next() & 1u) != 0, (next() & 1u) != 0, f, sh);
        double sb, cb;
        sincos_reduced(-(double)b * 1564.0 * dphi + 0.3, &sb, &cb);
        const double c[3] = {(next() & 1u) ? 1.0 : -1.0, (next() & 1u) ? 1.0 : -1.0, (next() & 1u) ? 1.0 : -1.0};   // c(q-1), c(q), c(q+1)
        // per tap, as the forms with run-time positions and the five-tap ones combine: g = c_after ptot + (c_before - c_after) ps
        for (int t = 0; t < 3; ++t) {
            double gr, gi;
            if (t == 1) {
                gr = c[1] * s.tr, gi = c[1] * s.ti;
            } else {
                const double ca = c[t == 0 ? 0 : 1], cbn = c[t == 0 ? 1 : 2], diff = ca - cbn;
                gr = fma(diff, s.hr, cbn * s.tr), gi = fma(diff, s.hi, cbn * s.ti);
            }
            dr[t] = fma(-sb, gi, fma(cb, gr, dr[t]));
            di[t] = fma(sb, gr, fma(cb, gi, di[t]));
        }
        const double xr = fma(-sb, s.ti, cb * s.tr), xi = fma(sb, s.tr, cb * s.ti);
        const double yr = fma(-sb, s.hi, cb * s.hr), yi = fma(sb, s.hr, cb * s.hi);
        const double zr = yr - xr, zi = yi - xi, de = c[0] - c[1], dl = c[1] - c[2];
        tr[1] = fma(c[1], xr, tr[1]), ti[1] = fma(c[1], xi, ti[1]);
        tr[0] = fma(de, yr, tr[0]), ti[0] = fma(de, yi, ti[0]);
        tr[2] = fma(dl, zr, tr[2]), ti[2] = fma(dl, zi, ti[2]);
    }
    tr[0] += tr[1], ti[0] += ti[1];
    tr[2] += tr[1], ti[2] += ti[1];
    printf("direct %.17g %.17g %.17g %.17g %.17g %.17g\n", dr[0], di[0], dr[1], di[1], dr[2], di[2]);
    printf("turned %.17g %.17g %.17g %.17g %.17g %.17g\n", tr[0], ti[0], tr[1], ti[1], tr[2], ti[2]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "turn") == 0) return turn_mode(argc, argv);
    if (argc != 10) {
        fprintf(stderr, "usage: chip_mask_dump <KM> <half> <ks> <fold> <carrier_hz> <fs> <random|rail> <n_blocks> <seed>\n");
        return 2;
    }
    const int KM = atoi(argv[1]), half = atoi(argv[2]);
    const bool ks = atoi(argv[3]) != 0, fold = atoi(argv[4]) != 0;
    const double carrier = atof(argv[5]), fs = atof(argv[6]);
    const bool rail = strcmp(argv[7], "rail") == 0;
    const int n_blocks = atoi(argv[8]);
    uint64_t state = strtoull(argv[9], nullptr, 10) * 6364136223846793005ull + 1442695040888963407ull;
    if (KM < 1 || KM + 1 > kChipMax || half < 2 || half > kStaticHalf || half >= KM || 2 * half < KM + 1 || 2 * half > KM + 2) return 2;
    const double dphi = carrier_step(carrier, fs);
    ChipFold f{};
    ChipRot r{};
    ChipShares sh;
    double ref = 0.0;
    if (fold) {
        chip_fold_constants(dphi, KM, half, ks, f);
        sh = chip_mask_shares(f, ks);
        ref = 0.5 * (double)(chip_fold_count(KM, half, ks, 0) - 1);
    } else {
        chip_rotations(dphi, 1, r, half, KM - half);
        sh = chip_mask_shares(r, KM, half, ks);
    }
    printf("const dphi=%.17g ref=%.17g c1=%.17g s1=%.17g c2=%.17g s2=%.17g\n", dphi, ref, sh.c1, sh.s1, sh.c2, sh.s2);
    for (int b = 0; b < n_blocks; ++b) {
        uint8_t bytes[4 * kChipRawDwords] = {0};
        for (int i = 0; i < 2 * (KM + 1); ++i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t rnd = (uint32_t)(state >> 33);
            // (rail: every byte 0 or 255; the first two blocks all low and all high)
            bytes[i] = rail ? (b == 0 ? 0u : b == 1 ? 255u : ((rnd & 1u) ? 255u : 0u)) : (uint8_t)(rnd & 0xFFu);
        }
        uint32_t raw[kChipRawDwords];
        memcpy(raw, bytes, sizeof raw);   // (little endian, as the device reads the ring)
        printf("b ");
        for (int i = 0; i < 2 * (KM + 1); ++i) printf("%02x", bytes[i]);
        for (int sw = 0; sw < (ks ? 2 : 1); ++sw)
            for (int dn = 0; dn < 2; ++dn) {
                const Sums s = fold ? fold_block(raw, KM, half, ks, sw != 0, dn != 0, f, sh) : direct_block(raw, KM, half, ks, sw != 0, dn != 0, r, sh);
                printf(" %.17g %.17g %.17g %.17g", s.hr, s.hi, s.tr, s.ti);
            }
        printf("\n");
    }
    return 0;
}
