// Host-side dump of the folded half-block sums of the straight-line correlators (correlator_chip.h: ChipFold,
// chip_fold_constants) for tests/test_chip_fold.py: the plan's constants of one epoch, and blocks of sample bytes summed
// in the kernels' own order -- the v_perm_b32 gather, the complement of the b half, the four v_dot4_u32_u8 onto the high
// word of 8192.0, fp64 fma, the offsets' shares taken out where a sum is read -- with the instructions written out as
// integer arithmetic.  Built with `hipcc --cuda-host-only`: no device code, no GPU.
//   usage: chip_fold_dump <KM> <half> <ks 0|1> <carrier_hz> <fs> <random|rail> <n_blocks> <seed>
//     -> "const dphi=.. n0=.. n1=.. pc0_0=.. ps0_0=.. ... sc0= ss0= sc1= ss1= tc= ts= shc0= shs0= .. shc3= shs3="
//        then per block "b <hex of the 2 * (KM + 1) ring bytes> <first half before its last sample> <first half>
//        <block of KM samples> <block of KM + 1 samples>", each a pair re im (%.17g), about the first half's centre
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

struct Sums {
    double cr[3], ci[3], pr, pi;   // capr / capi and the running sum behind the block's last sample, shares taken out
};

static void fold_block(const uint32_t* raw, int KM, int half, bool ks, const ChipFold& f, Sums& out) {
    double pr = 0.0, pi = 0.0;
    auto single = [&](int k, bool start, double rc, double rs) {
        const double ar = from_high_word(perm(raw[k >> 1], 0x40B00000u, cvt_selector((k & 1) ? 2 : 0)));
        const double ai = from_high_word(perm(raw[k >> 1], 0x40B00000u, cvt_selector((k & 1) ? 3 : 1)));
        if (start) {
            pr = ar, pi = ai;
        } else {
            pr = fma(-ai, rs, fma(ar, rc, pr));
            pi = fma(ai, rc, fma(ar, rs, pi));
        }
    };
    auto pair = [&](int ka, int kb, bool start, double c, double sn) {
        const uint32_t ia = 4u + 2u * (ka & 1), ib = 2u * (kb & 1);
        const uint32_t g = perm(raw[ka >> 1], raw[kb >> 1], ((ib + 1u) << 24) | (ib << 16) | ((ia + 1u) << 8) | ia);
        const uint32_t g2 = g ^ 0xFFFF0000u;
        const double si = from_high_word(dot4(g, 0x00800080u, 0x40C00000u)), sq = from_high_word(dot4(g, 0x80008000u, 0x40C00000u));
        const double di = from_high_word(dot4(g2, 0x00800080u, 0x40C00000u)), dq = from_high_word(dot4(g2, 0x80008000u, 0x40C00000u));
        if (start) {
            pr = fma(-sn, dq, c * si);
            pi = fma(sn, di, c * sq);
        } else {
            pr = fma(-sn, dq, fma(c, si, pr));
            pi = fma(sn, di, fma(c, sq, pi));
        }
    };
    for (int h = 0; h < 2; ++h) {
        const int first = chip_fold_first(half, h), count = chip_fold_count(KM, half, ks, h), odd = count & 1;
        if (odd) single(first + count / 2, true, 1.0, 0.0);
        for (int i = 0; i < count / 2; ++i) pair(first + i, first + count - 1 - i, !odd && i == 0, f.pc[h][i], f.ps[h][i]);
        if (h == 0) {
            out.cr[0] = pr, out.ci[0] = pi;
            if (ks) single(first + count, false, f.sc[0], f.ss[0]);
            out.cr[2] = pr, out.ci[2] = pi;
        } else {
            out.cr[1] = pr, out.ci[1] = pi;
            single(first + count, false, f.sc[1], f.ss[1]);
        }
    }
    out.pr = pr - f.shc[3], out.pi = pi - f.shs[3];
    out.cr[1] -= f.shc[2], out.ci[1] -= f.shs[2];
    out.cr[2] -= f.shc[ks ? 1 : 0], out.ci[2] -= f.shs[ks ? 1 : 0];
    out.cr[0] -= f.shc[0], out.ci[0] -= f.shs[0];
}

int main(int argc, char** argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: chip_fold_dump <KM> <half> <ks> <carrier_hz> <fs> <random|rail> <n_blocks> <seed>\n");
        return 2;
    }
    const int KM = atoi(argv[1]), half = atoi(argv[2]);
    const bool ks = atoi(argv[3]) != 0;
    const double carrier = atof(argv[4]), fs = atof(argv[5]);
    const bool rail = strcmp(argv[6], "rail") == 0;
    const int n_blocks = atoi(argv[7]);
    uint64_t state = strtoull(argv[8], nullptr, 10) * 6364136223846793005ull + 1442695040888963407ull;
    if (KM < 1 || KM + 1 > kChipMax || half < 2 || half > kStaticHalf || half >= KM || 2 * half < KM + 1) return 2;
    const double dphi = carrier_step(carrier, fs);
    ChipFold f;
    chip_fold_constants(dphi, KM, half, ks, f);
    printf("const dphi=%.17g n0=%d n1=%d", dphi, chip_fold_count(KM, half, ks, 0), chip_fold_count(KM, half, ks, 1));
    for (int h = 0; h < 2; ++h)
        for (int i = 0; i < chip_fold_count(KM, half, ks, h) / 2; ++i) printf(" pc%d_%d=%.17g ps%d_%d=%.17g", h, i, f.pc[h][i], h, i, f.ps[h][i]);
    printf(" sc0=%.17g ss0=%.17g sc1=%.17g ss1=%.17g tc=%.17g ts=%.17g", f.sc[0], f.ss[0], f.sc[1], f.ss[1], f.tc, f.ts);
    for (int i = 0; i < 4; ++i) printf(" shc%d=%.17g shs%d=%.17g", i, f.shc[i], i, f.shs[i]);
    printf("\n");
    for (int b = 0; b < n_blocks; ++b) {
        uint8_t bytes[4 * kChipRawDwords] = {0};
        for (int i = 0; i < 2 * (KM + 1); ++i) {
            state = state * 6364136223846793005ull + 1442695040888963407ull;
            const uint32_t r = (uint32_t)(state >> 33);
            // (rail: every byte 0 or 255; the first two blocks all low and all high)
            bytes[i] = rail ? (b == 0 ? 0u : b == 1 ? 255u : ((r & 1u) ? 255u : 0u)) : (uint8_t)(r & 0xFFu);
        }
        uint32_t raw[kChipRawDwords];
        memcpy(raw, bytes, sizeof raw);   // (little endian, as the device reads the ring)
        Sums s;
        fold_block(raw, KM, half, ks, f, s);
        printf("b ");
        for (int i = 0; i < 2 * (KM + 1); ++i) printf("%02x", bytes[i]);
        printf(" %.17g %.17g %.17g %.17g", s.cr[0], s.ci[0], s.cr[2], s.ci[2]);
        for (int dn = 0; dn < 2; ++dn) {      // the block's sum as the kernels form it: the second half turned onto the first
            const double qr = dn ? s.pr : s.cr[1], qi = dn ? s.pi : s.ci[1];
            printf(" %.17g %.17g", fma(-qi, f.ts, fma(qr, f.tc, s.cr[2])), fma(qi, f.tc, fma(qr, f.ts, s.ci[2])));
        }
        printf("\n");
    }
    return 0;
}
