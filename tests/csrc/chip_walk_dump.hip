// Host-side walk of the straight-line correlators' blocks (correlator_chip.h: ChipWalk, chip_walk_step, chip_walk_clamp,
// chip_walk_flags) over whole epochs, lane by lane and round by round as a wave does it, for tests/test_chip_walk.py to hold
// against the 64-bit formulation.  Built with `hipcc --cuda-host-only`: no device code, no GPU.
//   usage: chip_walk_dump <geometry> <n_items> <seed>      geometry: 25 | 20 | 50h
//            -> "item ..." per epoch, then "b <round> <lane> <S> <dn> <ds first tap> <ds last tap> <dd> <near> <inside>" per block
//          chip_walk_dump crafted
//            -> "c <f> <T_lo> <d0_lo> <d2_lo> <stride_lo> <dn> <ds0> <ds2> <near> <dd> <f after the step>" per combination
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

static uint64_t g_state;
static double uni() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

// view: 1 = the taps as they are, 2 = the half-chip view (rem_code, code_step and spacing doubled)
template <int NT, int KM, int KS, int KI>
static int walk_items(double fs, int view, const double* spacing_chips, int n_items) {
    constexpr int A = NT / 2;
    const int stride = 64;
    for (int i = 0; i < n_items; ++i) {
        const double step1 = (1.023e6 + (uni() * 12.0 - 6.0)) / fs;
        const double rem1 = i == 0 ? 0.0 : uni() * step1;
        const int n = (int)std::ceil((1023.0 - rem1) / step1) + (int)(uni() * 3.0) - 1;
        const double code_step = step1 * view, rem_code = rem1 * view;
        double shift[NT], step[NT], inv[NT];
        for (int t = 0; t < NT; ++t) {
            shift[t] = rem_code + spacing_chips[t] * view;
            double stop = code_step * (double)n;
            stop = stop + shift[t];
            step[t] = (stop - shift[t]) / (double)n;
            inv[t] = 1.0 / step[t];
        }
        ChipGeom<NT> g;
        chip_geometry<NT, KM, KS, KI>(n, shift, step, inv, g);
        const int64_t stride_fx = (int64_t)stride * g.Tfx;
        const int Dmin = (int)(stride_fx >> 32);
        printf("item n=%d rem_code=%.17g code_step=%.17g q0=%d F=%d Tfx=%lld Ufx=%lld d0=%llu d2=%llu m0=%d m2=%d Dmin=%d bad=%d\n", n, rem_code,
               code_step, g.q0, g.F, (long long)g.Tfx, (long long)g.Ufx, (unsigned long long)g.delta[0],
               (unsigned long long)g.delta[NT - 1], g.m[0], g.m[NT - 1], Dmin, g.bad);
        if (g.F <= 0) continue;
        const uint32_t T_lo = (uint32_t)g.Tfx, stride_lo = (uint32_t)stride_fx;
        uint32_t delta_lo[NT];
        for (int t = 0; t < NT; ++t) delta_lo[t] = (uint32_t)g.delta[t];
        const int rounds = (g.F + stride - 1) / stride, last_idx = g.F - 1;
        const ChipWalk w_last = chip_walk_at((uint64_t)(g.Ufx + (int64_t)(g.q0 + last_idx) * g.Tfx + ((int64_t)1 << 32)));
        for (int lane = 0; lane < stride; ++lane) {
            ChipWalk w = chip_walk_at((uint64_t)(g.Ufx + (int64_t)g.q0 * g.Tfx + ((int64_t)1 << 32)) + (uint64_t)((int64_t)lane * g.Tfx));
            for (int r = 0; r < rounds; ++r) {
                bool dd = false;
                if (r > 0) dd = chip_walk_step(w, stride_lo, Dmin);
                // (the kernels clamp only where the round may be the last one; clamping a lane that is inside changes nothing)
                const bool inside = r * stride + lane <= last_idx;
                const ChipWalk b = r == rounds - 1 ? chip_walk_clamp(w, inside, w_last) : w;
                bool dn, ds[NT], near;
                chip_walk_flags<NT, KI>(b.f, T_lo, delta_lo, dn, ds, near);
                printf("b %d %d %d %d %d %d %d %d %d\n", r, lane, b.S, dn ? 1 : 0, ds[0] ? 1 : 0, ds[NT - 1] ? 1 : 0, dd ? 1 : 0, near ? 1 : 0,
                       inside ? 1 : 0);
            }
        }
    }
    return 0;
}

static int crafted() {
    const uint32_t fs[] = {0u, 1u, 0xFFFFu, 0x10000u, 0x10001u, 0x7FFFFFFFu, 0x80000000u, 0xFFFEFFFFu, 0xFFFF0000u, 0xFFFF0001u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const uint32_t adds[] = {0u, 1u, 0xFFFFu, 0x10000u, 0x66666666u, 0x80000000u, 0xFFFEFFFFu, 0xFFFF0000u, 0xFFFFFFFFu};
    for (uint32_t f : fs)
        for (uint32_t T_lo : adds)
            for (uint32_t d0 : adds)
                for (uint32_t d2 : {d0, d0 + 3u, 0x33333333u}) {
                    const uint32_t delta_lo[3] = {d0, 0u, d2};
                    bool dn, ds[3], near;
                    chip_walk_flags<3, 0>(f, T_lo, delta_lo, dn, ds, near);
                    const uint32_t stride_lo = T_lo * 64u;
                    ChipWalk w{1000, f};
                    const bool dd = chip_walk_step(w, stride_lo, 1561);
                    if (w.S != 1000 + 1561 + (dd ? 1 : 0)) return 1;
                    printf("c %u %u %u %u %u %d %d %d %d %d %u\n", f, T_lo, d0, d2, stride_lo, dn ? 1 : 0, ds[0] ? 1 : 0, ds[2] ? 1 : 0, near ? 1 : 0,
                           dd ? 1 : 0, w.f);
                }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "crafted")) return crafted();
    if (argc < 4) return 2;
    const int n_items = atoi(argv[2]);
    g_state = strtoull(argv[3], nullptr, 10) * 6364136223846793005ull + 1442695040888963407ull;
    const double three[3] = {-0.5, 0.0, 0.5};
    const double five[5] = {-1.0, -0.5, 0.0, 0.5, 1.0};
    if (!strcmp(argv[1], "25")) return walk_items<3, 24, 12, 0>(25e6, 1, three, n_items);
    if (!strcmp(argv[1], "20")) return walk_items<3, 19, 9, 0>(20e6, 1, three, n_items);
    if (!strcmp(argv[1], "50h")) return walk_items<5, 24, 0, 1>(50e6, 2, five, n_items);
    return 2;
}
