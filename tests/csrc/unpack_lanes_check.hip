// Host-side proof of the unpack kernels' lane arithmetic (sydr_amd/csrc/unpack_lanes.h): every byte value at every byte position
// of a granule, both field orders, all three widths, hostile tables (-128, 127, repeated levels, random ones) -- the granule
// path and the per-sample path against the per-field statement of the format in include/sydr_amd.h, written out here once more
// on its own.  Built with `hipcc --cuda-host-only`: the byte permute takes its plain-C++ stand-in, no device code, no GPU.
//   usage: unpack_lanes_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../sydr_amd/csrc/unpack_lanes.h"

using namespace sdr;

// value of field j of a slab, straight from the format's definition
static int8_t field_value(const uint8_t* slab, int j, int bits, bool msb, const int8_t* levels) {
    const int F = 8 / bits;
    const int p = j % F;
    const int shift = msb ? bits * (F - 1 - p) : bits * p;
    return levels[(slab[j / F] >> shift) & ((1 << bits) - 1)];
}

template <int BITS>
static long check_width(uint64_t& state) {
    auto next = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(state >> 33);
    };
    const int GB = 2 * BITS;                      // packed bytes of a granule
    long cases = 0;
    for (int table = 0; table < 6; ++table) {
        int8_t levels[16];
        for (int c = 0; c < 16; ++c) {
            switch (table) {
                case 0: levels[c] = (int8_t)(c % 2 ? -128 : 127); break;           // the extremes, repeated
                case 1: levels[c] = (int8_t)(c - 128); break;                      // -128 upwards
                case 2: levels[c] = (int8_t)(127 - c); break;                      // 127 downwards
                case 3: levels[c] = (int8_t)(c == 0 ? -128 : c == (1 << BITS) - 1 ? 127 : 0); break;
                default: levels[c] = (int8_t)next(); break;                        // anything
            }
        }
        const UnpackTable tab = unpack_table(levels, BITS);
        for (int msb = 0; msb < 2; ++msb)
            for (int pos = 0; pos < GB; ++pos)
                for (int v = 0; v < 256; ++v) {
                    uint8_t slab[8];
                    for (int b = 0; b < GB; ++b) slab[b] = (uint8_t)next();
                    slab[pos] = (uint8_t)v;
                    uint64_t packed = 0;
                    for (int b = 0; b < GB; ++b) packed |= (uint64_t)slab[b] << (8 * b);
                    uint32_t out[4];
                    unpack_granule<BITS>(packed, tab, msb != 0, out);
                    uint8_t got[16];
                    memcpy(got, out, 16);
                    for (int j = 0; j < 16; ++j) {
                        const uint8_t want = (uint8_t)field_value(slab, j, BITS, msb != 0, levels) ^ 0x80u;
                        const uint32_t pair = unpack_sample(slab, j / 2, BITS, msb != 0, tab);
                        const uint8_t plain = (uint8_t)(pair >> (8 * (j & 1)));
                        if (got[j] != want || plain != want) {
                            printf("mismatch: bits=%d msb=%d table=%d pos=%d value=%d field=%d granule=%02x sample=%02x want=%02x\n", BITS, msb, table,
                                   pos, v, j, got[j], plain, want);
                            return -1;
                        }
                    }
                    ++cases;
                }
    }
    return cases;
}

int main() {
    uint64_t state = 20260007;
    long total = 0;
    const long a = check_width<1>(state), b = check_width<2>(state), c = check_width<4>(state);
    if (a < 0 || b < 0 || c < 0) return 1;
    total = a + b + c;
    printf("ok %ld\n", total);
    return 0;
}
