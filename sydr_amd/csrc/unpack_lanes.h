// Packed 1-, 2- and 4-bit I,Q (include/sydr_amd.h, sdr_iq_packing) widened into the ci8 ring's bytes: what ONE lane of the
// unpack kernels (unpack.hip) does with the packed bytes of one 16-byte ring granule -- 8 samples = 16 fields, out of 2 / 4 / 8
// packed bytes.  Shared with the host (tests/csrc/unpack_lanes_check.hip runs it over every byte value, position, order and
// width against the per-field statement of the format), so the bit logic is proven before any device time is spent.
//
// The field codes of four consecutive fields are spread one per byte of a selector word, and a byte permute
// (v_perm_b32) looks the four levels up in one instruction: a table of four levels is one register; sixteen levels are two
// permutes over register pairs and a per-byte select on bit 3 of the code.  The table holds the levels as the ring wants
// them (sign bit flipped: engine_internal.h), made once per launch by unpack_table().
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDR_UNPACK_HD __host__ __device__ inline
#else
#define SDR_UNPACK_HD inline
#endif

namespace sdr {

struct UnpackTable {
    uint32_t t[4];      // byte i of t[j] = levels[4 * j + i] ^ 0x80
};

inline UnpackTable unpack_table(const int8_t* levels, int bits) {
    UnpackTable tab = {{0, 0, 0, 0}};
    for (int c = 0; c < (1 << bits); ++c) tab.t[c >> 2] |= (uint32_t)((uint8_t)levels[c] ^ 0x80u) << (8 * (c & 3));
    return tab;
}

// D.byte[i] = {hi, lo}.byte[sel.byte[i]], selector bytes 0..7 (the only ones used here): lo holds bytes 0..3, hi bytes 4..7.
SDR_UNPACK_HD uint32_t unpack_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) out |= (uint32_t)((both >> (8 * ((sel >> (8 * i)) & 7))) & 0xFF) << (8 * i);
    return out;
#endif
}

SDR_UNPACK_HD uint32_t unpack_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// The codes of four consecutive fields, one per selector byte (field order = byte order).
// 1 bit: the four fields of a nibble `n` (least significant field first).
SDR_UNPACK_HD uint32_t spread1(uint32_t n) { return (n | n << 7 | n << 14 | n << 21) & 0x01010101u; }
// 2 bits: the four fields of a byte `c`.
SDR_UNPACK_HD uint32_t spread2(uint32_t c) { return (c | c << 6 | c << 12 | c << 18) & 0x03030303u; }
// 4 bits: the four fields of two bytes `h` (little endian).
SDR_UNPACK_HD uint32_t spread4(uint32_t h) { return (h & 0xFu) | (h & 0xF0u) << 4 | (h & 0xF00u) << 8 | (h & 0xF000u) << 12; }

// One granule: `packed` = its 2 (1 bit), 4 (2 bits) or 8 (4 bits) packed bytes, little endian, the first byte lowest;
// out[4] = the 16 ring bytes.  msb: SDR_PACK_MSB_FIRST (the first field of a byte in its most significant bits).
template <int BITS>
SDR_UNPACK_HD void unpack_granule(uint64_t packed, const UnpackTable& tab, bool msb, uint32_t out[4]) {
    if (BITS == 1) {
        for (int b = 0; b < 2; ++b) {
            const uint32_t c = (uint32_t)(packed >> (8 * b)) & 0xFFu;
            // (most significant first: fields 0..3 are bits 7..4 -- the high nibble, its fields in reverse order)
            const uint32_t s0 = msb ? unpack_bswap(spread1(c >> 4)) : spread1(c & 15u);
            const uint32_t s1 = msb ? unpack_bswap(spread1(c & 15u)) : spread1(c >> 4);
            out[2 * b] = unpack_perm(0u, tab.t[0], s0);
            out[2 * b + 1] = unpack_perm(0u, tab.t[0], s1);
        }
    } else if (BITS == 2) {
        for (int b = 0; b < 4; ++b) {
            const uint32_t s = spread2((uint32_t)(packed >> (8 * b)) & 0xFFu);
            out[b] = unpack_perm(0u, tab.t[0], msb ? unpack_bswap(s) : s);
        }
    } else {
        for (int b = 0; b < 4; ++b) {
            uint32_t h = (uint32_t)(packed >> (16 * b)) & 0xFFFFu;
            if (msb) h = (h & 0x0F0Fu) << 4 | (h >> 4 & 0x0F0Fu);       // (the two fields of each byte change places)
            const uint32_t s = spread4(h);
            const uint32_t lo = unpack_perm(tab.t[1], tab.t[0], s & 0x07070707u);
            const uint32_t hi = unpack_perm(tab.t[3], tab.t[2], s & 0x07070707u);
            const uint32_t pick = (s >> 3 & 0x01010101u) * 0xFFu;         // 0xFF in every byte whose code is 8..15
            out[b] = (hi & pick) | (lo & ~pick);
        }
    }
}

// The per-field statement of the format, for any sample (the kernels' plain path: every destination the granule path does
// not take -- odd offsets, heads, tails).  `src` = the slab's packed bytes; -> the ring's two bytes of sample k (I low, Q high).
SDR_UNPACK_HD uint32_t unpack_sample(const uint8_t* src, int64_t k, int bits, bool msb, const UnpackTable& tab) {
    const int per_byte = 8 / bits;
    uint32_t out = 0;
    for (int c = 0; c < 2; ++c) {
        const int64_t j = 2 * k + c;
        const int p = (int)(j % per_byte);
        const int shift = bits * (msb ? per_byte - 1 - p : p);
        const uint32_t code = ((uint32_t)src[j / per_byte] >> shift) & ((1u << bits) - 1u);
        out |= ((tab.t[code >> 2] >> (8 * (code & 3))) & 0xFFu) << (8 * c);
    }
    return out;
}

}  // namespace sdr
