// Host-side proof of the field arithmetic of an input layout (sydr_amd/csrc/ddc_layout.h), the code the converter's kernels
// decode their inputs with: every input j < 64 of every valid layout with stride <= 9 -- packed fields of 1, 2 and 4 bits in both
// bit orders, int8, int16 and float32 fields, every lane, real and complex, with and without the swap -- against a reading
// written out here: a packed stream is taken apart BIT BY BIT (bit n of the stream is bit n % 8 of byte n / 8; a field's code is
// assembled from its bits, most significant first, at the position the definition gives it), an unpacked one element by
// element.  Then the limits (ddc_layout_valid), the bytes of a push (ddc_layout_push_bytes) against a count of bits, and the
// history: inputs stored decoded by ddc_layout_history_store read back by ddc_layout_load as what went in.
// Built with `hipcc --cuda-host-only`.
//   usage: ddc_layout_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/ddc_layout.h"

using namespace sdr;

static uint64_t state = 20260019;
static uint64_t next_random() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

// Field f of a packed stream, bit by bit: F = 8 / bits fields to a byte, field f at position p = f % F of byte f / F, its
// code the `bits` bits from bit bits * p (or bits * (F - 1 - p)) up.
static int packed_field_bitwise(const std::vector<uint8_t>& bytes, int64_t f, int bits, bool msb_first, const int8_t* levels) {
    const int F = 8 / bits;
    const int64_t byte = f / F;
    const int p = (int)(f % F);
    const int low = bits * (msb_first ? F - 1 - p : p);
    int code = 0;
    for (int b = bits - 1; b >= 0; --b) {
        const int64_t n = byte * 8 + low + b;                      // (bit n of the stream)
        code = code * 2 + ((bytes[(size_t)(n / 8)] >> (n % 8)) & 1);
    }
    return levels[code];
}

int main() {
    long cases = 0;
    const int n_frames = 64;
    const int8_t tables[3][16] = {{1, -1}, {1, 3, -1, -3}, {0, 1, 2, 3, 4, 5, 6, 7, -8, -7, -6, -5, -4, -3, -2, -128}};
    for (int kind = kDdcFieldInt8; kind <= kDdcFieldPacked; ++kind)
        for (int bits_at = 0; bits_at < (kind == kDdcFieldPacked ? 3 : 1); ++bits_at)
            for (int msb = 0; msb <= (kind == kDdcFieldPacked ? 1 : 0); ++msb)
                for (int stride = 1; stride <= 9; ++stride)
                    for (int cplx = 0; cplx <= 1; ++cplx)
                        for (int swap = 0; swap <= cplx; ++swap)
                            for (int lane = 0; lane + (cplx ? 2 : 1) <= stride; ++lane) {
                                const int bits = kind == kDdcFieldPacked ? 1 << bits_at : 0;
                                const int flags = (cplx ? kDdcLayoutComplex : 0) | (swap ? kDdcLayoutSwapIq : 0) | (msb ? kDdcLayoutMsbFirst : 0);
                                if (!ddc_layout_valid(kind, bits, stride, lane, flags, 0)) {
                                    printf("valid layout refused: kind=%d bits=%d stride=%d lane=%d flags=%d\n", kind, bits, stride, lane, flags);
                                    return 1;
                                }
                                const int8_t* levels = tables[bits_at];
                                const DdcLayout l = ddc_layout_make(kind, bits, stride, lane, flags, levels);
                                const int64_t n_fields = (int64_t)n_frames * stride;
                                // the stream's bytes (a packed stream's last byte may hold fields past the last frame) and
                                // every field's value read the long way
                                const int field_bits = kind == kDdcFieldPacked ? bits : 8 * ddc_field_bytes(kind);
                                std::vector<uint8_t> bytes((size_t)((n_fields * field_bits + 7) / 8));
                                for (auto& b : bytes) b = (uint8_t)next_random();
                                std::vector<double> want((size_t)n_fields);
                                for (int64_t f = 0; f < n_fields; ++f) {
                                    if (kind == kDdcFieldPacked) {
                                        want[(size_t)f] = packed_field_bitwise(bytes, f, bits, msb != 0, levels);
                                    } else if (kind == kDdcFieldInt8) {
                                        int8_t v;
                                        memcpy(&v, &bytes[(size_t)f], 1);
                                        want[(size_t)f] = v;
                                    } else if (kind == kDdcFieldInt16) {
                                        int16_t v;
                                        memcpy(&v, &bytes[(size_t)(2 * f)], 2);
                                        want[(size_t)f] = v;
                                    } else {
                                        float v = (float)((int)(next_random() % 65536) - 32768) * 0.37f;     // (finite: compared as values)
                                        memcpy(&bytes[(size_t)(4 * f)], &v, 4);
                                        want[(size_t)f] = v;
                                    }
                                }
                                const int64_t push_bits = n_fields * field_bits;
                                const int64_t b = ddc_layout_push_bytes(l, n_frames);
                                if (b != (push_bits % 8 ? -1 : push_bits / 8)) {
                                    printf("push bytes: kind=%d bits=%d stride=%d -> %lld\n", kind, bits, stride, (long long)b);
                                    return 1;
                                }
                                const DdcLayout h = ddc_layout_history(l);
                                std::vector<uint8_t> hist((size_t)n_frames * (size_t)ddc_layout_history_unit(l));
                                if (ddc_layout_history_unit(l) != (cplx ? 2 : 1) * (kind == kDdcFieldPacked ? 1 : ddc_field_bytes(kind))) {
                                    printf("history unit: kind=%d cplx=%d -> %d\n", kind, cplx, ddc_layout_history_unit(l));
                                    return 1;
                                }
                                for (int64_t j = 0; j < n_frames; ++j) {
                                    const double a = want[(size_t)(j * stride + lane)], q = cplx ? want[(size_t)(j * stride + lane + 1)] : 0.0;
                                    const double want_re = swap ? q : a, want_im = cplx ? (swap ? a : q) : 0.0;
                                    double re = -1e300, im = -1e300;
                                    ddc_layout_load(bytes.data(), j, l, &re, &im);
                                    if (re != want_re || im != want_im) {
                                        printf("decode: kind=%d bits=%d msb=%d stride=%d lane=%d cplx=%d swap=%d j=%lld: (%g, %g), want (%g, %g)\n", kind,
                                               bits, msb, stride, lane, cplx, swap, (long long)j, re, im, want_re, want_im);
                                        return 1;
                                    }
                                    ddc_layout_history_store(hist.data(), (int)j, h, re, im);
                                    ++cases;
                                }
                                for (int64_t j = 0; j < n_frames; ++j) {
                                    double re = -1e300, im = -1e300, re2, im2;
                                    ddc_layout_load(bytes.data(), j, l, &re, &im);
                                    ddc_layout_load(hist.data(), j, h, &re2, &im2);
                                    if (re != re2 || im != im2) {
                                        printf("history: kind=%d bits=%d stride=%d lane=%d j=%lld\n", kind, bits, stride, lane, (long long)j);
                                        return 1;
                                    }
                                }
                            }
    // the limits: everything outside them is refused
    struct Bad {
        int kind, bits, stride, lane, flags, reserved;
    };
    const Bad bad[] = {{-1, 0, 1, 0, 0, 0}, {4, 0, 1, 0, 0, 0},       {3, 0, 1, 0, 0, 0},  {3, 3, 1, 0, 0, 0},  {3, 8, 1, 0, 0, 0},  {0, 1, 1, 0, 0, 0},
                       {1, 2, 1, 0, 0, 0},  {2, 4, 1, 0, 0, 0},       {0, 0, 0, 0, 0, 0},  {0, 0, 65, 0, 0, 0}, {0, 0, 1, -1, 0, 0}, {0, 0, 1, 1, 0, 0},
                       {0, 0, 2, 1, 1, 0},  {0, 0, 1, 0, 1, 0},       {0, 0, 2, 0, 2, 0},  {0, 0, 2, 0, 4, 0},  {1, 0, 2, 0, 5, 0},  {2, 0, 2, 0, 4, 0},
                       {0, 0, 2, 0, 8, 0},  {0, 0, 2, 0, 1 << 30, 0}, {0, 0, 2, 0, -1, 0}, {0, 0, 1, 0, 0, 1},  {3, 2, 4, 3, 1, 0}};
    for (const Bad& c : bad) {
        if (ddc_layout_valid(c.kind, c.bits, c.stride, c.lane, c.flags, c.reserved)) {
            printf("bad layout accepted: kind=%d bits=%d stride=%d lane=%d flags=%d reserved=%d\n", c.kind, c.bits, c.stride, c.lane, c.flags, c.reserved);
            return 1;
        }
        ++cases;
    }
    if (!ddc_layout_valid(3, 4, 64, 62, 7, 0) || !ddc_layout_valid(2, 0, 64, 63, 0, 0)) {
        printf("the ends of the domain refused\n");
        return 1;
    }
    // large indices: the field index and the byte are 64-bit
    {
        const DdcLayout l = ddc_layout_make(kDdcFieldPacked, 2, 64, 63, kDdcLayoutMsbFirst, tables[1]);
        const int64_t j = ((int64_t)1 << 40) + 5, f = ddc_frame_field(l, j);
        if (f != j * 64 + 63 || ddc_field_byte(f, 2) != f / 4 || ddc_field_shift(f, 2, true) != 2 * (3 - (int)(f % 4)) ||
            ddc_layout_push_bytes(l, kDdcLayoutMaxFrames) != kDdcLayoutMaxFrames * 16) {
            printf("large indices\n");
            return 1;
        }
        ++cases;
    }
    printf("ok %ld\n", cases);
    return 0;
}
