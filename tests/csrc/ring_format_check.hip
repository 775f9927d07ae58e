// Host-side proof of sydr_amd/csrc/ring_format.h -- how a sample of each ring format lies in memory, read (ring_read), written
// (ring_write) and dispatched (with_fmt) -- built with `hipcc --cuda-host-only`, plain by tests/test_ring_format.py and under
// the address and undefined-behaviour sanitizers by `make check-sanitize`.  What is expected is restated here in integer and
// plain C arithmetic that knows nothing of the header:
//  - ci8 read: every stored byte pair (b0, b1) reads as (int8_t)(b ^ 0x80) per component;
//  - ci8 write: every multiple of 0.25 in -200 .. 200 is stored as (clip(round-half-even(v), +-127) + 128) & 0xff and reads
//    back as the clipped value; the byte 0x00 (-128) never appears; the ties 0.5, 1.5, 126.5, 127.5;
//  - ci16 write at the rails (+-32766.5, +-32767, +-32767.5, +-32768, +-1e9), and components of opposite sign side by side;
//  - cf32 stores (float)v, cf64 stores the bits, NaN and +-Inf included;
//  - NaN and +-Inf into the integer formats: what the store of the down-converter gave before this header existed (its
//    expression, copied below);
//  - the flip mask, and a ring filled with the fill byte reads as 0 + 0j in every format;
//  - with_fmt reaches each format's own constant; -1, 4 and 99 reach cf64;
//  - a write touches its own sample only.
//   usage: ring_format_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../sydr_amd/csrc/ring_format.h"

using namespace sdr;

static_assert(sdr_fmt_bytes(SDR_FMT_CI8) == 2 && sdr_fmt_bytes(SDR_FMT_CI16) == 4 && sdr_fmt_bytes(SDR_FMT_CF32) == 8 &&
                  sdr_fmt_bytes(SDR_FMT_CF64) == 16 && sdr_fmt_bytes(-1) == 0 && sdr_fmt_bytes(4) == 0,
              "bytes per sample");
static_assert(ring_granule_samples(SDR_FMT_CI8) == 8 && ring_granule_samples(SDR_FMT_CI16) == 4 &&
                  ring_granule_samples(SDR_FMT_CF32) == 2 && ring_granule_samples(SDR_FMT_CF64) == 1,
              "samples per 16-byte granule");
static_assert(ring_rail(SDR_FMT_CI8) == 127 && ring_rail(SDR_FMT_CI16) == 32767, "symmetric rails");
static_assert(kCi8Flip == 0x80808080u && ring_flip_mask(SDR_FMT_CI8) == 0x80808080u && ring_flip_mask(SDR_FMT_CI16) == 0u &&
                  ring_flip_mask(SDR_FMT_CF32) == 0u && ring_flip_mask(SDR_FMT_CF64) == 0u,
              "flip mask");
static_assert(ring_fill_byte(SDR_FMT_CI8) == 0x80 && ring_fill_byte(SDR_FMT_CI16) == 0 && ring_fill_byte(SDR_FMT_CF32) == 0 &&
                  ring_fill_byte(SDR_FMT_CF64) == 0,
              "fill byte");

static long long cases = 0;
#define EXPECT(cond, ...)                \
    do {                                 \
        ++cases;                         \
        if (!(cond)) {                   \
            printf(__VA_ARGS__);         \
            printf("  [%s]\n", #cond);   \
            return 1;                    \
        }                                \
    } while (0)

// v = quarters / 4 rounded to the nearest integer, ties to even, in integers
static long long round_half_even_quarters(long long quarters) {
    long long q = quarters / 4, rem = quarters % 4;
    if (rem < 0) --q, rem += 4;   // floor division
    if (rem < 2) return q;
    if (rem > 2) return q + 1;
    return (q % 2 == 0) ? q : q + 1;
}
static long long clip(long long v, long long lim) { return v < -lim ? -lim : (v > lim ? lim : v); }

// The down-converter's store into the integer formats as it stood before ring_format.h (ddc.hip ddc_store, ddc_handle.h
// ddc_clip_rint), copied: the statement for the values no integer arithmetic above covers.
static double parent_clip_rint(double v, double lim) { return fmin(fmax(rint(v), -lim), lim); }
static uint16_t parent_ci8(double ar, double ai) {
    const int re = (int)parent_clip_rint(ar, 127.0), im = (int)parent_clip_rint(ai, 127.0);
    return (uint16_t)((((unsigned)re & 0xffu) | (((unsigned)im & 0xffu) << 8)) ^ 0x8080u);
}
static uint32_t parent_ci16(double ar, double ai) {
    const int re = (int)parent_clip_rint(ar, 32767.0), im = (int)parent_clip_rint(ai, 32767.0);
    return ((unsigned)re & 0xffffu) | (((unsigned)im & 0xffffu) << 16);
}

constexpr int kSlots = 4;        // a little ring: the sample under test is slot 2, its neighbours carry a guard pattern
constexpr int kAt = 2;
constexpr unsigned char kGuard = 0xa5;

struct Ring {
    alignas(16) unsigned char b[kSlots * 16];
    void guard() { memset(b, kGuard, sizeof b); }
    // every byte outside sample kAt of a format of `bytes` per sample still carries the guard
    bool others_untouched(size_t bytes) const {
        for (size_t i = 0; i < sizeof b; ++i)
            if ((i < kAt * bytes || i >= (kAt + 1) * bytes) && b[i] != kGuard) return false;
        return true;
    }
};

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static int check_ci8() {
    Ring r;
    for (int b0 = 0; b0 < 256; ++b0)
        for (int b1 = 0; b1 < 256; ++b1) {
            r.guard();
            r.b[2 * kAt] = (unsigned char)b0, r.b[2 * kAt + 1] = (unsigned char)b1;
            const double2 x = ring_read<SDR_FMT_CI8>(r.b, kAt);
            EXPECT(x.x == (double)(int8_t)(b0 ^ 0x80) && x.y == (double)(int8_t)(b1 ^ 0x80), "ci8 read of %02x %02x: %g %g\n", b0, b1, x.x, x.y);
        }
    for (long long k = -800; k <= 800; ++k) {
        const double v = (double)k * 0.25;
        const long long c = clip(round_half_even_quarters(k), 127);
        r.guard();
        ring_write(r.b, SDR_FMT_CI8, kAt, v, v);
        const unsigned want = (unsigned)((c + 128) & 0xff);
        EXPECT(r.b[2 * kAt] == want && r.b[2 * kAt + 1] == want, "ci8 write of %g: bytes %02x %02x, want %02x\n", v, r.b[2 * kAt], r.b[2 * kAt + 1], want);
        EXPECT(r.b[2 * kAt] != 0x00, "ci8 write of %g produced -128\n", v);
        EXPECT(r.others_untouched(2), "ci8 write of %g touched a neighbour\n", v);
        const double2 x = ring_read<SDR_FMT_CI8>(r.b, kAt);
        EXPECT(x.x == (double)c && x.y == (double)c, "ci8 write of %g reads back %g %g, want %lld\n", v, x.x, x.y, c);
    }
    const double ties[4][2] = {{0.5, 0.0}, {1.5, 2.0}, {126.5, 126.0}, {127.5, 127.0}};
    for (const auto& t : ties)
        for (int sign = -1; sign <= 1; sign += 2) {
            r.guard();
            ring_write(r.b, SDR_FMT_CI8, kAt, sign * t[0], -sign * t[0]);
            const double2 x = ring_read<SDR_FMT_CI8>(r.b, kAt);
            EXPECT(x.x == sign * t[1] && x.y == -sign * t[1], "ci8 tie %g: %g %g\n", sign * t[0], x.x, x.y);
        }
    return 0;
}

static int check_ci16() {
    Ring r;
    const double in[] = {32766.5, 32767.0, 32767.5, 32768.0, 1e9, 0.5, 1.5, 2.5, 0.0, 1.0, 12345.25};
    const int want[] = {32766, 32767, 32767, 32767, 32767, 0, 2, 2, 0, 1, 12345};
    for (size_t i = 0; i < sizeof in / sizeof in[0]; ++i)
        for (int sign = -1; sign <= 1; sign += 2)
            for (int other = -1; other <= 1; other += 2) {   // (re, im) of equal and of opposite sign: neither bleeds into the other
                r.guard();
                const double re = sign * in[i], im = other * in[i];
                ring_write(r.b, SDR_FMT_CI16, kAt, re, im);
                int16_t got[2];
                memcpy(got, r.b + 4 * kAt, 4);
                EXPECT(got[0] == sign * want[i] && got[1] == other * want[i], "ci16 write of (%g, %g): %d %d\n", re, im, got[0], got[1]);
                EXPECT(r.others_untouched(4), "ci16 write of (%g, %g) touched a neighbour\n", re, im);
                const double2 x = ring_read<SDR_FMT_CI16>(r.b, kAt);
                EXPECT(x.x == (double)got[0] && x.y == (double)got[1], "ci16 read back of (%g, %g): %g %g\n", re, im, x.x, x.y);
            }
    r.guard();
    ring_write(r.b, SDR_FMT_CI16, kAt, -1.0, 1.0);
    uint32_t w;
    memcpy(&w, r.b + 4 * kAt, 4);
    EXPECT(w == 0x0001ffffu, "ci16 (-1, 1) is %08x\n", w);
    ring_write(r.b, SDR_FMT_CI16, kAt, 1.0, -1.0);
    memcpy(&w, r.b + 4 * kAt, 4);
    EXPECT(w == 0xffff0001u, "ci16 (1, -1) is %08x\n", w);
    // every int16 pair a ring can hold, read: the extremes and a walk through the rest
    for (int a = -32768; a <= 32767; a += 257)
        for (int b = 32767; b >= -32768; b -= 4099) {
            const int16_t pair[2] = {(int16_t)a, (int16_t)b};
            memcpy(r.b + 4 * kAt, pair, 4);
            const double2 x = ring_read<SDR_FMT_CI16>(r.b, kAt);
            EXPECT(x.x == (double)a && x.y == (double)b, "ci16 read of %d %d: %g %g\n", a, b, x.x, x.y);
        }
    return 0;
}

static int check_float() {
    Ring r;
    const double inf = std::numeric_limits<double>::infinity();
    double nan_payload;
    const uint64_t nan_bits = 0x7ff8000000abcdefull;
    memcpy(&nan_payload, &nan_bits, 8);
    const double in[] = {0.0, -0.0, 1.0, -3.75, 0.1, 16777217.0, -16777219.0, 1e-50, 1e40, inf, -inf, nan_payload};
    for (double re : in)
        for (double im : {in[4], re}) {
            r.guard();
            ring_write(r.b, SDR_FMT_CF32, kAt, re, im);
            const float want[2] = {(float)re, (float)im};
            EXPECT(memcmp(r.b + 8 * kAt, want, 8) == 0 && r.others_untouched(8), "cf32 write of (%g, %g)\n", re, im);
            const double2 x = ring_read<SDR_FMT_CF32>(r.b, kAt);
            EXPECT(same_bits(x.x, (double)want[0]) && same_bits(x.y, (double)want[1]), "cf32 read back of (%g, %g): %g %g\n", re, im, x.x, x.y);

            r.guard();
            ring_write(r.b, SDR_FMT_CF64, kAt, re, im);
            const double want64[2] = {re, im};
            EXPECT(memcmp(r.b + 16 * kAt, want64, 16) == 0 && r.others_untouched(16), "cf64 write of (%g, %g)\n", re, im);
            const double2 y = ring_read<SDR_FMT_CF64>(r.b, kAt);
            EXPECT(same_bits(y.x, re) && same_bits(y.y, im), "cf64 read back of (%g, %g): %g %g\n", re, im, y.x, y.y);
        }
    EXPECT((float)16777217.0 == 16777216.0f, "16777217 does not round in float here\n");
    // a format that is none of the four stores as cf64 (the default of every switch this header replaced)
    r.guard();
    ring_write(r.b, 99, kAt, 1.5, -2.5);
    const double want64[2] = {1.5, -2.5};
    EXPECT(memcmp(r.b + 16 * kAt, want64, 16) == 0, "format 99 does not store as cf64\n");
    return 0;
}

static int check_nonfinite_into_integers() {
    Ring r;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double in[] = {nan, -nan, inf, -inf, 3.0};
    for (double re : in)
        for (double im : in) {
            r.guard();
            ring_write(r.b, SDR_FMT_CI8, kAt, re, im);
            uint16_t h;
            memcpy(&h, r.b + 2 * kAt, 2);
            EXPECT(h == parent_ci8(re, im), "ci8 write of (%g, %g): %04x, the parent's store gives %04x\n", re, im, h, parent_ci8(re, im));
            r.guard();
            ring_write(r.b, SDR_FMT_CI16, kAt, re, im);
            uint32_t w;
            memcpy(&w, r.b + 4 * kAt, 4);
            EXPECT(w == parent_ci16(re, im), "ci16 write of (%g, %g): %08x, the parent's store gives %08x\n", re, im, w, parent_ci16(re, im));
        }
    return 0;
}

template <int FMT>
static int check_empty_ring() {
    Ring r;
    memset(r.b, ring_fill_byte(FMT), sizeof r.b);
    for (int pos = 0; pos < kSlots * ring_granule_samples(FMT); ++pos) {
        const double2 x = ring_read<FMT>(r.b, pos);
        EXPECT(x.x == 0.0 && x.y == 0.0, "format %d: sample %d of an empty ring reads %g %g\n", FMT, pos, x.x, x.y);
    }
    // the mask is the fill byte four times, and takes a ci8 word of the ring to its native bytes and back
    EXPECT(ring_flip_mask(FMT) == 0x01010101u * (unsigned)ring_fill_byte(FMT), "format %d: mask %08x\n", FMT, ring_flip_mask(FMT));
    return 0;
}

static int check_with_fmt() {
    const int in[] = {SDR_FMT_CI8, SDR_FMT_CI16, SDR_FMT_CF32, SDR_FMT_CF64, -1, 4, 99};
    const int want[] = {0, 1, 2, 3, 3, 3, 3};
    for (size_t i = 0; i < sizeof in / sizeof in[0]; ++i) {
        const int got = with_fmt(in[i], [](auto f) { return (int)decltype(f)::value; });
        EXPECT(got == want[i], "with_fmt(%d) reached %d\n", in[i], got);
        int seen = -1;
        with_fmt(in[i], [&](auto f) { seen = decltype(f)::value; });   // (a callable that returns nothing)
        EXPECT(seen == want[i], "with_fmt(%d), no result: reached %d\n", in[i], seen);
    }
    EXPECT(ci8_native((int)0x80808080u) == 0 && ci8_native((int)0x7f81ff00u) == (int)0xff017f80u, "ci8_native\n");
    return 0;
}

int main() {
    if (check_ci8() || check_ci16() || check_float() || check_nonfinite_into_integers() || check_empty_ring<SDR_FMT_CI8>() ||
        check_empty_ring<SDR_FMT_CI16>() || check_empty_ring<SDR_FMT_CF32>() || check_empty_ring<SDR_FMT_CF64>() || check_with_fmt())
        return 1;
    printf("ok %lld\n", cases);
    return 0;
}
