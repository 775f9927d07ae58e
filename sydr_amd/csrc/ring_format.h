// How a sample of each ring format (sdr_iq_format) lies in memory: the one place that knows.  Per-format constants, one
// sample out of a ring as fp64 (ring_read), one fp64 value into a ring under sdr_ddc_push's rounding rule (ring_write), and
// the host's choice of a kernel instantiation by format (with_fmt).  The whole-granule unpackers of the hot paths (Loader /
// Raw8 in correlator.h, biased_sample in correlator_chip.h, IntFmt in probe.hip, sample_get / sample_put in cancel.hip) are
// register layouts of their kernels and stay there; they take their constants from here.
// Everything is __host__ __device__ or constexpr: tests/csrc/ring_format_check.hip runs it on the CPU.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/sydr_amd.h"

constexpr size_t sdr_fmt_bytes(int fmt) {
    switch (fmt) {
        case SDR_FMT_CI8: return 2;
        case SDR_FMT_CI16: return 4;
        case SDR_FMT_CF32: return 8;
        case SDR_FMT_CF64: return 16;
    }
    return 0;
}

namespace sdr {

// Samples in one 16-byte granule: what a lane moves with one load or store.
constexpr int ring_granule_samples(int fmt) { return 16 / (int)sdr_fmt_bytes(fmt); }

// The symmetric rails an integer ring clips to (sdr_ddc_push: -128 and -32768 are never produced).
constexpr int ring_rail(int fmt) { return fmt == SDR_FMT_CI8 ? 127 : (fmt == SDR_FMT_CI16 ? 32767 : 0); }

// A ci8 ring holds its samples with the sign bit of every byte flipped (u = x + 128 as an unsigned byte: "offset binary") --
// the form the straight-line correlators build their doubles from with one v_perm_b32 per component (correlator_chip.h
// biased_sample).  Round 6: that IS the ring, not an image beside it -- the engine flips where samples enter (uploads, the
// ingest kernels, the synthesiser, ring_write) and flips back where they leave (sdr_iq_download); every other reader takes
// the bits back with one exclusive or per dword of two samples.
constexpr uint32_t kCi8Flip = 0x80808080u;
__host__ __device__ __forceinline__ int ci8_native(int w) { return w ^ (int)kCi8Flip; }

// The dword a ring's words are xor-ed with on their way in and out, and the byte an empty ring (every sample 0 + 0j) is
// filled with.
constexpr uint32_t ring_flip_mask(int fmt) { return fmt == SDR_FMT_CI8 ? kCi8Flip : 0u; }
constexpr int ring_fill_byte(int fmt) { return (int)(ring_flip_mask(fmt) & 0xffu); }

// One ring sample, widened to fp64.
template <int FMT>
__host__ __device__ __forceinline__ double2 ring_read(const void* ring, int64_t pos) {
    if (FMT == SDR_FMT_CI8) {
        constexpr int flip = ring_fill_byte(SDR_FMT_CI8);
        const char2 v = static_cast<const char2*>(ring)[pos];
        return make_double2((double)(int8_t)(v.x ^ flip), (double)(int8_t)(v.y ^ flip));
    } else if (FMT == SDR_FMT_CI16) {
        const short2 v = static_cast<const short2*>(ring)[pos];
        return make_double2((double)v.x, (double)v.y);
    } else if (FMT == SDR_FMT_CF32) {
        const float2 v = static_cast<const float2*>(ring)[pos];
        return make_double2((double)v.x, (double)v.y);
    } else {
        return static_cast<const double2*>(ring)[pos];
    }
}

// sdr_ddc_push's rule for an integer ring: round to nearest, ties to even, then clip to the symmetric rails.
__host__ __device__ __forceinline__ double clip_rint(double v, double lim) { return fmin(fmax(rint(v), -lim), lim); }

// One fp64 value into a ring (or a buffer) of format `fmt`: clip_rint for the integer formats, a ci8 ring's bytes flipped,
// (float) for cf32, the bits themselves for cf64.
__host__ __device__ __forceinline__ void ring_write(void* __restrict__ ring, int fmt, int64_t pos, double re, double im) {
    switch (fmt) {
        case SDR_FMT_CI8: {
            constexpr double lim = ring_rail(SDR_FMT_CI8);
            const int r = (int)clip_rint(re, lim), i = (int)clip_rint(im, lim);
            ((uint16_t*)ring)[pos] = (uint16_t)((((unsigned)r & 0xffu) | (((unsigned)i & 0xffu) << 8)) ^ (kCi8Flip & 0xffffu));
            break;
        }
        case SDR_FMT_CI16: {
            constexpr double lim = ring_rail(SDR_FMT_CI16);
            const int r = (int)clip_rint(re, lim), i = (int)clip_rint(im, lim);
            ((uint32_t*)ring)[pos] = ((unsigned)r & 0xffffu) | (((unsigned)i & 0xffffu) << 16);
            break;
        }
        case SDR_FMT_CF32: ((float2*)ring)[pos] = make_float2((float)re, (float)im); break;
        default: ((double2*)ring)[pos] = make_double2(re, im); break;
    }
}

// THE switch over the ring's format on the host: f(std::integral_constant<int, F>{}) for the ring's F, whatever f returns.
// A value that is none of ci8, ci16, cf32 goes to cf64.
template <class F>
decltype(auto) with_fmt(int fmt, F&& f) {
    switch (fmt) {
        case SDR_FMT_CI8: return f(std::integral_constant<int, SDR_FMT_CI8>{});
        case SDR_FMT_CI16: return f(std::integral_constant<int, SDR_FMT_CI16>{});
        case SDR_FMT_CF32: return f(std::integral_constant<int, SDR_FMT_CF32>{});
        default: return f(std::integral_constant<int, SDR_FMT_CF64>{});
    }
}

}  // namespace sdr
