// What the two covariance passes of a measuring converter share -- ddc_array.hip's (the Hermitian-packed R of an array) and
// ddc_stap.hip's (the full lag matrices of a space-time array): the shape of a workgroup, the three accumulation modes and their
// types, the wave's butterfly, the dispatch over K and mode, and the push's two calls.
#pragma once

#include <type_traits>

#include "ddc_handle.h"

namespace sdr {

constexpr int kCovThreads = 256, kCovWaves = kCovThreads / 64, kCovRun = 64;
constexpr int64_t kCovChunk = (int64_t)kCovThreads * kCovRun;     // frames of a workgroup
// INT8 and PACKED fields: int32 partials; INT16: int64 partials of int elements; FLOAT32: fp64 (the passes' files say why)
constexpr int kCovNarrow = 0, kCovWide = 1, kCovFloat = 2;

template <int MODE>
struct CovTypes {
    typedef int acc;
    typedef int el;
};
template <>
struct CovTypes<kCovWide> {
    typedef long long acc;
    typedef int el;
};
template <>
struct CovTypes<kCovFloat> {
    typedef double acc;
    typedef double el;
};

template <class T>
__device__ __forceinline__ T cov_wave_add(T v) {     // a fixed butterfly: the same bits every time
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

inline int cov_mode(const DdcLayout& l) { return l.kind == kDdcFieldFloat32 ? kCovFloat : l.kind == kDdcFieldInt16 ? kCovWide : kCovNarrow; }

inline int64_t cov_workgroups(int64_t n_in) { return (n_in + kCovChunk - 1) / kCovChunk; }

// launch(k, m) with K and the mode as integral constants: decltype(k)::value, decltype(m)::value.
template <int K, class F>
void cov_dispatch_mode(int mode, F& launch) {
    if (mode == kCovFloat) launch(std::integral_constant<int, K>(), std::integral_constant<int, kCovFloat>());
    else if (mode == kCovWide) launch(std::integral_constant<int, K>(), std::integral_constant<int, kCovWide>());
    else launch(std::integral_constant<int, K>(), std::integral_constant<int, kCovNarrow>());
}
template <class F>
void cov_dispatch(int K, int mode, F launch) {
    switch (K) {
        case 2: return cov_dispatch_mode<2>(mode, launch);
        case 3: return cov_dispatch_mode<3>(mode, launch);
        case 4: return cov_dispatch_mode<4>(mode, launch);
        case 5: return cov_dispatch_mode<5>(mode, launch);
        case 6: return cov_dispatch_mode<6>(mode, launch);
        case 7: return cov_dispatch_mode<7>(mode, launch);
        default: return cov_dispatch_mode<8>(mode, launch);
    }
}

// ddc_array.hip / ddc_stap.hip: the pass over the n_in > 0 frames in the staging buffer, behind the converter's kernel on the
// engine's stream, under the scope "ddc_array_cov_kernel" / "ddc_stap_cov_kernel".
void ddc_array_cov_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in);
void ddc_stap_cov_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in);

// A push of n_in > 0 inputs, before it has changed anything: room for the float pass's rows, one of the converter's slots per
// workgroup (SDR_ERR_NOMEM otherwise); no-op for a converter that does not measure.
inline int ddc_cov_reserve(sdr_engine* e, sdr_ddc* d, int64_t n_in) {
    if (!d->cov) return SDR_OK;
    const int64_t grid = cov_workgroups(n_in);
    if (grid > 0x7fffffff) return sdr_fail(SDR_ERR_RANGE, "%lld frames in one push of a measuring array", (long long)n_in);
    if (cov_mode(d->layout) != kCovFloat) return SDR_OK;
    return sdr_devbuf_reserve(e, &d->cov_slab, (size_t)grid * ddc_cov_bytes(d));
}

// ... and behind its kernel: the pass of its kind.
inline void ddc_cov_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in) {
    if (!d->cov) return;
    if (d->kind == kDdcKindStap) ddc_stap_cov_launch(e, d, n_in);
    else ddc_array_cov_launch(e, d, n_in);
}

}  // namespace sdr
