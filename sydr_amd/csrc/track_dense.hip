// The closed-loop kernel for more channels than compute units, in a translation unit of its own: 256-thread workgroups
// capped at 168 registers so that THREE share a CU.  It is compiled with -mllvm -disable-machine-licm: hoisting the fp64
// polynomial constants of sincos / atan / division out of the epoch loop parks ~80 of them in VGPRs for the whole kernel
// (256 instead of 173 registers).
#ifdef SDR_TRACE_DENSE   // (diagnostics: the per-phase clocks of THIS unit's kernels, under their own names)
#define SDR_TRACE_TRACK 1
#define g_track_phase g_track_phase_dense
#define sdr_debug_track_phases sdr_debug_track_phases_dense
#else
#undef SDR_TRACE_TRACK  // (the per-phase clocks of the debug build live in track.hip's own translation unit)
#endif
#include "track_kernel.h"

hipError_t sdr_track_dense_launch(int fmt, int n_taps, int n_ch, size_t shmem, hipStream_t stream, void** args) {
    auto launch = [&](auto kernel) {
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        return hipLaunchKernel((const void*)kernel, dim3(n_ch), dim3(256), args, shmem, stream);
    };
    auto by_taps = [&](auto fmt_c) {
        constexpr int F = decltype(fmt_c)::value;
        return n_taps == 5 ? launch(track_kernel<F, 256, 3, 5>) : launch(track_kernel<F, 256, 3, 3>);
    };
    return sdr::with_fmt(fmt, by_taps);
}
