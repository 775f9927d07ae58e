// K1, the straight-line forms by block length: `epl_kernel<ci8, NT taps, one chip per lane, KM, .., KS | KI>` for the rows of
// SDR_EPL_ROWS_STRAIGHT (epl_variant.h) -- the block lengths KM = 16 .. 25 that epl.hip does not instantiate itself (it keeps
// SDR_EPL_ROWS_HEADLINE: the headline geometries).  A list whose epochs all hold KM.x samples per (half-)chip gets the kernel
// compiled for that length -- 16.4 .. 26.6 MHz for GPS L1 C/A, 32.7 .. 53 MHz through the half-chip view -- instead of the
// run-time-position kernel: three taps half a chip apart (KS), three or five taps whole (half-)chips apart (KI), three taps at
// any other spacing (the block length alone).  One translation unit of its own: ~35 large kernels, compiled beside epl.hip.
#ifdef SDR_TRACE_WG
#undef SDR_TRACE_WG   // (the per-workgroup clocks of the debug build live in epl.hip's kernels)
#endif
#include "engine_internal.h"
#include "epl_kernel.h"

const void* sdr_epl_straight_kernel(int nt, int km, int ks, int ki) {
#define SDR_ROW(NT, KM, KS, KI) \
    if (nt == NT && km == KM && ks == KS && ki == KI) return (const void*)epl_kernel<SDR_FMT_CI8, NT, sdr::kChipMax, KM, 1, KS, KI>;
    SDR_EPL_ROWS_STRAIGHT(SDR_ROW)
#undef SDR_ROW
    return nullptr;
}
