// Rational-rate resampling in the down-converter (sdr_ddc_create_rational): interpolation by L, a prototype FIR at the
// up-sampled rate, decimation by M -- a 16.368 MHz recording enters the ring at 12 MHz (250 / 341).  The mixer is ddc.hip's;
// of the zero-stuffed stream only the non-zero products are formed: output m takes the K_p taps h[p + k L] of its phase
// p = (m M) mod L against the inputs z_{q-k}, q = (m M) div L.  What the ring must hold is stated in include/sydr_amd.h and,
// as NumPy, in sydr_amd/signal/downconvert.py: the same products added in the same order whatever tile or push an output
// falls into, so the ring does not depend on how the stream was cut into pushes, bit for bit.
// Lanes of consecutive outputs sit on different phases, so the taps are no longer wave-uniform: they come by per-lane
// (vector) loads from a table laid out [k][r], r the output's index within the period of L' = L / gcd(L, M) outputs -- for a
// fixed k the loads of a wave are one contiguous run (a wrap at L' aside).  Every index comes from resample_tiles.h.
// The kernel, the push and the constructor are ddc.hip's, with the polyphase filter (DdcPolyphase) in the integer FIR's place;
// what is left here is the entry point.
#include "engine_internal.h"
#include "ddc_handle.h"
#include "resample_tiles.h"

using namespace sdr;

// interpolation == 1 IS sdr_ddc_create: the integer converter's limits, its filter, its launches, its bytes.
extern "C" int sdr_ddc_create_rational(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, sdr_ddc** out) {
    return ddc_create(e, kDdcKindFormat, cfg, interpolation, nullptr, nullptr, 0, nullptr, out);
}
