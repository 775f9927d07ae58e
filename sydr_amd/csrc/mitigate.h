// What ddc.hip needs of the mitigator (mitigate.hip): a pulse blanker and a narrow-band excisor between the converter's
// fp64 output and the ring's format.  The statement is sydr_amd/signal/mitigate.py; the index arithmetic is mit_plan.h.
#pragma once

#include "engine_internal.h"

namespace sdr {

struct Mitigator;

// Checks cfg (SDR_ERR_INVALID as include/sydr_amd.h lists) and makes the device tables, the zero state and the counters.
int mit_create(sdr_engine* e, const sdr_mit_cfg* cfg, Mitigator** out);
void mit_destroy(sdr_engine* e, Mitigator* m);
int mit_reset(sdr_engine* e, Mitigator* m);
int64_t mit_delay_of(const Mitigator* m);
// A push of k outputs behind n earlier ones.  begin: sizes the buffers and says where ddc_kernel is to write its cf64
// outputs (a linear buffer: *dst, first output at sample *offset, *capacity samples); it queues nothing and changes no state.
// finish: the kernels behind ddc_kernel on the engine's stream -- blank, excise, combine into the ring at ring_offset -- and
// the state's hand-over.
int mit_push_begin(sdr_engine* e, Mitigator* m, int64_t n, int64_t k, void** dst, int64_t* offset, int64_t* capacity);
int mit_push_finish(sdr_engine* e, Mitigator* m, int64_t n, int64_t k, int64_t ring_offset);
// The counters once n outputs have been delivered (waits for the engine's stream); bins: nullable [nfft].
int mit_stats(sdr_engine* e, Mitigator* m, int64_t n, sdr_mit_stats* out, int64_t* bins);

}  // namespace sdr
