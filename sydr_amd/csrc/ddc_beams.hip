// Beams of an array or space-time converter (sdr_ddc_beam_attach, _beam_weights, _beam_count, _beams_clear): several weight sets
// over ONE push.  The push stages its bytes once; the converter's own stream (beam 0) is what it always was, and every attached
// beam b >= 1 is one more pass of the converter's kernel over the staged bytes in HBM -- ddc.hip's ddc_beam_kernel, the beam the
// grid's second dimension -- with the beam's weights, its own history of combined inputs and the ring of another engine on the
// same device as its destination.  What a beam's ring must hold needs no statement of its own: it is, byte for byte, what an
// independent converter with those weights on the target engine writes (include/sydr_amd.h).
//
// A beam's weights lie in a table in device memory, one row per beam, and are written there by a one-workgroup kernel on the
// engine's stream that takes them as its argument: the write is ordered behind every push queued so far, which keep the weights
// they were queued with, and in front of the next one -- sdr_ddc_array_weights' rule without a copy out of the caller's memory.
// This file holds the entry points and that kernel; the push is ddc.hip's, the loaders are ddc_handle.h's.
#include "engine_internal.h"
#include "ddc_handle.h"

#include <cmath>

using namespace sdr;

namespace {

struct BeamWeightRow {
    double w[kDdcBeamWeightRow];
};

__global__ __launch_bounds__(kDdcBeamWeightRow) void ddc_beam_set_kernel(double* __restrict__ row, BeamWeightRow v) {
    const int i = threadIdx.x;
    if (i < kDdcBeamWeightRow) row[i] = v.w[i];
}

// w as the caller gives it -- [K][2] of an array converter, [T][K][2] of a space-time one -- as a row of the table: DdcStap::w's
// layout [8][8][2], zero where there is no tap or element (an array's K weights are tap 0's, in front).
bool beam_row(const sdr_ddc* d, const double* w, BeamWeightRow* row) {
    const int K = d->array.K, T = d->kind == kDdcKindStap ? d->stap.T : 1;
    if (!ddc_stap_weights_valid(T, K, w)) return false;
    DdcStap image;
    ddc_stap_set(&image, T, K, w);
    static_assert(sizeof(image.w) == sizeof(row->w), "a row of the beams' table is DdcStap::w");
    for (int t = 0; t < kDdcStapMaxTaps; ++t)
        for (int a = 0; a < kDdcArrayMax; ++a)
            for (int c = 0; c < 2; ++c) row->w[2 * (t * kDdcArrayMax + a) + c] = image.w[t][a][c];
    return true;
}

int beam_row_write(sdr_engine* e, sdr_ddc* d, int beam, const BeamWeightRow& row) {
    hipLaunchKernelGGL(ddc_beam_set_kernel, dim3(1), dim3(kDdcBeamWeightRow), 0, e->stream, d->beam_w + (size_t)(beam - 1) * kDdcBeamWeightRow, row);
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

}  // namespace

void sdr::ddc_beams_release(sdr_ddc* d) {
    for (DdcBeam& b : d->beams) {
        if (b.hist) (void)hipFree(b.hist);
        if (b.ready) (void)hipEventDestroy(b.ready);
    }
    d->beams.clear();
    if (d->beam_w) (void)hipFree(d->beam_w);
    if (d->beams_done) (void)hipEventDestroy(d->beams_done);
    d->beam_w = nullptr, d->beams_done = nullptr;
}

extern "C" {

int sdr_ddc_beam_attach(sdr_engine* e, sdr_ddc* d, sdr_engine* target, const double* w, int* beam) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->kind < kDdcKindArray) return sdr_fail(SDR_ERR_INVALID, "the converter is neither an array nor a space-time converter");
    if (!target || !w) return sdr_fail(SDR_ERR_INVALID, "target or weights is NULL");
    if (target == e) return sdr_fail(SDR_ERR_INVALID, "the target is the converter's own engine: that is beam 0");
    if (target->device != e->device) return sdr_fail(SDR_ERR_INVALID, "the target engine is on another device");
    if (!e->iq || !target->iq) return sdr_fail(SDR_ERR_INVALID, "an engine without a ring");
    if (target->iq_capacity != e->iq_capacity)
        return sdr_fail(SDR_ERR_INVALID, "the target's ring holds %lld samples, the converter's %lld", (long long)target->iq_capacity, (long long)e->iq_capacity);
    for (const DdcBeam& b : d->beams)
        if (b.target == target) return sdr_fail(SDR_ERR_INVALID, "the target is attached already");
    if ((int)d->beams.size() + 1 >= kDdcMaxBeams) return sdr_fail(SDR_ERR_INVALID, "%d beams already", kDdcMaxBeams);
    BeamWeightRow row;
    if (!beam_row(d, w, &row)) return sdr_fail(SDR_ERR_INVALID, "a weight is not finite");
    if (d->mit) return sdr_fail(SDR_ERR_UNSUPPORTED, "the converter has a mitigator: its state is per stream, and there is one mitigator");
    if (d->n_seen != 0) return sdr_fail(SDR_ERR_STATE, "the converter has seen %lld inputs since its creation or reset", (long long)d->n_seen);

    // nothing has changed so far; from here a failure gives back what it has taken
    DdcBeam b;
    b.target = target;
    const bool first = d->beams.empty();
    hipError_t err = hipSuccess;
    if (first) {
        err = hipMalloc((void**)&d->beam_w, (size_t)(kDdcMaxBeams - 1) * kDdcBeamWeightRow * sizeof(double));
        if (err == hipSuccess) err = hipEventCreateWithFlags(&d->beams_done, hipEventDisableTiming);
    }
    if (err == hipSuccess) err = hipMalloc(&b.hist, ddc_hist_bytes(d));
    if (err == hipSuccess) err = hipMemsetAsync(b.hist, 0, ddc_hist_bytes(d), e->stream);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&b.ready, hipEventDisableTiming);
    if (err != hipSuccess) {
        if (b.hist) (void)hipFree(b.hist);
        if (b.ready) (void)hipEventDestroy(b.ready);
        if (first) ddc_beams_release(d);
        return sdr_fail(SDR_ERR_HIP, "sdr_ddc_beam_attach: %s", hipGetErrorString(err));
    }
    d->beams.push_back(b);
    const int index = (int)d->beams.size();
    if (int rc = beam_row_write(e, d, index, row)) return rc;
    if (beam) *beam = index;
    return SDR_OK;
}

int sdr_ddc_beam_weights(sdr_engine* e, sdr_ddc* d, int beam, const double* w) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (beam < 1 || beam > (int)d->beams.size())
        return sdr_fail(SDR_ERR_INVALID, "beam %d outside 1..%d (beam 0 takes sdr_ddc_array_weights / sdr_ddc_stap_weights)", beam, (int)d->beams.size());
    if (!w) return sdr_fail(SDR_ERR_INVALID, "weights is NULL");
    BeamWeightRow row;
    if (!beam_row(d, w, &row)) return sdr_fail(SDR_ERR_INVALID, "a weight is not finite");
    return beam_row_write(e, d, beam, row);
}

int sdr_ddc_beam_count(const sdr_ddc* d) {
    if (!d) return sdr_fail(SDR_ERR_INVALID, "converter is NULL");
    return 1 + (int)d->beams.size();
}

int sdr_ddc_beams_clear(sdr_engine* e, sdr_ddc* d) {
    if (int rc = sdr_set_device(e)) return rc;
    if (int rc = ddc_check(e, d)) return rc;
    if (d->n_seen != 0) return sdr_fail(SDR_ERR_STATE, "the converter has seen %lld inputs since its creation or reset", (long long)d->n_seen);
    SDR_HIP(hipStreamSynchronize(e->stream));     // (a push queued before the reset may still read them)
    ddc_beams_release(d);
    return SDR_OK;
}

}  // extern "C"
