// The converter's handle and what ddc.hip (mixer, FIR low-pass, integer decimation) and resample.hip (interpolation by L,
// decimation by M) share of its kernels: the raw input's formats and the rounding of an integer ring.
#pragma once

#include "engine_internal.h"
#include "ddc_layout.h"
#include "ddc_array.h"
#include "ddc_stap.h"
#include "mitigate.h"

struct sdr_ddc {
    sdr_engine* engine = nullptr;
    int in_fmt = 0, D = 1, T = 1;
    uint64_t fcw = 0;
    double gain = 1.0;
    double* taps = nullptr;      // device [T]
    void* hist = nullptr;        // device [max(T-1, 1)] raw inputs, oldest first
    int64_t n_seen = 0;          // inputs since creation / reset
    sdr::Mitigator* mit = nullptr;    // between the filter's output and the ring's format (sdr_ddc_mitigate), or none
    // a rational resampler (sdr_ddc_create_rational with L > 1, resample.hip): D is M, T the prototype's length, `taps` the
    // table [Tp][L'] of resample_tiles.h and `hist` the last Tp - 1 raw inputs
    int L = 1;
    int Tp = 1;                  // ceil(T / L): the history holds Tp - 1 inputs (L = 1: T)
    // a converter made by sdr_ddc_create_layout: in_fmt is not read, the staged bytes are decoded by `layout` where the kernels
    // load them and `hist` holds the last Tp - 1 inputs DECODED (ddc_layout.h)
    bool has_layout = false;
    sdr::DdcLayout layout = {};
    // a converter made by sdr_ddc_create_array (has_layout too): the kernels combine the K elements of a frame where they load
    // it and `hist` holds the last Tp - 1 COMBINED inputs as cf64 (ddc_array.h).  With SDR_DDC_ARRAY_MEASURE `cov` is the device's
    // 64 covariance slots (int64, or fp64 of a float32 layout), cov_n the inputs they hold, cov_slab the float pass's rows
    bool has_array = false;
    sdr::DdcArray array = {};
    void* cov = nullptr;
    int64_t cov_n = 0;
    DevBuf cov_slab;
    // a converter made by sdr_ddc_create_stap (has_array too; array.w is not read): T taps per element, `tail` the device's raw
    // tail of the last T - 1 decoded frames (ddc_stap.h) beside `hist`, and `cov` T lags of kDdcStapCovSlots slots each
    bool has_stap = false;
    sdr::DdcStap stap = {};
    double* tail = nullptr;
};

// Bytes of the covariance slots of a measuring converter.
inline size_t ddc_cov_bytes(const sdr_ddc* d) {
    return d->has_stap ? (size_t)d->stap.T * sdr::kDdcStapCovSlots * sizeof(int64_t) : (size_t)sdr::kDdcArrayCovSlots * sizeof(int64_t);
}

inline size_t ddc_in_bytes(int in_fmt) {
    switch (in_fmt) {
        case SDR_DDC_IN_R8: return 1;
        case SDR_DDC_IN_R16: return 2;
        case SDR_DDC_IN_CI8: return 2;
        case SDR_DDC_IN_CI16: return 4;
    }
    return 0;
}

// Bytes one input takes in the history.
inline size_t ddc_hist_unit(const sdr_ddc* d) {
    if (d->has_array) return (size_t)sdr::kDdcArrayHistoryUnit;
    return d->has_layout ? (size_t)sdr::ddc_layout_history_unit(d->layout) : ddc_in_bytes(d->in_fmt);
}

__device__ __forceinline__ void ddc_load(const void* __restrict__ p, int64_t i, int in_fmt, double* re, double* im) {
    switch (in_fmt) {
        case SDR_DDC_IN_R8: *re = (double)((const int8_t*)p)[i], *im = 0.0; break;
        case SDR_DDC_IN_R16: *re = (double)((const int16_t*)p)[i], *im = 0.0; break;
        case SDR_DDC_IN_CI8: {
            const uint16_t w = ((const uint16_t*)p)[i];
            *re = (double)(int8_t)(w & 0xff), *im = (double)(int8_t)(w >> 8);
            break;
        }
        default: {
            const uint32_t w = ((const uint32_t*)p)[i];
            *re = (double)(int16_t)(w & 0xffff), *im = (double)(int16_t)(w >> 16);
            break;
        }
    }
}

// How phase 1 of ddc_kernel / resample_kernel reads input `i` of the push's block or of the history: one of the four formats ...
struct DdcFormatLoad {
    int in_fmt;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const { ddc_load(p, i, in_fmt, re, im); }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { ddc_load(p, i, in_fmt, re, im); }
};
// ... or a layout's frames, the history holding decoded components.
struct DdcLayoutLoad {
    sdr::DdcLayout lay, hist;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_layout_load(p, i, lay, re, im); }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_layout_load(p, i, hist, re, im); }
};
// ... or an array's: the K elements of a frame combined with the weights, the history holding combined inputs as cf64.
struct DdcArrayLoad {
    sdr::DdcLayout lay;
    sdr::DdcArray arr;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_load(p, i, lay, arr, re, im); }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_history_load(p, i, re, im); }
};

// ... or a space-time array's: T frames of K elements combined per input, earlier frames than the push's first out of the raw tail.
struct DdcStapLoad {
    sdr::DdcLayout lay;
    sdr::DdcArray arr;
    sdr::DdcStap stap;
    const double* tail;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const {
        sdr::ddc_stap_load(p, tail, i, lay, arr, stap, re, im);
    }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_history_load(p, i, re, im); }
};

__device__ __forceinline__ double ddc_clip_rint(double v, double lim) { return fmin(fmax(rint(v), -lim), lim); }

inline int ddc_check(sdr_engine* e, const sdr_ddc* d) {
    if (!d) return sdr_fail(SDR_ERR_INVALID, "converter is NULL");
    if (d->engine != e) return sdr_fail(SDR_ERR_INVALID, "the converter belongs to another engine");
    return SDR_OK;
}

namespace sdr {

// resample.hip: the push of a converter with L > 1 (the arguments already checked against NULL and the engine by the caller).
// ddc.hip: the history launch behind a push's kernel -- the last d->Tp - 1 of the raw inputs in the staging buffer and the old
// history, under the scope "ddc_history_kernel".
void ddc_history_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in);
// ddc.hip: the bytes a push of n_in >= 0 inputs copies to the staging buffer; of a converter with a layout SDR_ERR_INVALID when
// they are not whole (nothing has changed then).
int ddc_push_bytes(const sdr_ddc* d, int64_t n_in, size_t* bytes);
int rs_push_impl(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t off, int64_t* n_out, bool wait);
// ddc_array.hip: the covariance pass of a converter with SDR_DDC_ARRAY_MEASURE over the n_in frames in the staging buffer, behind
// the converter's kernel on the engine's stream, under the scope "ddc_array_cov_kernel"; no-op for every other converter.
// ddc_array_cov_reserve, before the push has changed anything, makes room for the float pass's rows (SDR_ERR_NOMEM otherwise).
int ddc_array_cov_reserve(sdr_engine* e, sdr_ddc* d, int64_t n_in);
void ddc_array_cov_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in);
// ddc_stap.hip: the same two for a converter of sdr_ddc_create_stap (ddc_array_cov_* hand over to them): a lag per grid row,
// partners before the push's first frame out of the raw tail, under the scope "ddc_stap_cov_kernel".
int ddc_stap_cov_reserve(sdr_engine* e, sdr_ddc* d, int64_t n_in);
void ddc_stap_cov_launch(sdr_engine* e, sdr_ddc* d, int64_t n_in);

}  // namespace sdr
