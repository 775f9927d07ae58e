// The converter's handle and its LOADERS: how the one converter kernel and the one history kernel of ddc.hip read an input of the
// push's block or of the history, and what the history keeps of it.  The kind of a converter picks its loader in one place,
// ddc_with_loader.
#pragma once

#include "engine_internal.h"
#include "ddc_layout.h"
#include "ddc_array.h"
#include "ddc_stap.h"
#include "mitigate.h"

// What a converter's inputs are; every kind has what the kinds before it have (an array has a layout, a space-time array an array).
enum DdcKind {
    kDdcKindFormat = 0,     // sdr_ddc_create / _rational: one of the four raw formats, `hist` raw inputs
    kDdcKindLayout,         // sdr_ddc_create_layout: in_fmt is not read, the staged bytes are decoded by `layout` where the kernels
                            // load them and `hist` holds the inputs DECODED (ddc_layout.h)
    kDdcKindArray,          // sdr_ddc_create_array: the K elements of a frame combined where they are loaded, `hist` holds COMBINED
                            // inputs as cf64 (ddc_array.h)
    kDdcKindStap            // sdr_ddc_create_stap (array.w is not read): T taps per element, `tail` the raw tail (ddc_stap.h)
};

// An attached BEAM (sdr_ddc_beam_attach): a further weight set of an array or space-time converter whose stream goes into the
// ring of `target`.  Its weights are row (beam - 1) of sdr_ddc::beam_w, its history the converter's own kind of history.
constexpr int kDdcMaxBeams = SDR_DDC_MAX_BEAMS;
constexpr int kDdcBeamWeightRow = sdr::kDdcStapMaxTaps * sdr::kDdcArrayMax * 2;     // doubles: DdcStap::w's layout; an array's w in front
struct DdcBeam {
    sdr_engine* target = nullptr;
    void* hist = nullptr;             // device [max(Tp-1, 1)] combined inputs, cf64
    hipEvent_t ready = nullptr;       // recorded on the target's stream in front of a push: what it queued on its ring comes first
};

// The attached beams' destinations as their kernels take them, by value: entry b is beam b + 1.
struct DdcBeamDst {
    void* ring[kDdcMaxBeams - 1];
    void* hist[kDdcMaxBeams - 1];
    int fmt[kDdcMaxBeams - 1];
};

struct sdr_ddc {
    sdr_engine* engine = nullptr;
    DdcKind kind = kDdcKindFormat;
    int in_fmt = 0, D = 1, T = 1;
    uint64_t fcw = 0;
    double gain = 1.0;
    // interpolation by L (sdr_ddc_create_rational; 1: the integer converter, `taps` its T taps): D is M, T the prototype's length,
    // `taps` the table [Tp][L'] of resample_tiles.h
    int L = 1;
    int Tp = 1;                  // ceil(T / L): the history holds Tp - 1 inputs
    double* taps = nullptr;      // device
    void* hist = nullptr;        // device [max(Tp-1, 1)] inputs as the kind keeps them, oldest first
    int64_t n_seen = 0;          // inputs since creation / reset
    sdr::Mitigator* mit = nullptr;    // between the filter's output and the ring's format (sdr_ddc_mitigate), or none
    sdr::DdcLayout layout = {};
    sdr::DdcArray array = {};
    // with SDR_DDC_ARRAY_MEASURE `cov` is the device's covariance slots (int64, or fp64 of a float32 layout) -- an array's 64, a
    // space-time array's T lags of kDdcStapCovSlots --, cov_n the inputs they hold, cov_slab the float pass's rows
    void* cov = nullptr;
    int64_t cov_n = 0;
    DevBuf cov_slab;
    sdr::DdcStap stap = {};
    double* tail = nullptr;      // device: the last stap.T - 1 decoded frames
    std::vector<DdcBeam> beams;  // beam 1 .. (beam 0 is the converter's own stream)
    double* beam_w = nullptr;    // device [kDdcMaxBeams - 1][kDdcBeamWeightRow], written on the engine's stream (ddc_beam_set_kernel)
    hipEvent_t beams_done = nullptr;   // recorded on the engine's stream behind the beams' kernels: the targets' streams wait for it
};

// Bytes of the covariance slots of a measuring converter.
inline size_t ddc_cov_bytes(const sdr_ddc* d) {
    return d->kind == kDdcKindStap ? (size_t)d->stap.T * sdr::kDdcStapCovSlots * sizeof(int64_t) : (size_t)sdr::kDdcArrayCovSlots * sizeof(int64_t);
}

SDR_DDC_HD inline size_t ddc_in_bytes(int in_fmt) {
    switch (in_fmt) {
        case SDR_DDC_IN_R8: return 1;
        case SDR_DDC_IN_R16: return 2;
        case SDR_DDC_IN_CI8: return 2;
        case SDR_DDC_IN_CI16: return 4;
    }
    return 0;
}

// Bytes one input takes in the history, and the history's (at least one unit, so that there is always a buffer).
inline size_t ddc_hist_unit(const sdr_ddc* d) {
    if (d->kind >= kDdcKindArray) return (size_t)sdr::kDdcArrayHistoryUnit;
    return d->kind == kDdcKindLayout ? (size_t)sdr::ddc_layout_history_unit(d->layout) : ddc_in_bytes(d->in_fmt);
}
inline size_t ddc_hist_bytes(const sdr_ddc* d) { return (size_t)(d->Tp > 1 ? d->Tp - 1 : 1) * ddc_hist_unit(d); }

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

// A loader is a kernel argument by value.  block / history: input `i` of the push's block or of the history as x = re + i im, for
// the converter kernel.  Kept, kept_block / kept_history and keep: what the history holds of an input, its read out of the block or
// out of the old history and its store as element i, for the history kernel.  kTail: whether a raw tail is kept beside the history.
//
// One of the four formats: the history holds raw inputs, copied as units of 1, 2 or 4 bytes ...
struct DdcFormatLoad {
    int in_fmt;
    typedef uint32_t Kept;
    static constexpr bool kTail = false;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const { ddc_load(p, i, in_fmt, re, im); }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { ddc_load(p, i, in_fmt, re, im); }
    __device__ __forceinline__ Kept kept_block(const void* p, int64_t i) const {
        const int unit = (int)ddc_in_bytes(in_fmt);
        return unit == 1 ? ((const uint8_t*)p)[i] : unit == 2 ? ((const uint16_t*)p)[i] : ((const uint32_t*)p)[i];
    }
    __device__ __forceinline__ Kept kept_history(const void* p, int64_t i) const { return kept_block(p, i); }
    __device__ __forceinline__ void keep(void* hist, int i, Kept v) const {
        const int unit = (int)ddc_in_bytes(in_fmt);
        if (unit == 1) ((uint8_t*)hist)[i] = (uint8_t)v;
        else if (unit == 2) ((uint16_t*)hist)[i] = (uint16_t)v;
        else ((uint32_t*)hist)[i] = v;
    }
};

// ... or a layout's frames, decoded here and nowhere else; the history holds decoded components, itself a layout.
struct DdcLayoutLoad {
    sdr::DdcLayout lay;
    typedef double2 Kept;
    static constexpr bool kTail = false;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_layout_load(p, i, lay, re, im); }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const {
        sdr::ddc_layout_load(p, i, sdr::ddc_layout_history(lay), re, im);
    }
    __device__ __forceinline__ Kept kept_block(const void* p, int64_t i) const {
        Kept v;
        block(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ Kept kept_history(const void* p, int64_t i) const {
        Kept v;
        history(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ void keep(void* hist, int i, Kept v) const { sdr::ddc_layout_history_store(hist, i, sdr::ddc_layout_history(lay), v.x, v.y); }
};

// ... or an array's: the K elements of a frame combined with the push's weights; the history holds combined inputs as cf64, and
// one out of the old history keeps the value it was combined to.
struct DdcArrayLoad {
    sdr::DdcLayout lay;
    sdr::DdcArray arr;
    typedef double2 Kept;
    static constexpr bool kTail = false;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_load(p, i, lay, arr, re, im); }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_history_load(p, i, re, im); }
    __device__ __forceinline__ Kept kept_block(const void* p, int64_t i) const {
        Kept v;
        block(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ Kept kept_history(const void* p, int64_t i) const {
        Kept v;
        history(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ void keep(void* hist, int i, Kept v) const { sdr::ddc_array_history_store(hist, i, v.x, v.y); }
};

// ... or a space-time array's: T frames of K elements combined per input, earlier frames than the push's first out of the raw
// tail.  The 64 weights are part of the argument: a queued push keeps the weights it was queued with.  The tail after a push:
// lane i < (T - 1) K of the history kernel takes element i % K of slot i / K -- out of the block, or, of a push shorter than T - 1
// frames, further up the old tail (a shift, ddc_stap_tail_next).
struct DdcStapLoad {
    sdr::DdcLayout lay;
    sdr::DdcArray arr;
    sdr::DdcStap stap;
    double* tail;
    typedef double2 Kept;
    static constexpr bool kTail = true;
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const {
        sdr::ddc_stap_load(p, tail, i, lay, arr, stap, re, im);
    }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_history_load(p, i, re, im); }
    // (the history kernel reads the parts through copies of their own: one 1.2 KiB argument read in place at some 600 points
    // is more than the compiler follows, and it would copy the whole argument to scratch memory, lane by lane)
    __device__ __forceinline__ Kept kept_block(const void* p, int64_t i) const {
        const sdr::DdcLayout l = lay;
        const sdr::DdcArray a = arr;
        const sdr::DdcStap s = stap;
        Kept v;
        sdr::ddc_stap_load(p, tail, i, l, a, s, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ Kept kept_history(const void* p, int64_t i) const {
        Kept v;
        history(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ void keep(void* hist, int i, Kept v) const { sdr::ddc_array_history_store(hist, i, v.x, v.y); }
    __device__ __forceinline__ double2 tail_next(const void* p, int64_t n_in, int i) const {
        double2 v = make_double2(0.0, 0.0);
        const int slot = i / arr.K;
        if (i < (stap.T - 1) * arr.K) sdr::ddc_stap_tail_next(p, tail, n_in, lay, arr, stap.T, slot, i - slot * arr.K, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ void tail_keep(int i, double2 v) const {
        const int slot = i / arr.K;
        if (i < (stap.T - 1) * arr.K) sdr::ddc_stap_tail_store(tail, slot, arr.K, i - slot * arr.K, v.x, v.y);
    }
};

// ... or those two with the weights of attached beam `b + 1`, a row of the table in device memory in place of the argument's
// own: the same statements on the same operands (ddc_array_combine, ddc_stap_load_table).  The raw tail is read, never kept: it
// holds elements, not beams, and the converter's own history launch brings it up to date behind the beams'.
struct DdcArrayBeamLoad {
    sdr::DdcLayout lay;
    sdr::DdcArray arr;
    const double* w;
    typedef double2 Kept;
    static constexpr bool kTail = false;
    __device__ __forceinline__ DdcArrayBeamLoad beam(int b) const {
        DdcArrayBeamLoad r = *this;
        r.w = w + (size_t)b * kDdcBeamWeightRow;
        return r;
    }
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const {
        sdr::ddc_array_combine(p, i, lay, arr, sdr::DdcArrayTableWeights{w}, re, im);
    }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_history_load(p, i, re, im); }
    __device__ __forceinline__ Kept kept_block(const void* p, int64_t i) const {
        Kept v;
        block(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ Kept kept_history(const void* p, int64_t i) const {
        Kept v;
        history(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ void keep(void* hist, int i, Kept v) const { sdr::ddc_array_history_store(hist, i, v.x, v.y); }
};

struct DdcStapBeamLoad {
    sdr::DdcLayout lay;
    sdr::DdcArray arr;
    int T;
    const double* tail;
    const double* w;
    typedef double2 Kept;
    static constexpr bool kTail = false;
    __device__ __forceinline__ DdcStapBeamLoad beam(int b) const {
        DdcStapBeamLoad r = *this;
        r.w = w + (size_t)b * kDdcBeamWeightRow;
        return r;
    }
    __device__ __forceinline__ void block(const void* __restrict__ p, int64_t i, double* re, double* im) const {
        sdr::ddc_stap_load_table(p, tail, i, lay, arr, T, w, re, im);
    }
    __device__ __forceinline__ void history(const void* __restrict__ p, int64_t i, double* re, double* im) const { sdr::ddc_array_history_load(p, i, re, im); }
    __device__ __forceinline__ Kept kept_block(const void* p, int64_t i) const {
        Kept v;
        block(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ Kept kept_history(const void* p, int64_t i) const {
        Kept v;
        history(p, i, &v.x, &v.y);
        return v;
    }
    __device__ __forceinline__ void keep(void* hist, int i, Kept v) const { sdr::ddc_array_history_store(hist, i, v.x, v.y); }
};

// The one place where a converter's kind becomes its loader: f(load) with the loader as the kernels take it, by value.
template <class F>
inline void ddc_with_loader(const sdr_ddc* d, F&& f) {
    switch (d->kind) {
        case kDdcKindStap: return f(DdcStapLoad{d->layout, d->array, d->stap, d->tail});
        case kDdcKindArray: return f(DdcArrayLoad{d->layout, d->array});
        case kDdcKindLayout: return f(DdcLayoutLoad{d->layout});
        default: return f(DdcFormatLoad{d->in_fmt});
    }
}

// ... and its beams' loader (d->kind >= kDdcKindArray).
template <class F>
inline void ddc_with_beam_loader(const sdr_ddc* d, F&& f) {
    if (d->kind == kDdcKindStap) return f(DdcStapBeamLoad{d->layout, d->array, d->stap.T, d->tail, d->beam_w});
    return f(DdcArrayBeamLoad{d->layout, d->array, d->beam_w});
}

inline int ddc_check(sdr_engine* e, const sdr_ddc* d) {
    if (!d) return sdr_fail(SDR_ERR_INVALID, "converter is NULL");
    if (d->engine != e) return sdr_fail(SDR_ERR_INVALID, "the converter belongs to another engine");
    return SDR_OK;
}

namespace sdr {

// ddc.hip: the one constructor behind the five sdr_ddc_create*: a converter of `kind` with interpolation L; `layout` from
// kDdcKindLayout on, `array` from kDdcKindArray on, stap_taps and stap_w ([stap_taps][K][2]) of kDdcKindStap, unread otherwise.
int ddc_create(sdr_engine* e, DdcKind kind, const sdr_ddc_cfg* cfg, int L, const sdr_ddc_layout* layout, const sdr_ddc_array* array, int stap_taps,
               const double* stap_w, sdr_ddc** out);

// ddc_beams.hip: every attachment of d released -- histories, events, the weight table (the caller has waited for the stream).
void ddc_beams_release(sdr_ddc* d);

}  // namespace sdr
