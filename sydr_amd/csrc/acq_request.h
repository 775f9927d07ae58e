// What an acquisition request means and whether the engine can serve it, derived in ONE place for sdr_pcps, sdr_pcps_spectra,
// sdr_pcps_signal (acq_signal_check, below: chip rate, code period, zero-padded search; tests/csrc/acq_signal_check.hip),
// sdr_acq_deep, sdr_acq_deep_detect, sdr_serial_search (pcps.hip, serial_search.hip), sdr_acq_deep_shift (acq_deep.hip) and
// sdr_pcps_bins: samples per code and per chip from the sampling rate, the Doppler grid with np.arange's semantics, and the one
// check of ring present / slots present / request sane / start and extent inside the ring / slots staged / grid limits.  Host
// code only, no engine in sight: the check takes what it needs of the engine as plain values, answers a status of
// include/sydr_amd.h and leaves its text in the request's shape (the caller hands it to sdr_fail) -- shared with the
// stand-alone check tests/csrc/acq_request_check.hip (`make check-sanitize`, tests/test_acq_request.py).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/sydr_amd.h"

namespace sdr {

// samplesPerCode (channel_l1ca_kaplan.py:186) and samplesPerCodeChip (:205-206), Python round = half-even
inline double acq_samples_per_code(double fs) { return std::nearbyint(fs * 1023.0 / 1.023e6); }
inline int acq_samples_per_chip(double fs) { return (int)std::nearbyint(fs / 1.023e6); }

// The Doppler grid np.arange(-R, R+1, S): len = ceil((stop - start)/step) bins, element k = start + k*delta with
// delta = (start+step) - start.  nbins == 0: no grid (a step that is not positive, a negative or NaN range, more bins than an int).
struct AcqGrid {
    int nbins = 0;
    double bin_start = 0.0, bin_delta = 0.0;
};
inline double acq_bin_delta(double doppler_range, double doppler_step) { return (-doppler_range + doppler_step) - -doppler_range; }
// element k of the grid (whatever its length: sdr_acq_deep_shift answers for any bin)
inline double acq_bin(double doppler_range, double doppler_step, int k) {
    return -doppler_range + (double)k * acq_bin_delta(doppler_range, doppler_step);
}
inline AcqGrid acq_grid(double doppler_range, double doppler_step) {
    AcqGrid g;
    if (!(doppler_step > 0.0) || !(doppler_range >= 0.0)) return g;
    const double len = std::ceil(((doppler_range + 1.0) - (-doppler_range)) / doppler_step);
    g.nbins = len > 0 && len <= 2147483647.0 ? (int)len : 0;
    g.bin_start = -doppler_range;
    g.bin_delta = acq_bin_delta(doppler_range, doppler_step);
    return g;
}

// Where the searches differ, and keep differing.
struct AcqLimits {
    const char* who;          // names the search in the ring-range text
    int grid_status;          // more than 65535 bins or PRNs: the FFT searches SDR_ERR_UNSUPPORTED, SerialSearch SDR_ERR_INVALID
    int length_status;        // samples per code outside 2 .. 2^24: SDR_ERR_UNSUPPORTED, SerialSearch SDR_ERR_RANGE
    bool one_code_length;     // SerialSearch: the staged codes of a request have one length, which holds every chip
                              // index trunc((ts*n)/tc) of a code period's samples, n < N ...
    int max_chips;            // ... of at most this many chips (0: any)
};
constexpr AcqLimits kAcqLimitsPcps = {"acquisition", SDR_ERR_UNSUPPORTED, SDR_ERR_UNSUPPORTED, false, 0};
constexpr AcqLimits kAcqLimitsDeep = {"deep acquisition", SDR_ERR_UNSUPPORTED, SDR_ERR_UNSUPPORTED, false, 0};
constexpr AcqLimits kAcqLimitsSerial = {"serial search", SDR_ERR_INVALID, SDR_ERR_RANGE, true, 4096};

struct AcqRequest {
    // of the engine
    bool ring = false;                  // the IQ ring is allocated, of
    int64_t capacity = 0;               // ... this many samples
    bool slots_allocated = false;
    int n_slots = 0;
    const int32_t* code_len = nullptr;  // [n_slots] chips staged per slot, <= 0: none
    // of the call
    const int32_t* slots = nullptr;     // [n_prn] slot numbers; nullptr: the caller hands in code spectra of n_code samples
    int64_t n_code = 0;
    int n_prn = 0;
    int64_t start = 0;
    double fs = 0.0, doppler_range = 0.0, doppler_step = 0.0;
    int64_t blocks = 1;                 // code periods read from `start` on (coh * noncoh), >= 1
};

struct AcqShape {
    int N = 0, spc = 0;                 // samples per code, per chip
    AcqGrid grid;                       // (set as soon as the grid is known, also where a later check refuses the request)
    int chips = 0;                      // one_code_length: that length
    char text[160] = {0};               // what is wrong, for sdr_last_error
};

inline int acq_request_check(const AcqRequest& r, const AcqLimits& lim, AcqShape* s) {
    auto fail = [&](int status, const char* what) {
        snprintf(s->text, sizeof s->text, "%s", what);
        return status;
    };
    *s = AcqShape{};
    if (!r.ring) return fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (r.slots && !r.slots_allocated) return fail(SDR_ERR_STATE, "code slots not allocated");
    if (r.n_prn <= 0) return fail(SDR_ERR_INVALID, "no PRN to search");
    if (!(r.fs > 0.0) || r.fs - r.fs != 0.0 || r.blocks < 1) return fail(SDR_ERR_INVALID, "bad fs / integration counts");
    s->grid = acq_grid(r.doppler_range, r.doppler_step);
    if (s->grid.nbins <= 0) return fail(SDR_ERR_INVALID, "empty Doppler grid");
    const double n_code = r.slots ? acq_samples_per_code(r.fs) : (double)r.n_code;
    if (!(n_code >= 2.0 && n_code <= (double)(1 << 24))) {
        snprintf(s->text, sizeof s->text, "samples per code %.0f unsupported", n_code);
        return lim.length_status;
    }
    s->N = (int)n_code;
    s->spc = acq_samples_per_chip(r.fs);
    if (r.start < 0 || r.blocks > r.capacity / s->N) {
        snprintf(s->text, sizeof s->text, "%s needs %lld x %d samples from %lld, ring holds %lld", lim.who, (long long)r.blocks, s->N,
                 (long long)r.start, (long long)r.capacity);
        return SDR_ERR_RANGE;
    }
    for (int i = 0; i < r.n_prn && r.slots; ++i) {
        const int slot = r.slots[i];
        if (slot < 0 || slot >= r.n_slots || r.code_len[slot] <= 0) {
            snprintf(s->text, sizeof s->text, "PRN entry %d: code slot %d is not staged", i, slot);
            return SDR_ERR_INVALID;
        }
        if (lim.one_code_length && s->chips && r.code_len[slot] != s->chips)
            return fail(SDR_ERR_INVALID, "the search needs codes of one length");
        s->chips = r.code_len[slot];
    }
    if (lim.one_code_length) {
        // the highest chip a code period's samples land on, with the kernel's own expression (ss_chipsum_kernel): a code
        // that ends before it has no chip for those samples (the reference raises IndexError there)
        const double ts = 1.0 / r.fs, tc = 1.0 / 1.023e6;
        const int reach = (int)std::trunc((ts * (double)(s->N - 1)) / tc) + 1;
        if (s->chips < reach) {
            snprintf(s->text, sizeof s->text, "codes of %d chips, the samples of a code period reach %d chips", s->chips, reach);
            return SDR_ERR_INVALID;
        }
    }
    if (lim.max_chips && s->chips > lim.max_chips) {
        snprintf(s->text, sizeof s->text, "codes longer than %d chips", lim.max_chips);
        return SDR_ERR_UNSUPPORTED;
    }
    if (s->grid.nbins > 65535 || r.n_prn > 65535) return fail(lim.grid_status, "grid too large");
    return SDR_OK;
}

// ---- sdr_pcps_signal: the same request with the signal's chip rate, its code period and the zero-padded search.  The code
// length L is the slots' own (one length per call), so the slots are looked at before the lengths:
//   N = nearbyint(fs * L / chip_rate) samples per code, T = N * (1 + pad) the transform length, excl the exclusion half-width
//   window = coh * noncoh * N samples (pad = 0), (noncoh + 1) * N (pad = 1: blocks advance by N and read 2N)
// {1.023e6, 0, 0} on 1023-chip slots answers acq_request_check's N and spc: the same expressions in the same order.
struct AcqSignalShape {
    int N = 0, T = 0, excl = 0, pad = 0, chips = 0;
    double chip_rate = 0.0;
    int64_t window = 0;                 // samples read from `start` on
};
inline double acq_signal_samples_per_code(double fs, int chips, double chip_rate) {
    return std::nearbyint(fs * (double)chips / chip_rate);
}

// (r.blocks is not read: coh and noncoh are taken apart here)
inline int acq_signal_check(const AcqRequest& r, const sdr_acq_signal* sig, int coh, int noncoh, AcqShape* s, AcqSignalShape* g) {
    auto fail = [&](int status, const char* what) {
        snprintf(s->text, sizeof s->text, "%s", what);
        return status;
    };
    *s = AcqShape{};
    *g = AcqSignalShape{};
    if (!r.ring) return fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!r.slots_allocated) return fail(SDR_ERR_STATE, "code slots not allocated");
    if (!sig) return fail(SDR_ERR_INVALID, "NULL signal descriptor");
    if (!(sig->chip_rate_hz > 0.0) || sig->chip_rate_hz - sig->chip_rate_hz != 0.0)
        return fail(SDR_ERR_INVALID, "chip rate not finite or not positive");
    if (sig->pad < 0 || sig->pad > 1) return fail(SDR_ERR_INVALID, "pad outside 0..1");
    if (sig->excl_samples < 0) return fail(SDR_ERR_INVALID, "negative excl_samples");
    if (sig->reserved[0] != 0 || sig->reserved[1] != 0) return fail(SDR_ERR_INVALID, "non-zero reserved field");
    if (!r.slots) return fail(SDR_ERR_INVALID, "code_slots is NULL");
    if (r.n_prn <= 0) return fail(SDR_ERR_INVALID, "no PRN to search");
    if (!(r.fs > 0.0) || r.fs - r.fs != 0.0 || coh < 1 || noncoh < 1) return fail(SDR_ERR_INVALID, "bad fs / integration counts");
    if (sig->pad == 1 && coh != 1) return fail(SDR_ERR_INVALID, "the zero-padded search takes coh = 1");
    s->grid = acq_grid(r.doppler_range, r.doppler_step);
    if (s->grid.nbins <= 0) return fail(SDR_ERR_INVALID, "empty Doppler grid");
    for (int i = 0; i < r.n_prn; ++i) {
        const int slot = r.slots[i];
        if (slot < 0 || slot >= r.n_slots || r.code_len[slot] <= 0) {
            snprintf(s->text, sizeof s->text, "PRN entry %d: code slot %d is not staged", i, slot);
            return SDR_ERR_INVALID;
        }
        if (s->chips && r.code_len[slot] != s->chips) return fail(SDR_ERR_INVALID, "the search needs codes of one length");
        s->chips = r.code_len[slot];
    }
    const double n_code = acq_signal_samples_per_code(r.fs, s->chips, sig->chip_rate_hz);
    const double t_len = n_code * (double)(1 + sig->pad);
    if (!(n_code >= 1.0 && t_len >= 2.0 && t_len <= (double)(1 << 24))) {
        snprintf(s->text, sizeof s->text, "transform length %.0f unsupported", t_len);
        return SDR_ERR_UNSUPPORTED;
    }
    const int N = (int)n_code;
    const double excl = sig->excl_samples ? (double)sig->excl_samples : std::nearbyint(r.fs / sig->chip_rate_hz);
    // (an exclusion window as wide as the row leaves no second peak; the default's never is where a code has four chips or more)
    if (2.0 * excl + 1.0 >= n_code) return fail(SDR_ERR_INVALID, "2 * excl_samples + 1 covers the code period");
    const int64_t blocks = sig->pad ? (int64_t)noncoh + 1 : (int64_t)coh * noncoh;
    if (r.start < 0 || blocks > r.capacity / N) {
        snprintf(s->text, sizeof s->text, "acquisition needs %lld x %d samples from %lld, ring holds %lld", (long long)blocks, N,
                 (long long)r.start, (long long)r.capacity);
        return SDR_ERR_RANGE;
    }
    if (s->grid.nbins > 65535 || r.n_prn > 65535) return fail(SDR_ERR_UNSUPPORTED, "grid too large");
    s->N = N;
    s->spc = (int)excl;
    g->N = N, g->T = N * (1 + sig->pad), g->excl = (int)excl, g->pad = sig->pad, g->chips = s->chips;
    g->chip_rate = sig->chip_rate_hz;
    g->window = blocks * N;
    return SDR_OK;
}

}  // namespace sdr
