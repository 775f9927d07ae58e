// What a request to sdr_pcps_coherent means and whether the engine can serve it (the contract in include/sydr_amd.h).  Host code
// only, no engine in sight, beside acq_request.h and secondary_request.h, whose pieces it is made of: the search side of the
// request is sdr_pcps_signal's zero-padded search of noncoh = n_periods blocks (acq_signal_check: ring, slots, chip rate, grid,
// code length, transform length, exclusion window, window inside the ring), the overlay side sdr_acq_secondary's (its limits of
// periods and chips, its chip check) -- shared with the stand-alone check tests/csrc/coherent_request_check.hip
// (`make check-sanitize`, tests/test_coherent.py).  Also here: how the (PRN, bin) units of a call are cut into chunks under the
// scratch budget (coherent_chunks).
#pragma once

#include "acq_request.h"
#include "secondary_request.h"

namespace sdr {

constexpr int kCohMaxBins = 64;          // K, frequencies of the fine grid
constexpr int kCohMaxCells = 4096;       // sec_len * K: the table P[h][k] of one cell (32 KB of LDS in the pick kernel)
constexpr int kCohMaxUnits = 32768;      // (PRN, bin) units of one chunk (a launch's grid.y)
constexpr int64_t kCohDefaultScratch = 2ll << 30;

struct CohRequest {
    AcqRequest acq;                     // the engine and the search side of the call (blocks is not read)
    const sdr_coh_cfg* cfg = nullptr;
    const int32_t* sec_rows = nullptr;  // [n_prn]
    const int8_t* sec_codes = nullptr;  // [n_sec][cfg->sec_len]
    int n_sec = 0;
    int K = 0;                          // sdr_acq_refine_bins(span_hz, step_hz): the one helper the grid's length comes from
    bool results = false;               // the results pointer is not NULL
};

struct CohShape {
    AcqShape acq;                       // N (samples per code), spc (the exclusion half-width), the Doppler grid; text
    AcqSignalShape sig;                 // N, T = 2N, window = (M + 1) * N
};

// SDR_OK: *s is filled; else s->acq.text says what is wrong (s->acq.grid is set as soon as the grid is known).
inline int coherent_request_check(const CohRequest& r, CohShape* s) {
    auto fail = [&](int status, const char* what) {
        snprintf(s->acq.text, sizeof s->acq.text, "%s", what);
        return status;
    };
    *s = CohShape{};
    if (!r.acq.ring) return fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (!r.acq.slots_allocated) return fail(SDR_ERR_STATE, "code slots not allocated");
    if (!r.cfg) return fail(SDR_ERR_INVALID, "NULL cfg");
    if (!r.results) return fail(SDR_ERR_INVALID, "results is NULL");
    if (!r.sec_rows) return fail(SDR_ERR_INVALID, "sec_rows is NULL");
    if (!r.sec_codes) return fail(SDR_ERR_INVALID, "sec_codes is NULL");
    const sdr_coh_cfg& c = *r.cfg;
    if (c.reserved[0] != 0 || c.reserved[1] != 0) return fail(SDR_ERR_INVALID, "non-zero reserved field");
    if (c.n_periods < 2 || c.n_periods > kSecMaxPeriods) {
        snprintf(s->acq.text, sizeof s->acq.text, "n_periods %d outside 2..%d", c.n_periods, kSecMaxPeriods);
        return SDR_ERR_INVALID;
    }
    if (c.sec_len < 2 || c.sec_len > kSecMaxLen) {
        snprintf(s->acq.text, sizeof s->acq.text, "sec_len %d outside 2..%d", c.sec_len, kSecMaxLen);
        return SDR_ERR_INVALID;
    }
    if (c.mode != SDR_SEC_PILOT && c.mode != SDR_SEC_DATA) return fail(SDR_ERR_INVALID, "mode is neither SDR_SEC_PILOT nor SDR_SEC_DATA");
    if (r.K <= 0 || !std::isfinite(c.span_hz) || !std::isfinite(c.step_hz)) return fail(SDR_ERR_INVALID, "bad fine frequency grid");
    // the search side: sdr_pcps_signal's zero-padded search of n_periods blocks
    sdr_acq_signal sig = {c.chip_rate_hz, 1, c.excl_samples, {0, 0}};
    if (int rc = acq_signal_check(r.acq, &sig, 1, c.n_periods, &s->acq, &s->sig)) return rc;
    if (r.n_sec < 1 || r.n_sec > r.acq.n_prn) {
        snprintf(s->acq.text, sizeof s->acq.text, "n_sec %d outside 1..n_prn = %d", r.n_sec, r.acq.n_prn);
        return SDR_ERR_INVALID;
    }
    if (int rc = secondary_chips_check(r.sec_codes, r.n_sec, c.sec_len, s->acq.text, sizeof s->acq.text)) return rc;
    for (int p = 0; p < r.acq.n_prn; ++p)
        if (r.sec_rows[p] < 0 || r.sec_rows[p] >= r.n_sec) {
            snprintf(s->acq.text, sizeof s->acq.text, "PRN entry %d: sec_row %d outside the %d rows of sec_codes", p, r.sec_rows[p], r.n_sec);
            return SDR_ERR_INVALID;
        }
    if (r.K > kCohMaxBins) {
        snprintf(s->acq.text, sizeof s->acq.text, "fine grid of %d frequencies (at most %d)", r.K, kCohMaxBins);
        return SDR_ERR_UNSUPPORTED;
    }
    if (c.sec_len * r.K > kCohMaxCells) {
        snprintf(s->acq.text, sizeof s->acq.text, "%d hypotheses x %d frequencies (at most %d cells)", c.sec_len, r.K, kCohMaxCells);
        return SDR_ERR_UNSUPPORTED;
    }
    return SDR_OK;
}

// ---- the cut of a call's n_prn * nbins units (unit u = p * nbins + b) into chunks whose scratch, [M][units][T] complex doubles,
// stays under `budget` bytes (<= 0: the default; never less than one unit).  A chunk is whole PRNs (bins == nbins), or, where
// the budget holds less than one PRN's bins, a run of bins of ONE PRN -- what one inverse sweep's (PRN, bin) numbering takes.
struct CohChunk {
    int prn0 = 0, prns = 0;             // PRNs [prn0, prn0 + prns)
    int bin0 = 0, bins = 0;             // bins [bin0, bin0 + bins) of each of them
    int units() const { return prns * bins; }
};
inline int64_t coherent_unit_bytes(int M, int T) { return (int64_t)M * T * 16; }
// units one chunk may hold
inline int coherent_chunk_units(int64_t budget, int M, int T) {
    const int64_t fit = (budget > 0 ? budget : kCohDefaultScratch) / coherent_unit_bytes(M, T);
    return (int)std::min<int64_t>(kCohMaxUnits, std::max<int64_t>(1, fit));
}
// the number of chunks; chunk i of them through coherent_chunk
inline int coherent_chunk_count(int cap, int n_prn, int nbins) {
    if (cap >= nbins) return (n_prn + cap / nbins - 1) / (cap / nbins);
    return n_prn * ((nbins + cap - 1) / cap);
}
inline CohChunk coherent_chunk(int cap, int n_prn, int nbins, int i) {
    CohChunk c;
    if (cap >= nbins) {
        const int per = cap / nbins;
        c.prn0 = i * per, c.prns = std::min(per, n_prn - c.prn0);
        c.bin0 = 0, c.bins = nbins;
    } else {
        const int per_prn = (nbins + cap - 1) / cap;
        c.prn0 = i / per_prn, c.prns = 1;
        c.bin0 = (i % per_prn) * cap, c.bins = std::min(cap, nbins - c.bin0);
    }
    return c;
}

}  // namespace sdr
