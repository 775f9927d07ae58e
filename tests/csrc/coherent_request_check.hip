// Host-side check of what a request to sdr_pcps_coherent means (sydr_amd/csrc/coherent_request.h), built with
// `hipcc --cuda-host-only` (tests/test_coherent.py; `make check-sanitize` runs it under the address and undefined-behaviour
// sanitizers): a good request and its shape, then every request that is wrong in ONE way against the status the contract in
// include/sydr_amd.h names, the limits at their last good and first bad values, the order ring, slots, arguments -- and the
// cut of a call's units into chunks: every unit in exactly one chunk, in ascending order, no chunk above the budget.
// "ok <cases>" and exit status 0, or the mismatches and 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/coherent_request.h"

using namespace sdr;

static int failures = 0, cases = 0;
static void expect(bool ok, const char* what) {
    ++cases;
    if (!ok) {
        printf("%s\n", what);
        ++failures;
    }
}

// an engine with a ring of 400 000 samples and four slots: 1023 chips, nothing, 4092 chips, 1023 chips
static const int32_t kCodeLen[4] = {1023, 0, 4092, 1023};
static std::vector<int8_t> g_sec;
static std::vector<int32_t> g_slots, g_rows;
static sdr_coh_cfg g_cfg;

static CohRequest good() {
    g_sec.assign(2 * 20, 1);
    for (size_t q = 0; q < g_sec.size(); q += 3) g_sec[q] = -1;
    g_slots = {0, 3}, g_rows = {0, 1};
    g_cfg = sdr_coh_cfg{1.023e6, 125.0, 25.0, 20, 20, SDR_SEC_PILOT, 0, {0, 0}};
    CohRequest r;
    r.acq.ring = true, r.acq.capacity = 400000, r.acq.slots_allocated = true, r.acq.n_slots = 4, r.acq.code_len = kCodeLen;
    r.acq.slots = g_slots.data(), r.acq.n_prn = 2, r.acq.start = 1234, r.acq.fs = 4e6, r.acq.doppler_range = 500.0,
    r.acq.doppler_step = 250.0;
    r.cfg = &g_cfg, r.sec_rows = g_rows.data(), r.sec_codes = g_sec.data(), r.n_sec = 2, r.K = 11, r.results = true;
    return r;
}

static void check(const CohRequest& r, int status, const char* fault, const char* word = nullptr) {
    CohShape s;
    const int rc = coherent_request_check(r, &s);
    char what[400];
    snprintf(what, sizeof what, "%s: status %d, expected %d, text \"%s\"", fault, rc, status, s.acq.text);
    expect(rc == status && (rc == SDR_OK) == (s.acq.text[0] == 0) && (!word || strstr(s.acq.text, word)), what);
}

static void check_cut(int64_t budget, int M, int T, int n_prn, int nbins, int want_chunks, const char* what) {
    const int cap = coherent_chunk_units(budget, M, T);
    const int n = coherent_chunk_count(cap, n_prn, nbins);
    int next = 0;      // the unit the next chunk has to begin with
    bool ok = cap >= 1 && cap <= kCohMaxUnits && (want_chunks < 0 || n == want_chunks);
    for (int i = 0; i < n && ok; ++i) {
        const CohChunk c = coherent_chunk(cap, n_prn, nbins, i);
        ok = c.prns >= 1 && c.bins >= 1 && c.units() <= cap && c.prn0 * nbins + c.bin0 == next &&
             (c.bins == nbins ? c.bin0 == 0 : c.prns == 1 && c.bin0 + c.bins <= nbins) && c.prn0 + c.prns <= n_prn;
        if (budget > 0 && c.units() > 1) ok = ok && (int64_t)c.units() * coherent_unit_bytes(M, T) <= budget;
        next += c.units();
    }
    expect(ok && next == n_prn * nbins, what);
}

int main() {
    {
        CohRequest r = good();
        CohShape s;
        expect(coherent_request_check(r, &s) == SDR_OK && s.acq.text[0] == 0, "a good request");
        expect(s.sig.N == 4000 && s.sig.T == 8000 && s.sig.window == 21 * 4000 && s.acq.spc == 4 && s.acq.grid.nbins == 5 &&
                   s.acq.grid.bin_start == -500.0 && s.acq.grid.bin_delta == 250.0 && s.sig.chip_rate == 1.023e6,
               "the shape of a good request");
    }
    CohRequest r = good();
    r.acq.ring = false;
    check(r, SDR_ERR_STATE, "no ring", "ring");
    r = good(), r.acq.slots_allocated = false;
    check(r, SDR_ERR_STATE, "no slots", "slots");
    r = good(), r.acq.ring = false, r.acq.slots_allocated = false, r.cfg = nullptr;
    check(r, SDR_ERR_STATE, "neither, and no cfg: the ring is named first", "ring");
    r = good(), r.cfg = nullptr;
    check(r, SDR_ERR_INVALID, "cfg NULL", "cfg");
    r = good(), r.results = false;
    check(r, SDR_ERR_INVALID, "results NULL", "results");
    r = good(), r.sec_rows = nullptr;
    check(r, SDR_ERR_INVALID, "sec_rows NULL", "sec_rows");
    r = good(), r.sec_codes = nullptr;
    check(r, SDR_ERR_INVALID, "sec_codes NULL", "sec_codes");
    r = good(), r.acq.slots = nullptr;
    check(r, SDR_ERR_INVALID, "code_slots NULL", "code_slots");
    for (int q = 0; q < 2; ++q) {
        r = good(), g_cfg.reserved[q] = 1;
        check(r, SDR_ERR_INVALID, "a reserved field that is not 0", "reserved");
    }
    // ---- the overlay side
    for (int m : {1, 0, -3, 129}) {
        r = good(), g_cfg.n_periods = m;
        check(r, SDR_ERR_INVALID, "n_periods outside 2..128", "n_periods");
    }
    for (int m : {2, 128}) {      // (129 periods of 4000 samples: the ring must hold them)
        r = good(), g_cfg.n_periods = m, r.acq.capacity = 600000;
        check(r, SDR_OK, "n_periods 2 and 128");
    }
    for (int ls : {1, 0, -1, 129}) {
        r = good(), g_cfg.sec_len = ls;
        check(r, SDR_ERR_INVALID, "sec_len outside 2..128", "sec_len");
    }
    {
        std::vector<int8_t> longest(128, 1), shortest(2, -1);
        r = good(), r.sec_codes = longest.data(), r.n_sec = 1, g_cfg.sec_len = 128, g_rows[1] = 0;
        check(r, SDR_OK, "sec_len 128");
        r = good(), r.sec_codes = shortest.data(), r.n_sec = 1, g_cfg.sec_len = 2, g_rows[1] = 0;
        check(r, SDR_OK, "sec_len 2");
    }
    for (int ns : {0, -1, 3}) {
        r = good(), r.n_sec = ns;
        check(r, SDR_ERR_INVALID, "n_sec outside 1..n_prn", "n_sec");
    }
    for (int mode : {-1, 2}) {
        r = good(), g_cfg.mode = mode;
        check(r, SDR_ERR_INVALID, "mode outside 0..1", "mode");
    }
    r = good(), g_cfg.mode = SDR_SEC_DATA;
    check(r, SDR_OK, "mode 1");
    for (int k : {0, -1}) {
        r = good(), r.K = k;
        check(r, SDR_ERR_INVALID, "no grid", "grid");
    }
    for (double v : {(double)NAN, (double)INFINITY}) {
        r = good(), g_cfg.span_hz = v;
        check(r, SDR_ERR_INVALID, "span not finite", "grid");
        r = good(), g_cfg.step_hz = v;
        check(r, SDR_ERR_INVALID, "step not finite", "grid");
    }
    r = good(), r.K = 1;
    check(r, SDR_OK, "K = 1");
    r = good(), r.K = 64;         // (the check takes K as it is given: an even K is the helper's business)
    check(r, SDR_OK, "K = 64");
    r = good(), r.K = 65;
    check(r, SDR_ERR_UNSUPPORTED, "K = 65", "frequencies");
    {
        std::vector<int8_t> longest(128, 1);
        r = good(), r.sec_codes = longest.data(), r.n_sec = 1, g_cfg.sec_len = 128, g_rows[1] = 0, r.K = 32;
        check(r, SDR_OK, "128 x 32 cells");
        r.K = 33;
        check(r, SDR_ERR_UNSUPPORTED, "128 x 33 cells", "cells");
        g_cfg.sec_len = 64, r.K = 64;
        check(r, SDR_OK, "64 x 64 cells");
        g_cfg.sec_len = 65;
        check(r, SDR_ERR_UNSUPPORTED, "65 x 64 cells", "cells");
    }
    for (int8_t chip : {(int8_t)0, (int8_t)2, (int8_t)-2, (int8_t)127, (int8_t)-128}) {
        r = good(), g_sec[39] = chip;
        check(r, SDR_ERR_INVALID, "a chip that is neither +1 nor -1", "neither");
    }
    for (int row : {-1, 2}) {
        r = good(), g_rows[1] = row;
        check(r, SDR_ERR_INVALID, "a bad sec_row", "sec_row");
    }
    // ---- the search side: sdr_pcps_signal's causes
    for (double v : {0.0, -1.023e6, (double)NAN, (double)INFINITY}) {
        r = good(), g_cfg.chip_rate_hz = v;
        check(r, SDR_ERR_INVALID, "a bad chip rate", "chip rate");
    }
    r = good(), g_cfg.excl_samples = -1;
    check(r, SDR_ERR_INVALID, "negative excl_samples", "excl_samples");
    r = good(), g_cfg.excl_samples = 1999;
    check(r, SDR_OK, "excl_samples 1999 of 4000");
    r = good(), g_cfg.excl_samples = 2000;
    check(r, SDR_ERR_INVALID, "excl_samples 2000 of 4000", "covers");
    for (int n : {0, -1}) {
        r = good(), r.acq.n_prn = n;
        check(r, SDR_ERR_INVALID, "no PRN", "PRN");
    }
    for (double fs : {0.0, -4e6, (double)NAN, (double)INFINITY}) {
        r = good(), r.acq.fs = fs;
        check(r, SDR_ERR_INVALID, "bad fs");
    }
    r = good(), r.acq.doppler_step = 0.0;
    check(r, SDR_ERR_INVALID, "no Doppler grid", "grid");
    r = good(), r.acq.doppler_range = (double)NAN;
    check(r, SDR_ERR_INVALID, "no Doppler grid", "grid");
    for (int slot : {1, 4, -1}) {
        r = good(), g_slots[1] = slot;
        check(r, SDR_ERR_INVALID, "a slot that is not staged", "not staged");
    }
    r = good(), g_slots[1] = 2;
    check(r, SDR_ERR_INVALID, "codes of two lengths", "one length");
    r = good(), r.acq.start = -1;
    check(r, SDR_ERR_RANGE, "a negative start_sample", "ring holds");
    r = good(), g_cfg.n_periods = 100;                // 101 x 4000 of 400 000 samples
    check(r, SDR_ERR_RANGE, "a window longer than the ring", "ring holds");
    r = good(), g_cfg.n_periods = 99;
    check(r, SDR_OK, "a window as long as the ring");
    r = good(), r.acq.fs = 1e3, g_cfg.chip_rate_hz = 1e9;      // a code period of no sample
    check(r, SDR_ERR_UNSUPPORTED, "a code period of no sample", "transform length");
    r = good(), r.acq.fs = 8388608.0, g_cfg.chip_rate_hz = 1023.0, r.acq.capacity = (int64_t)1 << 40;   // N = 2^23, T = 2^24
    check(r, SDR_OK, "T = 2^24");
    r = good(), r.acq.fs = 8388609.0, g_cfg.chip_rate_hz = 1023.0, r.acq.capacity = (int64_t)1 << 40;
    check(r, SDR_ERR_UNSUPPORTED, "T = 2^24 + 2", "transform length");
    r = good(), r.acq.doppler_range = 65535.0 * 0.5, r.acq.doppler_step = 1.0;
    check(r, SDR_ERR_UNSUPPORTED, "more than 65535 bins", "grid too large");

    // ---- the cut into chunks
    const int64_t unit = coherent_unit_bytes(20, 8000);
    expect(unit == 2560000, "a unit at N = 4000, M = 20");
    expect(coherent_unit_bytes(20, 50000) == 16000000, "a unit at N = 25 000, M = 20");
    check_cut(0, 20, 8000, 3, 5, 1, "the default budget: one chunk");
    check_cut(2 * unit, 20, 8000, 1, 5, 3, "two units: one PRN's five bins in three chunks");
    check_cut(2 * unit + 1, 20, 8000, 1, 5, 3, "two units and a byte");
    check_cut(1, 20, 8000, 2, 5, 10, "less than a unit: a unit per chunk");
    check_cut(5 * unit, 20, 8000, 3, 5, 3, "five units: a PRN per chunk");
    check_cut(5 * unit - 1, 20, 8000, 3, 5, 6, "a byte less: four bins, then one, per PRN");
    check_cut(12 * unit, 20, 8000, 5, 5, 3, "twelve units: two whole PRNs per chunk");
    check_cut(0, 2, 2, 65535, 9, -1, "more units than a launch takes: chunks of at most 32768");
    for (int cap_units = 1; cap_units <= 23; ++cap_units)
        for (int n_prn = 1; n_prn <= 4; ++n_prn)
            for (int nbins = 1; nbins <= 7; ++nbins) check_cut(cap_units * unit, 20, 8000, n_prn, nbins, -1, "a cut");
    if (failures) return 1;
    printf("ok %d\n", cases);
    return 0;
}
