// Host-side check of what a request to sdr_acq_secondary means (sydr_amd/csrc/secondary_request.h), built with
// `hipcc --cuda-host-only` (tests/test_secondary.py; `make check-sanitize` runs it under the address and undefined-behaviour
// sanitizers): a good request and its shape, then every request that is wrong in ONE way against the status the contract in
// include/sydr_amd.h names, the limits at their last good and first bad values, and the order ring, slots, arguments.
// "ok <cases>" and exit status 0, or the mismatches and 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/secondary_request.h"

using namespace sdr;

static int failures = 0, cases = 0;
static void expect(bool ok, const char* what) {
    ++cases;
    if (!ok) {
        printf("%s\n", what);
        ++failures;
    }
}

// an engine with a ring of 400 000 samples, rows of 4200 words and three slots: 1023 chips, nothing, 4092 chips
static const int32_t kCodeLen[3] = {1023, 0, 4092};
static std::vector<int8_t> g_sec;
static std::vector<sdr_sec_item> g_items;

static SecRequest good() {
    g_sec.assign(2 * 20, 1);
    for (size_t q = 0; q < g_sec.size(); q += 3) g_sec[q] = -1;
    g_items.assign(2, sdr_sec_item{0, 0, 100, 1750.0, 1.023e6});
    g_items[1].sec_row = 1, g_items[1].start_sample = 400000 + 17;     // (indices are taken modulo the capacity)
    SecRequest r;
    r.ring = true, r.slots_allocated = true;
    r.g = RefineRing{400000, 3, kCodeLen, 4200};
    r.items = g_items.data(), r.n_items = 2, r.sec_codes = g_sec.data(), r.n_sec = 2, r.sec_len = 20;
    r.fs = 4e6, r.n_periods = 40, r.n_segments = 4, r.span_hz = 125.0, r.step_hz = 5.0, r.K = 51, r.mode = SDR_SEC_PILOT;
    r.results = true;
    return r;
}

static void check(const SecRequest& r, int status, const char* fault, const char* word = nullptr) {
    SecShape s;
    std::vector<RefineItemDev> dev(r.n_items > 0 && r.n_items < 100000 ? r.n_items : 1);
    const int rc = secondary_request_check(r, &s, dev.data());
    char what[400];
    snprintf(what, sizeof what, "%s: status %d, expected %d, text \"%s\"", fault, rc, status, s.text);
    expect(rc == status && (rc == SDR_OK) == (s.text[0] == 0) && (!word || strstr(s.text, word)), what);
}

int main() {
    {
        SecRequest r = good();
        SecShape s;
        RefineItemDev dev[2];
        expect(secondary_request_check(r, &s, dev) == SDR_OK && s.text[0] == 0, "a good request");
        expect(dev[0].N == 4000 && dev[0].slot == 0 && dev[0].base == 100 && dev[0].f0 == 1750.0 && dev[0].code_step == 1.023e6 / 4e6 &&
                   dev[0].sec_row == 0 && dev[1].sec_row == 1 && dev[1].base == 17,
               "the items of a good request");
        expect(dev[0].lut_words == 1023 + 8 && s.max_words == 1031, "the replica of one period, in words");
        expect(secondary_request_check(r, &s, nullptr) == SDR_OK, "no item list wanted");
    }
    SecRequest r = good();
    r.ring = false;
    check(r, SDR_ERR_STATE, "no ring", "ring");
    r = good(), r.slots_allocated = false;
    check(r, SDR_ERR_STATE, "no slots", "slots");
    r = good(), r.ring = false, r.slots_allocated = false, r.items = nullptr;
    check(r, SDR_ERR_STATE, "neither, and no items: the ring is named first", "ring");
    r = good(), r.items = nullptr;
    check(r, SDR_ERR_INVALID, "items NULL");
    r = good(), r.sec_codes = nullptr;
    check(r, SDR_ERR_INVALID, "sec_codes NULL", "sec_codes");
    r = good(), r.results = false;
    check(r, SDR_ERR_INVALID, "results NULL", "results");
    for (int n : {0, -1, 65536}) {
        r = good(), r.n_items = n;
        check(r, SDR_ERR_INVALID, "n_items outside 1..65535");
    }
    for (double fs : {0.0, -4e6, (double)NAN, (double)INFINITY}) {
        r = good(), r.fs = fs;
        check(r, SDR_ERR_INVALID, "bad fs");
    }
    for (int m : {1, 0, -3, 129}) {
        r = good(), r.n_periods = m, r.n_segments = 1;
        check(r, SDR_ERR_INVALID, "n_periods outside 2..128", "n_periods");
    }
    for (int m : {2, 128}) {      // (128 periods of 4000 samples: the ring must hold them)
        r = good(), r.n_periods = m, r.n_segments = 16, r.g.capacity = 600000;
        check(r, SDR_OK, "n_periods 2 and 128");
    }
    for (int sg : {0, -1, 65}) {
        r = good(), r.n_periods = 2, r.n_segments = sg;
        check(r, SDR_ERR_INVALID, "n_segments outside 1..64", "n_segments");
    }
    r = good(), r.n_periods = 32, r.n_segments = 64;
    check(r, SDR_OK, "32 x 64 segments");
    r = good(), r.n_periods = 33, r.n_segments = 64;
    check(r, SDR_ERR_UNSUPPORTED, "33 x 64 segments", "segments");
    for (int ls : {1, 0, -1, 129}) {
        r = good(), r.sec_len = ls;
        check(r, SDR_ERR_INVALID, "sec_len outside 2..128", "sec_len");
    }
    {
        std::vector<int8_t> longest(128, 1), shortest(2, -1);
        r = good(), r.sec_codes = longest.data(), r.n_sec = 1, r.sec_len = 128, g_items[1].sec_row = 0;
        check(r, SDR_OK, "sec_len 128");
        r = good(), r.sec_codes = shortest.data(), r.n_sec = 1, r.sec_len = 2, g_items[1].sec_row = 0;
        check(r, SDR_OK, "sec_len 2");
    }
    for (int ns : {0, -1, 3}) {
        r = good(), r.n_sec = ns;
        check(r, SDR_ERR_INVALID, "n_sec outside 1..n_items", "n_sec");
    }
    for (int mode : {-1, 2}) {
        r = good(), r.mode = mode;
        check(r, SDR_ERR_INVALID, "mode outside 0..1", "mode");
    }
    r = good(), r.mode = SDR_SEC_DATA;
    check(r, SDR_OK, "mode 1");
    for (int k : {0, -1}) {
        r = good(), r.K = k;
        check(r, SDR_ERR_INVALID, "no grid", "grid");
    }
    for (double v : {(double)NAN, (double)INFINITY}) {
        r = good(), r.span_hz = v;
        check(r, SDR_ERR_INVALID, "span not finite", "grid");
        r = good(), r.step_hz = v;
        check(r, SDR_ERR_INVALID, "step not finite", "grid");
    }
    r = good(), r.K = 4096;       // (the check takes K as it is given: an even K is the helper's business)
    check(r, SDR_OK, "K = 4096");
    r = good(), r.K = 4097;
    check(r, SDR_ERR_UNSUPPORTED, "K = 4097", "frequencies");
    for (int8_t chip : {(int8_t)0, (int8_t)2, (int8_t)-2, (int8_t)127, (int8_t)-128}) {
        r = good(), g_sec[39] = chip;
        check(r, SDR_ERR_INVALID, "a chip that is neither +1 nor -1", "neither");
    }
    for (int row : {-1, 2}) {
        r = good(), g_items[1].sec_row = row;
        check(r, SDR_ERR_INVALID, "a bad sec_row", "sec_row");
    }
    for (int slot : {1, 3, -1}) {
        r = good(), g_items[0].code_slot = slot;
        check(r, SDR_ERR_INVALID, "a slot that is not staged", "not staged");
    }
    for (double v : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
        r = good(), g_items[1].carrier_hz = v;
        check(r, SDR_ERR_INVALID, "a carrier that is not finite", "item 1");
    }
    for (double v : {0.0, -1.023e6, (double)NAN, (double)INFINITY}) {
        r = good(), g_items[0].code_hz = v;
        check(r, SDR_ERR_INVALID, "a bad code_hz", "item 0");
    }
    r = good(), g_items[1].start_sample = -1;
    check(r, SDR_ERR_RANGE, "a negative start_sample", "negative");
    r = good(), r.n_periods = 101;                  // 404 000 of 400 000 samples
    check(r, SDR_ERR_RANGE, "a window longer than the ring", "ring holds");
    r = good(), r.n_periods = 100;
    check(r, SDR_OK, "a window as long as the ring");
    r = good(), r.fs = 2e3, r.n_periods = 2, r.n_segments = 4;      // a code period of 2 samples
    check(r, SDR_ERR_UNSUPPORTED, "n_segments > N", "segments in a code period");
    r = good(), r.fs = 1e3, g_items[0].code_hz = 1e9, g_items[1].code_hz = 1e9;   // a code period of no sample
    check(r, SDR_ERR_RANGE, "a code period of no sample");
    r = good(), r.fs = 4e15, r.n_periods = 2, r.g.capacity = (int64_t)1 << 62;    // a code period of 4e12 samples
    check(r, SDR_ERR_UNSUPPORTED, "a code period of more than 2^30 samples", "2^30");
    r = good(), r.g.lut_stride = 1030;              // the row is a word short of a period of 1023 chips
    check(r, SDR_ERR_UNSUPPORTED, "a staged row too short", "chips");
    r = good(), g_items[0].code_slot = 2, g_items[0].code_hz = 1.023e6, r.n_periods = 2, r.g.lut_stride = 1 << 20,
    r.fs = 4.092e6;
    check(r, SDR_OK, "4092 chips");
    {
        static const int32_t big[1] = {20000};
        r = good(), r.g = RefineRing{(int64_t)1 << 30, 1, big, 1 << 20}, r.n_periods = 2;
        check(r, SDR_ERR_UNSUPPORTED, "a code period beyond the LDS", "chips");
    }
    if (failures) return 1;
    printf("ok %d\n", cases);
    return 0;
}
