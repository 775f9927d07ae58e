// Host-side check of what an acquisition request means (sydr_amd/csrc/acq_request.h), built with `hipcc --cuda-host-only`
// (tests/test_acq_request.py; `make check-sanitize` runs it under the address and undefined-behaviour sanitizers).
//   acq_request_check            -> the samples per code at exact .5 cases (half-even), and every request that is wrong in ONE way
//                                   against the status its entry point has always answered, per flavour of the check; the text
//                                   names the ring before the slots.  "ok <cases>" and exit status 0, or the mismatches and 1
//   acq_request_check grid       -> reads "range step" pairs (hexadecimal floats) from standard input and prints the grid
//                                   length of each: the pytest side compares with len(np.arange(-R, R + 1, S))
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/acq_request.h"

using namespace sdr;

static int failures = 0, cases = 0;
static void expect(bool ok, const char* what) {
    ++cases;
    if (!ok) {
        printf("%s\n", what);
        ++failures;
    }
}

// an engine with a ring of 8000 samples and three slots: 1023 chips, nothing, 5000 chips
static const int32_t kCodeLen[3] = {1023, 0, 5000};
static AcqRequest good(const int32_t* slots) {
    AcqRequest r;
    r.ring = true, r.capacity = 8000, r.slots_allocated = true, r.n_slots = 3, r.code_len = kCodeLen;
    r.slots = slots, r.n_prn = 1, r.start = 0, r.fs = 4e6, r.doppler_range = 5000.0, r.doppler_step = 250.0, r.blocks = 2;
    return r;
}

static void single_faults(const AcqLimits& lim, const char* name, int grid_status, int length_status) {
    static const int32_t staged[1] = {0}, unstaged[1] = {1}, outside[1] = {3}, negative[1] = {-1};
    static std::vector<int32_t> many(65536, 0);
    AcqShape s;
    char what[200];
    auto check = [&](const AcqRequest& r, int status, const char* fault, const char* word) {
        const int rc = acq_request_check(r, lim, &s);
        snprintf(what, sizeof what, "%s, %s: status %d, expected %d, text \"%s\"", name, fault, rc, status, s.text);
        expect(rc == status && (rc == SDR_OK) == (s.text[0] == 0) && (!word || strstr(s.text, word)), what);
    };
    AcqRequest r = good(staged);
    check(r, SDR_OK, "nothing wrong", nullptr);
    expect(s.N == 4000 && s.spc == 4 && s.grid.nbins == 41 && s.grid.bin_start == -5000.0 && s.grid.bin_delta == 250.0 && s.chips == 1023,
           "the shape of a good request");
    r = good(staged), r.ring = false;
    check(r, SDR_ERR_STATE, "no ring", "ring");
    r = good(staged), r.slots_allocated = false;
    check(r, SDR_ERR_STATE, "no slots", "slots");
    r = good(staged), r.ring = false, r.slots_allocated = false;
    check(r, SDR_ERR_STATE, "neither: the ring is named first", "ring");
    r = good(staged), r.n_prn = 0;
    check(r, SDR_ERR_INVALID, "n_prn = 0", nullptr);
    for (double fs : {0.0, -4e6, (double)NAN, (double)INFINITY}) {
        r = good(staged), r.fs = fs;
        check(r, SDR_ERR_INVALID, "bad fs", nullptr);
    }
    r = good(staged), r.blocks = 0;
    check(r, SDR_ERR_INVALID, "no block", nullptr);
    for (double step : {0.0, -250.0, (double)NAN, (double)INFINITY}) {
        r = good(staged), r.doppler_step = step;
        check(r, SDR_ERR_INVALID, "bad step", nullptr);
    }
    for (double range : {-1.0, (double)NAN, (double)INFINITY}) {
        r = good(staged), r.doppler_range = range;
        check(r, SDR_ERR_INVALID, "bad range", nullptr);
    }
    r = good(staged), r.fs = 1000.0;          // one sample per code
    check(r, length_status, "a code of one sample", nullptr);
    r = good(staged), r.fs = 1e12, r.capacity = (int64_t)1 << 40;
    check(r, length_status, "a code of 10^9 samples", nullptr);
    r = good(staged), r.start = -1;
    check(r, SDR_ERR_RANGE, "start = -1", nullptr);
    r = good(staged), r.blocks = 3;           // 12000 of 8000 samples
    check(r, SDR_ERR_RANGE, "one block more than the ring holds", nullptr);
    r = good(staged), r.blocks = (int64_t)1 << 62;
    check(r, SDR_ERR_RANGE, "2^62 blocks", nullptr);
    for (const int32_t* slots : {unstaged, outside, negative}) {
        r = good(slots);
        check(r, SDR_ERR_INVALID, "a slot that is not staged", "not staged");
    }
    r = good(staged), r.doppler_range = 40000.0, r.doppler_step = 1.0;    // 80001 bins
    check(r, grid_status, "80001 bins", nullptr);
    r = good(many.data()), r.n_prn = 65536;
    check(r, grid_status, "65536 PRNs", nullptr);
    r = good(many.data()), r.n_prn = 65535;
    check(r, SDR_OK, "65535 PRNs", nullptr);
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "grid")) {
        double range, step;
        while (scanf("%la %la", &range, &step) == 2) printf("%d\n", acq_grid(range, step).nbins);
        return 0;
    }
    // samples per code = round(fs * 1023 / 1.023e6), Python's round: halves go to the even neighbour (fs / 1000 is exact here)
    expect(acq_samples_per_code(4000500.0) == 4000.0, "4000.5 -> 4000");
    expect(acq_samples_per_code(4001500.0) == 4002.0, "4001.5 -> 4002");
    expect(acq_samples_per_code(2500.0) == 2.0, "2.5 -> 2");
    expect(acq_samples_per_code(3500.0) == 4.0, "3.5 -> 4");
    expect(acq_samples_per_code(16.368e6) == 16368.0 && acq_samples_per_chip(16.368e6) == 16, "16.368 MHz");
    expect(acq_samples_per_chip(25e6) == 24 && acq_samples_per_chip(10e6) == 10 && acq_samples_per_chip(50e6) == 49, "samples per chip");
    // the grid's elements: start + k * ((start + step) - start)
    expect(acq_bin(5000.0, 250.0, 40) == 5000.0 && acq_bin(10.0, 3.0, 6) == 8.0, "grid elements");
    expect(acq_grid(5000.0, 250.0).nbins == 41 && acq_grid(5000.0, 300.0).nbins == 34 && acq_grid(10.0, 3.0).nbins == 7, "grid lengths");
    expect(acq_grid(1e300, 1e-300).nbins == 0 && acq_grid(0.0, 1e-12).nbins == 0, "a grid of more bins than an int holds is no grid");

    // the FFT searches (sdr_pcps, sdr_acq_deep, sdr_acq_deep_detect) and SerialSearch: where they differ, they keep differing
    single_faults(kAcqLimitsPcps, "pcps", SDR_ERR_UNSUPPORTED, SDR_ERR_UNSUPPORTED);
    single_faults(kAcqLimitsDeep, "deep", SDR_ERR_UNSUPPORTED, SDR_ERR_UNSUPPORTED);
    single_faults(kAcqLimitsSerial, "serial", SDR_ERR_INVALID, SDR_ERR_RANGE);
    {
        // SerialSearch alone: codes of one length, at most 4096 chips
        static const int32_t mixed[2] = {0, 2}, same[2] = {0, 0}, long_code[1] = {2};
        AcqShape s;
        AcqRequest r = good(mixed);
        r.n_prn = 2;
        expect(acq_request_check(r, kAcqLimitsSerial, &s) == SDR_ERR_INVALID && strstr(s.text, "one length"), "serial: two lengths");
        expect(acq_request_check(r, kAcqLimitsPcps, &s) == SDR_OK, "pcps: two lengths");
        r = good(same), r.n_prn = 2;
        expect(acq_request_check(r, kAcqLimitsSerial, &s) == SDR_OK && s.chips == 1023, "serial: one length");
        r = good(long_code);
        expect(acq_request_check(r, kAcqLimitsSerial, &s) == SDR_ERR_UNSUPPORTED, "serial: 5000 chips");
        expect(acq_request_check(r, kAcqLimitsDeep, &s) == SDR_OK, "deep: 5000 chips");
    }
    {
        // SerialSearch alone: the code holds every chip index trunc((ts*n)/tc), n < N, that a code period's samples reach --
        // 1023 at 4 MHz and at 1.023 MHz + 1 kHz, 1022 at 1.0 and 1.023 MHz; the rule follows the index, not the number 1023
        static const int32_t lens[4] = {1022, 1023, 1021, 4096};
        static const int32_t slot0[1] = {0}, slot1[1] = {1}, slot2[1] = {2}, slot3[1] = {3};
        AcqShape s;
        auto with = [&](const int32_t* slots, double fs) {
            AcqRequest r = good(slots);
            r.n_slots = 4, r.code_len = lens, r.fs = fs, r.doppler_range = 500.0, r.capacity = 1 << 20;
            return r;
        };
        expect(acq_request_check(with(slot0, 4e6), kAcqLimitsSerial, &s) == SDR_ERR_INVALID && strstr(s.text, "1022") &&
                   strstr(s.text, "1023"), "serial: 1022 chips at 4 MHz, the text names both numbers");
        expect(acq_request_check(with(slot0, 4e6), kAcqLimitsPcps, &s) == SDR_OK && s.text[0] == 0, "pcps: 1022 chips at 4 MHz");
        expect(acq_request_check(with(slot1, 4e6), kAcqLimitsSerial, &s) == SDR_OK && s.chips == 1023, "serial: 1023 chips at 4 MHz");
        expect(acq_request_check(with(slot3, 4e6), kAcqLimitsSerial, &s) == SDR_OK && s.chips == 4096, "serial: 4096 chips at 4 MHz");
        expect(acq_request_check(with(slot0, 1.0e6), kAcqLimitsSerial, &s) == SDR_OK && s.N == 1000 && s.chips == 1022,
               "serial: 1022 chips at 1.0 MHz (highest index 1021)");
        expect(acq_request_check(with(slot0, 1.023e6), kAcqLimitsSerial, &s) == SDR_OK && s.N == 1023,
               "serial: 1022 chips at 1.023 MHz (highest index 1021)");
        expect(acq_request_check(with(slot2, 1.0e6), kAcqLimitsSerial, &s) == SDR_ERR_INVALID && strstr(s.text, "1021") &&
                   strstr(s.text, "1022"), "serial: 1021 chips at 1.0 MHz");
        expect(acq_request_check(with(slot2, 1.023e6), kAcqLimitsSerial, &s) == SDR_ERR_INVALID, "serial: 1021 chips at 1.023 MHz");
        expect(acq_request_check(with(slot0, 16.368e6), kAcqLimitsSerial, &s) == SDR_ERR_INVALID, "serial: 1022 chips at 16.368 MHz");
        expect(acq_request_check(with(slot1, 16.368e6), kAcqLimitsSerial, &s) == SDR_OK, "serial: 1023 chips at 16.368 MHz");
        // a slot that is not staged is named before the length is looked at
        static const int32_t none[1] = {1};
        AcqRequest r = good(none);
        r.fs = 1.0e6;
        expect(acq_request_check(r, kAcqLimitsSerial, &s) == SDR_ERR_INVALID && strstr(s.text, "not staged"), "serial: unstaged slot");
    }
    {
        // sdr_pcps_spectra: no slots, the code length is the caller's
        AcqShape s;
        AcqRequest r = good(nullptr);
        r.slots_allocated = false, r.n_slots = 0, r.code_len = nullptr, r.n_code = 4000;
        expect(acq_request_check(r, kAcqLimitsPcps, &s) == SDR_OK && s.N == 4000, "spectra handed in");
        r.n_code = ((int64_t)1 << 24) + 1;
        expect(acq_request_check(r, kAcqLimitsPcps, &s) == SDR_ERR_UNSUPPORTED, "spectra of 2^24 + 1 samples");
    }
    if (failures) return 1;
    printf("ok %d\n", cases);
    return 0;
}
