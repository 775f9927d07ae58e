// Host-side check of what sdr_pcps_signal's request means (sydr_amd/csrc/acq_request.h acq_signal_check), built with
// `hipcc --cuda-host-only` (tests/test_acq_signal_request.py; `make check-sanitize` runs it under the address and
// undefined-behaviour sanitizers).
//   acq_signal_check            -> every refusal of include/sydr_amd.h in its order, each a request wrong in ONE way; N, T, the
//                                  exclusion width and the window for awkward rates; the C/A descriptor against acq_request_check
//                                  on the old request; the old request's own answers; the plan of a padded search (pcps_plan.h:
//                                  the map route, a map of N columns, buffers for T) beside the unchanged circular one.
//                                  "ok <cases>" and exit status 0, or the mismatches and 1
//   acq_signal_check lengths    -> reads "fs chips chip_rate" triples (hexadecimal floats, an int) from standard input and prints N
//                                  of each: the pytest side compares with NumPy's rint(fs * chips / chip_rate)
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/acq_request.h"
#include "../../sydr_amd/csrc/pcps_plan.h"

using namespace sdr;

static int failures = 0, cases = 0;
static void expect(bool ok, const char* what) {
    ++cases;
    if (!ok) {
        printf("%s\n", what);
        ++failures;
    }
}

// an engine with a ring of 80000 samples and four slots: 1023 chips, nothing, 4092 chips, 1023 chips
static const int32_t kCodeLen[4] = {1023, 0, 4092, 1023};
static AcqRequest good(const int32_t* slots, int n_prn = 1) {
    AcqRequest r;
    r.ring = true, r.capacity = 80000, r.slots_allocated = true, r.n_slots = 4, r.code_len = kCodeLen;
    r.slots = slots, r.n_prn = n_prn, r.start = 0, r.fs = 4e6, r.doppler_range = 5000.0, r.doppler_step = 250.0, r.blocks = 1;
    return r;
}
static sdr_acq_signal ca(int pad = 0, int excl = 0) {
    sdr_acq_signal g = {1.023e6, pad, excl, {0, 0}};
    return g;
}

static AcqShape s;
static AcqSignalShape g;
static void refused(const AcqRequest& r, const sdr_acq_signal* sig, int coh, int noncoh, int status, const char* fault, const char* word) {
    char what[240];
    const int rc = acq_signal_check(r, sig, coh, noncoh, &s, &g);
    snprintf(what, sizeof what, "%s: status %d, expected %d, text \"%s\"", fault, rc, status, s.text);
    expect(rc == status && (rc == SDR_OK) == (s.text[0] == 0) && (!word || strstr(s.text, word)), what);
    if (rc != SDR_OK) expect(g.N == 0 && g.T == 0 && g.window == 0, "a refused request leaves no shape");
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "lengths")) {
        double fs, rate;
        int chips;
        while (scanf("%la %d %la", &fs, &chips, &rate) == 3) printf("%.0f\n", acq_signal_samples_per_code(fs, chips, rate));
        return 0;
    }
    static const int32_t one[1] = {0}, pair[2] = {0, 3}, mixed[2] = {0, 2}, long_code[1] = {2}, unstaged[1] = {1}, outside[1] = {4},
                         negative[1] = {-1};
    sdr_acq_signal sig = ca();

    // ---- the refusals, in the header's order
    AcqRequest r = good(one);
    refused(r, &sig, 1, 2, SDR_OK, "nothing wrong", nullptr);
    expect(g.N == 4000 && g.T == 4000 && g.excl == 4 && g.pad == 0 && g.chips == 1023 && g.window == 8000 && g.chip_rate == 1.023e6 &&
               s.N == 4000 && s.spc == 4 && s.grid.nbins == 41,
           "the shape of a good circular request");
    refused(r, nullptr, 1, 1, SDR_ERR_INVALID, "NULL sig", "NULL");
    for (double rate : {0.0, -1.023e6, (double)NAN, (double)INFINITY, -(double)INFINITY}) {
        sig = ca(), sig.chip_rate_hz = rate;
        refused(r, &sig, 1, 1, SDR_ERR_INVALID, "bad chip rate", "chip rate");
    }
    for (int pad : {-1, 2, 1 << 30}) {
        sig = ca(pad);
        refused(r, &sig, 1, 1, SDR_ERR_INVALID, "pad outside 0..1", "pad");
    }
    sig = ca(0, -1);
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "negative excl_samples", "excl");
    sig = ca(), sig.reserved[0] = 1;
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "reserved[0]", "reserved");
    sig = ca(), sig.reserved[1] = -1;
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "reserved[1]", "reserved");
    sig = ca(1);
    refused(r, &sig, 2, 1, SDR_ERR_INVALID, "pad = 1 with coh = 2", "coh = 1");
    refused(r, &sig, 1, 1, SDR_OK, "pad = 1 with coh = 1", nullptr);
    expect(g.N == 4000 && g.T == 8000 && g.pad == 1 && g.window == 8000 && s.N == 4000, "the shape of a good padded request");
    sig = ca();
    r = good(mixed, 2);
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "slots of different lengths", "one length");
    r = good(pair, 2);
    refused(r, &sig, 1, 1, SDR_OK, "two slots of one length", nullptr);
    r = good(one);
    sig = ca(0, 2000);                       // 2 * 2000 + 1 >= 4000
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "2 * excl + 1 = N + 1", "excl");
    sig = ca(0, 1999);                       // 3999 < 4000
    refused(r, &sig, 1, 1, SDR_OK, "2 * excl + 1 = N - 1", nullptr);
    expect(g.excl == 1999 && s.spc == 1999, "the caller's exclusion width");
    sig = ca(0, 2147483647);
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "excl_samples = INT_MAX", "excl");
    sig = ca();
    // every cause sdr_pcps names
    r = good(one), r.ring = false;
    refused(r, &sig, 1, 1, SDR_ERR_STATE, "no ring", "ring");
    r = good(one), r.slots_allocated = false;
    refused(r, &sig, 1, 1, SDR_ERR_STATE, "no slots", "slots");
    r = good(one), r.ring = false, r.slots_allocated = false;
    refused(r, nullptr, 1, 1, SDR_ERR_STATE, "neither, and no sig: the ring is named first", "ring");
    r = good(nullptr);
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "NULL slots", "NULL");
    r = good(one), r.n_prn = 0;
    refused(r, &sig, 1, 1, SDR_ERR_INVALID, "n_prn = 0", nullptr);
    for (double fs : {0.0, -4e6, (double)NAN, (double)INFINITY}) {
        r = good(one), r.fs = fs;
        refused(r, &sig, 1, 1, SDR_ERR_INVALID, "bad fs", nullptr);
    }
    r = good(one);
    refused(r, &sig, 0, 1, SDR_ERR_INVALID, "coh = 0", nullptr);
    refused(r, &sig, 1, 0, SDR_ERR_INVALID, "noncoh = 0", nullptr);
    refused(r, &sig, 1, -3, SDR_ERR_INVALID, "noncoh = -3", nullptr);
    for (double step : {0.0, -250.0, (double)NAN, (double)INFINITY}) {
        r = good(one), r.doppler_step = step;
        refused(r, &sig, 1, 1, SDR_ERR_INVALID, "bad step", "grid");
    }
    for (double range : {-1.0, (double)NAN, (double)INFINITY}) {
        r = good(one), r.doppler_range = range;
        refused(r, &sig, 1, 1, SDR_ERR_INVALID, "bad range", "grid");
    }
    for (const int32_t* slots : {unstaged, outside, negative}) {
        r = good(slots);
        refused(r, &sig, 1, 1, SDR_ERR_INVALID, "a slot that is not staged", "not staged");
    }
    // SDR_ERR_UNSUPPORTED: T outside 2 .. 2^24
    r = good(one), r.fs = 1000.0;            // N = 1: no second peak either way; T = 1 circular
    refused(r, &sig, 1, 1, SDR_ERR_UNSUPPORTED, "a code of one sample, circular", nullptr);
    r = good(one), r.fs = 400.0;             // N = 0
    refused(r, &sig, 1, 1, SDR_ERR_UNSUPPORTED, "a code of no sample", nullptr);
    r = good(one), r.fs = 1e12, r.capacity = (int64_t)1 << 40;
    refused(r, &sig, 1, 1, SDR_ERR_UNSUPPORTED, "a code of 10^9 samples", nullptr);
    r = good(one), r.fs = 16777216e3, r.capacity = (int64_t)1 << 40;       // N = 2^24 exactly
    refused(r, &sig, 1, 1, SDR_OK, "N = 2^24 circular", nullptr);
    expect(g.N == 1 << 24 && g.T == 1 << 24, "N = T = 2^24");
    sig = ca(1);
    refused(r, &sig, 1, 1, SDR_ERR_UNSUPPORTED, "N = 2^24 padded: T = 2^25", nullptr);
    r = good(one), r.fs = 8388608e3, r.capacity = (int64_t)1 << 40;        // N = 2^23, T = 2^24
    refused(r, &sig, 1, 1, SDR_OK, "T = 2^24 padded", nullptr);
    expect(g.N == 1 << 23 && g.T == 1 << 24 && g.window == (int64_t)1 << 24, "N = 2^23, T = 2^24");
    sig = ca();
    r = good(one), r.doppler_range = 40000.0, r.doppler_step = 1.0;        // 80001 bins
    refused(r, &sig, 1, 1, SDR_ERR_UNSUPPORTED, "80001 bins", "grid");
    {
        static std::vector<int32_t> many(65536, 0);
        r = good(many.data(), 65536);
        refused(r, &sig, 1, 1, SDR_ERR_UNSUPPORTED, "65536 PRNs", "grid");
        r = good(many.data(), 65535);
        refused(r, &sig, 1, 1, SDR_OK, "65535 PRNs", nullptr);
    }
    // SDR_ERR_RANGE: the window against the ring (80000 samples = 20 periods of 4000)
    r = good(one);
    refused(r, &sig, 4, 5, SDR_OK, "circular, 20 periods", nullptr);
    expect(g.window == 80000, "coh * noncoh * N");
    refused(r, &sig, 3, 7, SDR_ERR_RANGE, "circular, 21 periods", "ring holds");
    refused(r, &sig, 1 << 30, 1 << 30, SDR_ERR_RANGE, "circular, 2^60 periods", nullptr);
    sig = ca(1);
    refused(r, &sig, 1, 19, SDR_OK, "padded, 19 blocks: 20 periods", nullptr);
    expect(g.window == 80000, "(noncoh + 1) * N");
    refused(r, &sig, 1, 20, SDR_ERR_RANGE, "padded, 20 blocks: 21 periods", "ring holds");
    refused(r, &sig, 1, 2147483647, SDR_ERR_RANGE, "padded, INT_MAX blocks", nullptr);
    r = good(one), r.start = -1;
    refused(r, &sig, 1, 1, SDR_ERR_RANGE, "start = -1", nullptr);
    r = good(one), r.start = 79999;
    refused(r, &sig, 1, 1, SDR_OK, "a window across the ring's end", nullptr);

    // ---- N, T and the exclusion width for awkward rates (half-even; the chip rate and the code length are parameters)
    struct Len {
        double fs, rate;
        const int32_t* slots;
        int excl_in, N, excl;
    };
    const Len lens[] = {
        {4.092e6, 1.023e6, long_code, 0, 16368, 4},     // E1-like: 4092 chips in 4 ms
        {4.0e6, 2.046e6, long_code, 4, 8000, 4},        // 4092 half chips at twice the rate: 2 ms
        {2.038e6, 1.023e6, one, 0, 2038, 2},            // 2 x 1019: chirp-z
        {4000500.0, 1.023e6, one, 0, 4000, 4},          // 4000.5 -> 4000
        {4001500.0, 1.023e6, one, 0, 4002, 4},          // 4001.5 -> 4002
        {10.23e6, 10.23e6, one, 0, 1023, 1},            // one sample per chip
        {50e6, 10.23e6, long_code, 0, 20000, 5},        // 4.8876 samples per chip
        {5.5e6, 1.023e6, one, 0, 5500, 5},              // 5.376 -> 5
        {3.5805e6, 1.023e6, one, 0, 3580, 4},           // 3580.5 -> 3580, 3.5 -> 4
    };
    for (const Len& l : lens) {
        char what[120];
        for (int pad = 0; pad < 2; ++pad) {
            r = good(l.slots), r.fs = l.fs;
            sig = ca(pad, l.excl_in), sig.chip_rate_hz = l.rate;
            const int rc = acq_signal_check(r, &sig, 1, 1, &s, &g);
            snprintf(what, sizeof what, "fs %.1f rate %.1f pad %d: rc %d N %d T %d excl %d", l.fs, l.rate, pad, rc, g.N, g.T, g.excl);
            expect(rc == SDR_OK && g.N == l.N && g.T == l.N * (1 + pad) && g.excl == l.excl && s.N == l.N && s.spc == l.excl &&
                       g.window == (int64_t)l.N * (1 + pad),
                   what);
        }
    }

    // ---- the C/A descriptor on 1023-chip slots answers the old check's N, spc and grid, rate by rate
    for (double fs : {4e6, 10e6, 25e6, 50e6, 16.368e6, 4000500.0, 4001500.0, 5.001e6, 2.038e6, 2500.0, 3500.0}) {
        AcqShape old;
        r = good(pair, 2), r.fs = fs, r.capacity = (int64_t)1 << 30, r.blocks = 6;
        sig = ca();
        const int rc_old = acq_request_check(r, kAcqLimitsPcps, &old);
        const int rc = acq_signal_check(r, &sig, 2, 3, &s, &g);
        char what[120];
        snprintf(what, sizeof what, "C/A descriptor at %.1f Hz: rc %d / %d, N %d / %d, spc %d / %d", fs, rc, rc_old, g.N, old.N, g.excl, old.spc);
        expect(rc == SDR_OK && rc_old == SDR_OK && g.N == old.N && g.T == old.N && s.N == old.N && s.spc == old.spc && g.excl == old.spc &&
                   s.grid.nbins == old.grid.nbins && s.grid.bin_start == old.grid.bin_start && s.grid.bin_delta == old.grid.bin_delta &&
                   g.window == 6 * (int64_t)old.N && g.chip_rate == 1.023e6,
               what);
    }

    // ---- the old request keeps its answers (tests/csrc/acq_request_check.hip has them all; the ones next to the additions)
    {
        AcqShape old;
        r = good(one), r.blocks = 2;
        expect(acq_request_check(r, kAcqLimitsPcps, &old) == SDR_OK && old.N == 4000 && old.spc == 4 && old.grid.nbins == 41 && old.chips == 1023,
               "old: a good request");
        r = good(mixed, 2);
        expect(acq_request_check(r, kAcqLimitsPcps, &old) == SDR_OK && acq_request_check(r, kAcqLimitsSerial, &old) == SDR_ERR_INVALID,
               "old: two lengths are the FFT searches' business, not SerialSearch's");
        r = good(long_code), r.fs = 4.092e6;
        expect(acq_request_check(r, kAcqLimitsPcps, &old) == SDR_OK && old.N == 4092 && old.spc == 4,
               "old: a 4092-chip slot is still searched as 1 ms of C/A");
        r = good(one), r.blocks = 21;
        expect(acq_request_check(r, kAcqLimitsPcps, &old) == SDR_ERR_RANGE, "old: 21 periods of 20");
        expect(acq_samples_per_code(4000500.0) == 4000.0 && acq_samples_per_chip(50e6) == 49, "old: rounding");
    }
    // ---- the plan: a padded search is the map route over transforms of T with a map of N columns; the default is the old plan
    {
        using namespace pcps;
        const PcpsSwitches sw;
        const size_t cplx = 2 * sizeof(double);
        // indices only, one block: circular runs map-free, padded does not
        const PcpsPlan c = plan_pcps(sw, 16368, 4, 4.092e6, 9, -1000.0, 250.0, 1, 1, 32, false);
        const PcpsPlan d = plan_pcps(sw, 16368, 4, 4.092e6, 9, -1000.0, 250.0, 1, 1, 32, false, 16368, 1.023e6);
        const PcpsPlan p = plan_pcps(sw, 32736, 4, 4.092e6, 9, -1000.0, 250.0, 1, 1, 32, false, 16368, 1.023e6);
        expect(c.route == ROUTE_SWEEPS && c.cols == 16368 && c.chip_rate == 1.023e6 && c.map_bytes == (size_t)32 * 16368 * sizeof(double),
               "plan: the circular search as it was");
        expect(d.route == c.route && d.cols == c.cols && d.prn_chunk == c.prn_chunk && d.work_bytes == c.work_bytes && d.map_bytes == c.map_bytes &&
                   d.part_bytes == c.part_bytes && d.fwd_bytes == c.fwd_bytes,
               "plan: cols = N handed in is the default");
        expect(p.route == ROUTE_MAP && p.N == 32736 && p.cols == 16368 && p.xf.four.ok && p.xf.four.N1 == 176 && p.xf.four.N2 == 186 && !p.M &&
                   !p.overlap && !p.done_words && !p.sh.P,
               "plan: padded, 32736 = 176 x 186 on the map route");
        expect(p.map_bytes == (size_t)32 * 9 * 16368 * sizeof(double) && p.code_bytes == (size_t)32 * 32736 * cplx &&
                   p.fwd_bytes == (size_t)32 * 32736 * cplx && p.work_bytes == (size_t)p.prn_chunk * 9 * 32736 * cplx && p.prn_chunk == 32,
               "plan: padded, a map of N columns and buffers for transforms of T");
        // N = 10 000 padded never takes the fused 10 MHz search; chirp-z and radix-pass lengths
        const PcpsPlan f = plan_pcps(sw, 10000, 10, 5e6, 41, -5000.0, 250.0, 1, 2, 8, false, 5000, 1.023e6);
        expect(f.route == ROUTE_MAP && plan_pcps(sw, 10000, 10, 10e6, 41, -5000.0, 250.0, 1, 2, 8, false).route == ROUTE_FUSED10K,
               "plan: T = 10 000 padded stays off the fused search");
        const PcpsPlan z = plan_pcps(sw, 4076, 2, 2.038e6, 9, -1000.0, 250.0, 1, 3, 2, true, 2038, 1.023e6);
        expect(z.route == ROUTE_MAP && z.M == 8192 && z.map_bytes == (size_t)2 * 9 * 2038 * sizeof(double), "plan: 4076 = 4 x 1019 through chirp-z");
        const PcpsPlan w = plan_pcps(sw, 400000, 49, 50e6, 9, -1000.0, 250.0, 1, 2, 32, false, 200000, 1.023e6);
        expect(w.route == ROUTE_MAP && !w.xf.four.ok && !w.M && w.xf.radices.size() == 8, "plan: 400 000 has no four-step split: eight radix passes");
    }
    if (failures) return 1;
    printf("ok %d\n", cases);
    return 0;
}
