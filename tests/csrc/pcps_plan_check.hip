// Host-side check of the planner of an acquisition search (sydr_amd/csrc/pcps_plan.h), built with `hipcc --cuda-host-only`
// (tests/test_pcps_plan.py; `make check-sanitize` runs it under the address and undefined-behaviour sanitizers).
//   - prints one line per request with every field of the plan: tests/test_pcps_plan.py compares the output with
//     tests/golden/pcps_plans.txt, which was recorded from the planner as it stood inside pcps.hip before it became a header;
//   - asserts, whatever that file says, the decisions that matter: where the fused sweep takes over from the two-kernel
//     sweeps at 25 / 50 / 10 MHz, the shared-spectra classes of the shipped grids, the chirp-z length of N = 5001, and the
//     sweep sizes of a 32-PRN search on one and on two streams.
// Exit status 0, or the first failed assertion and 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/acq_request.h"
#include "../../sydr_amd/csrc/pcps_plan.h"

using namespace pcps;

struct Request {
    double fs;
    double range, step;
    int coh, noncoh, n_prn;
    bool want_map;
    const char* sw;      // the one switch that is not at its default ("-": none; "fused+ovl": pcps_fused = 0 and pcps_no_overlap = 1)
};

static PcpsSwitches switches(const char* sw) {
    PcpsSwitches s;
    if (!strcmp(sw, "fused") || !strcmp(sw, "fused+ovl")) s.fused = false;
    if (!strcmp(sw, "no_fast")) s.no_fast = true;
    if (!strcmp(sw, "force_map")) s.force_map = true;
    if (!strcmp(sw, "no_overlap") || !strcmp(sw, "fused+ovl")) s.no_overlap = true;
    if (!strcmp(sw, "no_shared")) s.no_shared_spectra = true;
    if (!strcmp(sw, "chunk5")) s.prn_chunk = 5;
    if (!strcmp(sw, "prof")) s.prof = true;
    return s;
}

static PcpsPlan plan(const Request& r) {
    const sdr::AcqGrid g = sdr::acq_grid(r.range, r.step);
    return plan_pcps(switches(r.sw), (int)sdr::acq_samples_per_code(r.fs), sdr::acq_samples_per_chip(r.fs), r.fs, g.nbins, g.bin_start,
                     g.bin_delta, r.coh, r.noncoh, r.n_prn, r.want_map);
}

static void print(const Request& r, const PcpsPlan& p) {
    static const char* const route[] = {"fused10k", "fused", "sweeps", "map"};
    static const char* const fast[] = {"none", "25k", "n"};
    // (bytes: tbytes fwd work code code2 map csum part res pinned blu blu_work)
    printf("fs=%.0f grid=%.0f/%.0f int=%dx%d prn=%d map=%d sw=%s | N=%d bins=%d four=%dx%d route=%s terms=%d chunk=%d overlap=%d "
           "PqH=%d/%d/%d M=%d fast=%s/%s rec=%d/%d/%d bytes=%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu done=%d\n",
           r.fs, r.range, r.step, r.coh, r.noncoh, r.n_prn, (int)r.want_map, r.sw, p.N, p.nbins, p.xf.four.N1, p.xf.four.N2,
           route[p.route], p.terms, p.prn_chunk, (int)p.overlap, p.sh.P, p.sh.q, p.sh.H, p.M, fast[p.xf.fast], fast[p.xm.fast],
           p.records_sweep, p.records_per_prn, p.records_second, p.tbytes, p.fwd_bytes, p.work_bytes, p.code_bytes, p.code2_bytes,
           p.map_bytes, p.csum_bytes, p.part_bytes, p.res_bytes, p.pinned_bytes, p.blu_bytes, p.blu_work_bytes, (int)p.done_words);
}

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

int main() {
    // fs = 5.001 MHz: N = 5001 = 3 x 1667, a prime factor above 64 -- the chirp-z route
    const double rates[] = {4e6, 10e6, 16.368e6, 25e6, 50e6, 5.001e6};
    const double grids[][2] = {{5000.0, 250.0}, {5000.0, 300.0}, {10.0, 3.0}};     // 41, 34 and 7 bins
    const int pairs[][2] = {{1, 1}, {1, 3}, {2, 1}, {2, 2}};
    std::vector<Request> rq;
    // indices and ratio only, one block: both sides of where a route takes over (fused: 256 units -- 6 | 7, 7 | 8, 36 | 37 PRNs
    // at 25 MHz, 3 | 4, 18 | 19 at 50 MHz; fused 10 MHz: 32 units -- 4 | 5 PRNs over 7 bins)
    for (double fs : rates)
        for (const auto& g : grids)
            for (int n_prn : {3, 4, 5, 6, 7, 8, 18, 19, 36, 37})
                if (fs != 5.001e6 || n_prn == 3 || n_prn == 37) rq.push_back({fs, g[0], g[1], 1, 1, n_prn, false, "-"});
    // map wanted or not, every integration
    for (double fs : rates)
        for (const auto& c : pairs)
            for (bool want_map : {false, true})
                rq.push_back({fs, 5000.0, 250.0, c[0], c[1], 32, want_map, "-"});
    // each switch on its own (and the two that together give the one-stream sweeps of the planner's own comment)
    for (const char* sw : {"fused", "no_fast", "force_map", "no_overlap", "no_shared", "chunk5", "prof", "fused+ovl"})
        for (double fs : {4e6, 10e6, 25e6, 50e6})
            for (int n_prn : {6, 7, 32}) rq.push_back({fs, 5000.0, 250.0, 1, 1, n_prn, false, sw});
    // sweeps that fill the Infinity Cache budget of two streams (100 MB: 39 | 40 PRNs at 4 MHz) and of one (200 MB: 79 | 80),
    // a sweep of 65535 transforms (1598 | 1599 PRNs x 41 bins), a work buffer of 8 GiB (261 | 262 PRNs at 50 MHz, map wanted)
    for (int n_prn : {39, 40, 79, 80, 1598, 1599}) {
        rq.push_back({4e6, 5000.0, 250.0, 1, 1, n_prn, false, "-"});
        rq.push_back({4e6, 5000.0, 250.0, 1, 1, n_prn, false, "no_overlap"});
    }
    for (int n_prn : {261, 262}) rq.push_back({50e6, 5000.0, 250.0, 1, 1, n_prn, true, "-"});
    for (const Request& r : rq) print(r, plan(r));

    auto at = [](double fs, double range, double step, int n_prn, const char* sw) {
        return plan({fs, range, step, 1, 1, n_prn, false, sw});
    };
    // 25 MHz x 41 bins: 6 PRNs (246 transforms) -> sweeps, 7 PRNs (287) -> fused, terms 1
    EXPECT(at(25e6, 5000.0, 250.0, 6, "-").route == ROUTE_SWEEPS);
    EXPECT(at(25e6, 5000.0, 250.0, 7, "-").route == ROUTE_FUSED && at(25e6, 5000.0, 250.0, 7, "-").terms == 1);
    // 50 MHz x 41 bins: 3 PRNs -> sweeps, 4 PRNs (328 units) -> fused, terms 2
    EXPECT(at(50e6, 5000.0, 250.0, 3, "-").route == ROUTE_SWEEPS);
    EXPECT(at(50e6, 5000.0, 250.0, 4, "-").route == ROUTE_FUSED && at(50e6, 5000.0, 250.0, 4, "-").terms == 2);
    // 10 MHz x 7 bins: 4 PRNs (28) -> sweeps, 5 PRNs (35) -> fused 10k
    EXPECT(at(10e6, 10.0, 3.0, 4, "-").route == ROUTE_SWEEPS);
    EXPECT(at(10e6, 10.0, 3.0, 5, "-").route == ROUTE_FUSED10K);
    // 250 Hz grid at 25 or 10 MHz -> P = 4, q = 1, H = 10; 300 Hz at 10 MHz -> P = 10, q = 3, H = 9
    for (double fs : {25e6, 10e6}) {
        const PcpsPlan p = at(fs, 5000.0, 250.0, 32, "-");
        EXPECT(p.sh.P == 4 && p.sh.q == 1 && p.sh.H == 10);
    }
    {
        const PcpsPlan p = at(10e6, 5000.0, 300.0, 32, "-");
        EXPECT(p.sh.P == 10 && p.sh.q == 3 && p.sh.H == 9);
    }
    // N = 5001 -> M = 10125, map route
    {
        const PcpsPlan p = at(5.001e6, 5000.0, 250.0, 2, "-");
        EXPECT(p.N == 5001 && p.M == 10125 && p.route == ROUTE_MAP);
        EXPECT(chirpz_length(5001) == 10125);
    }
    // 25 MHz x 41 bins x 32 PRNs with pcps_fused off -> sweeps of 6 PRNs on two streams; with pcps_no_overlap also set ->
    // 11 PRNs per sweep (the 11 / 11 / 10 of the planner's own comment)
    {
        const PcpsPlan p = at(25e6, 5000.0, 250.0, 32, "fused");
        EXPECT(p.route == ROUTE_SWEEPS && p.prn_chunk == 6 && p.overlap);
        const PcpsPlan o = at(25e6, 5000.0, 250.0, 32, "fused+ovl");
        EXPECT(o.route == ROUTE_SWEEPS && o.prn_chunk == 11 && !o.overlap);
    }
    // the result block: sizes and places as the searches have always had them
    {
        alignas(8) char base[4 * 5 * 8 + 2 * 5 * 4];
        const ResultBlock b = result_block(5, true, true, true, base);
        EXPECT((char*)b.bin == base && (char*)b.code == base + 40 && (char*)b.ratio == base + 80 && (char*)b.value == base + 120);
        EXPECT((char*)b.slots == base + 160 && (char*)b.done == base + 180 && b.bytes == sizeof base);
        const ResultBlock c = result_block(5, false, true, false, base);
        EXPECT(c.value == nullptr && (char*)c.slots == base + 120 && c.done == nullptr && c.bytes == 140);
        EXPECT(result_block(1, false, true, false, nullptr).bytes == 3 * sizeof(double) + sizeof(int32_t));
    }
    if (failures) return 1;
    fprintf(stderr, "ok %zu requests\n", rq.size());
    return 0;
}
