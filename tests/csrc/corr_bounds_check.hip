// The run walk of sdr_corr_profile (sydr_amd/csrc/corr_bounds.h), compiled for the host alone (`hipcc --cuda-host-only
// -ffp-contract=off`: no device code, no GPU): prints the runs -- (first sample, padded index) pairs -- the kernel's lanes
// would walk, for tests/test_corr_profile.py to hold against the run-length encoding of NumPy's chip indices.
//   usage: corr_bounds_check [text] < parameter sets, one per line: n rem_code code_step spacing (C99 hex floats)
//   stdout, per set: int32 count, then count x (int32 first sample, int32 padded index) -- native byte order;
//   with `text`: "first:index" pairs, a line per set.
// The walk is driven the way the kernel drives it: the epoch in segments of 4096 samples, each segment cut into pieces for the
// lanes that share a tap, every piece started from an exact evaluation of its first sample; pieces that continue a run are
// merged here, so the output is the run-length encoding whatever the cut.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/corr_bounds.h"

using namespace sdr;

int main(int argc, char** argv) {
    const bool text = argc > 1 && !strcmp(argv[1], "text");
    std::vector<int32_t> runs;
    int n;
    double rem_code, code_step, spacing;
    long sets = 0;
    while (scanf("%d %la %la %la", &n, &rem_code, &code_step, &spacing) == 4) {
        if (n < 1) return 2;
        const CorrTap t = corr_tap(n, rem_code, code_step, spacing);
        runs.clear();
        const int lanes = 1 << (sets % 7);   // 1 .. 64 lanes per tap, by turns
        for (int s0 = 0; s0 < n; s0 += 4096) {
            const int len = n - s0 < 4096 ? n - s0 : 4096;
            for (int g = 0; g < lanes; ++g) {
                int a = s0 + (int)(((int64_t)len * g) / lanes);
                const int b = s0 + (int)(((int64_t)len * (g + 1)) / lanes);
                if (a >= b) continue;
                int p = corr_index(t, a);
                while (a < b) {
                    if (runs.empty() || runs.back() != p) {
                        runs.push_back(a);
                        runs.push_back(p);
                    }
                    int pn;
                    const int e = corr_run_end(t, a, b, p, &pn);
                    if (e <= a || e > b || (e < b && pn <= p)) {
                        fprintf(stderr, "set %ld: the walk does not advance (a=%d e=%d b=%d p=%d pn=%d)\n", sets, a, e, b, p, pn);
                        return 1;
                    }
                    a = e;
                    p = pn;
                }
            }
        }
        const int32_t count = (int32_t)(runs.size() / 2);
        if (text) {
            for (int32_t r = 0; r < count; ++r) printf("%d:%d ", runs[2 * r], runs[2 * r + 1]);
            printf("\n");
        } else {
            fwrite(&count, sizeof(count), 1, stdout);
            fwrite(runs.data(), sizeof(int32_t), runs.size(), stdout);
        }
        ++sets;
    }
    fflush(stdout);
    fprintf(stderr, "ok %ld\n", sets);
    return 0;
}
