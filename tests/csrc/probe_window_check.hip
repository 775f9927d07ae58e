// Host-side proof of the window arithmetic of sdr_iq_probe (sydr_amd/csrc/probe_window.h): for rings of a few granules and
// every (base, n, samples per granule), walking granules 0 .. total - 1 the way the moments kernel does visits every sample of
// the window exactly once and no other, every granule lies inside the ring, every granule holds at least one sample of the
// window; and the Welch segments' samples are the window's, in order, for every nfft that fits.  Then the same properties
// for random windows of a ring of 2^33 samples (64-bit arithmetic: nothing truncates).  Built with `hipcc --cuda-host-only`.
//   usage: probe_window_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sydr_amd/csrc/probe_window.h"

using namespace sdr;

static bool small_ring(int64_t capacity, int spg, long& cases) {
    std::vector<int> seen((size_t)capacity);
    for (int64_t base = 0; base < capacity; ++base)
        for (int64_t n = 1; n <= capacity; ++n) {
            const ProbeWindow w = probe_window(base, n, capacity, spg);
            for (auto& v : seen) v = 0;
            for (int64_t i = 0; i < w.total; ++i) {
                int64_t lo, hi;
                const int64_t g = probe_granule(w, i, spg, &lo, &hi);
                if (g < 0 || (g + 1) * spg > capacity || lo >= hi || lo < g * spg || hi > (g + 1) * spg) {
                    printf("granule: capacity=%lld spg=%d base=%lld n=%lld i=%lld g=%lld lo=%lld hi=%lld\n", (long long)capacity, spg,
                           (long long)base, (long long)n, (long long)i, (long long)g, (long long)lo, (long long)hi);
                    return false;
                }
                for (int64_t s = lo; s < hi; ++s) ++seen[(size_t)s];
            }
            for (int64_t s = 0; s < capacity; ++s) {
                const int64_t rel = s >= base ? s - base : s + capacity - base;
                if (seen[(size_t)s] != (rel < n ? 1 : 0)) {
                    printf("cover: capacity=%lld spg=%d base=%lld n=%lld sample=%lld seen=%d\n", (long long)capacity, spg, (long long)base,
                           (long long)n, (long long)s, seen[(size_t)s]);
                    return false;
                }
            }
            for (int nfft = 4; nfft <= 16; nfft *= 2) {   // (the arithmetic does not care that the call wants 64 or more)
                const int64_t S = probe_segments(n, nfft);
                if ((n < nfft) != (S == 0) || (S > 0 && ((S - 1) * (nfft / 2) + nfft > n || S * (nfft / 2) + nfft <= n))) {
                    printf("segments: n=%lld nfft=%d S=%lld\n", (long long)n, nfft, (long long)S);
                    return false;
                }
                for (int64_t s = 0; s < S; ++s)
                    for (int j = 0; j < nfft; ++j)
                        if (probe_segment_sample(base, capacity, s, nfft, j) != (base + s * (nfft / 2) + j) % capacity) {
                            printf("segment sample: capacity=%lld base=%lld s=%lld nfft=%d j=%d\n", (long long)capacity, (long long)base,
                                   (long long)s, nfft, j);
                            return false;
                        }
            }
            ++cases;
        }
    return true;
}

int main() {
    long cases = 0;
    for (int spg = 1; spg <= 8; spg *= 2)
        for (int granules = 1; granules <= 5; ++granules)
            if (!small_ring((int64_t)granules * spg, spg, cases)) return 1;
    uint64_t state = 20260017;
    auto next = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return state >> 11;
    };
    const int64_t capacity = (int64_t)1 << 33;
    for (int k = 0; k < 200000; ++k) {
        const int spg = 1 << (next() % 4);
        const int64_t base = (int64_t)(next() % (uint64_t)capacity);
        const int64_t n = 1 + (int64_t)(next() % ((uint64_t)1 << 31));
        const ProbeWindow w = probe_window(base, n, capacity, spg);
        int64_t samples = 0;
        const int64_t picks[4] = {0, w.piece[0].count - 1, w.piece[0].count, w.total - 1};
        for (int64_t i : picks) {
            if (i < 0 || i >= w.total) continue;
            int64_t lo, hi;
            const int64_t g = probe_granule(w, i, spg, &lo, &hi);
            if (g < 0 || (g + 1) * spg > capacity || lo >= hi || lo < g * spg || hi > (g + 1) * spg) {
                printf("large: base=%lld n=%lld spg=%d i=%lld\n", (long long)base, (long long)n, spg, (long long)i);
                return 1;
            }
        }
        for (int p = 0; p < 2; ++p) samples += w.piece[p].hi - w.piece[p].lo;
        if (samples != n || w.total < (n + spg - 1) / spg || w.total > n / spg + 4) {
            printf("large: base=%lld n=%lld spg=%d samples=%lld total=%lld\n", (long long)base, (long long)n, spg, (long long)samples,
                   (long long)w.total);
            return 1;
        }
        ++cases;
    }
    printf("ok %ld\n", cases);
    return 0;
}
