// Host-side proof of the index arithmetic of the mitigator (sydr_amd/csrc/mit_plan.h) against a brute-force restatement:
// a stream is cut into pushes the way ddc.hip and mitigate.hip do, over small N (8, 16 and none), blank_lead, blank_hold, push
// lengths, ring offsets and capacities.  Sample m of v has the value m + 1 (0 = before the stream); the work buffer W, the
// blanker's U and the segments are built by the header's arithmetic alone and every value an output is made of is traced
// back by definition.  Checked, push by push:
//   W = [state, push] holds v_{n-K} .. v_{n+k-1}; the state handed over is W[k .. k + K); K is tight (some push reads W[0]);
//   every u in U has its whole blanker reach inside W, and U[x] stands for u_{j_lo + x};
//   every computed segment lies inside U and begins at u_{s H};
//   output i is y_{n+i-L}: its two terms are sample m - (q-1)H of segment q - 1 and sample m - qH of segment q, both
//   computed in this push (or, without the excisor, U holds u_m), and nothing is read for m < 0;
//   every u index >= 0 is counted by exactly one push, and after n outputs exactly those below n - L are; every segment
//   s >= -1 is counted as finished by exactly one push, exactly when s H + N <= n - L, and mit_segments_finished(n) agrees;
//   the ring samples written are the push's window (ring_offset + i) mod capacity, each once.
// Built with `hipcc --cuda-host-only`.
//   usage: mit_plan_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "../../sydr_amd/csrc/ddc_tiles.h"
#include "../../sydr_amd/csrc/mit_plan.h"

using namespace sdr;

#define FAIL(...)            \
    do {                     \
        printf(__VA_ARGS__); \
        return false;        \
    } while (0)

static int64_t value_of(int64_t m) { return m >= 0 ? m + 1 : 0; }

static bool run_stream(int N, int lead, int hold, const std::vector<int64_t>& lens, int64_t capacity, int64_t ring_offset, bool* read_w0, long& cases) {
    const int H = N / 2;
    const int64_t L = (N ? N : 0) + lead, K = mit_state_length(N, lead, hold);
    if (mit_delay(N, lead) != L) FAIL("delay: N=%d lead=%d\n", N, lead);
    std::vector<int64_t> state((size_t)K, 0);
    std::map<int64_t, int> u_counted, seg_counted;
    int64_t n = 0;
    for (int64_t k : lens) {
        const MitPlan p = mit_plan(n, k, N, lead, hold);
        if (p.K != K || p.L != L) FAIL("plan: K / L\n");
        std::vector<int64_t> W(state);
        for (int64_t r = 0; r < k; ++r) W.push_back(value_of(n + r));
        for (int64_t x = 0; x < K + k; ++x)
            if (W[(size_t)x] != value_of(n - K + x)) FAIL("W: N=%d lead=%d hold=%d n=%lld k=%lld x=%lld\n", N, lead, hold, (long long)n, (long long)k, (long long)x);
        if (k > 0) {
            // U: u_{j_lo + x} reads W[x .. x + hold + lead], its own v at W[x + hold]
            if (p.n_u < k || p.n_u + hold + lead != K + k) FAIL("U length: n=%lld k=%lld n_u=%lld\n", (long long)n, (long long)k, (long long)p.n_u);
            std::vector<int64_t> U((size_t)p.n_u);
            for (int64_t x = 0; x < p.n_u; ++x) {
                const int64_t j = p.j_lo + x;
                if (W[(size_t)(x + hold)] != value_of(j)) FAIL("U: u_%lld is not W[%lld]\n", (long long)j, (long long)(x + hold));
                if (value_of(j - hold) != W[(size_t)x] || value_of(j + lead) != W[(size_t)(x + hold + lead)]) FAIL("U reach: j=%lld\n", (long long)j);
                U[(size_t)x] = value_of(j);
            }
            std::vector<int64_t> B((size_t)(p.n_seg * N));     // B[sl][r] = the u index segment s_lo + sl, sample r, is made at
            for (int64_t sl = 0; sl < p.n_seg; ++sl) {
                const int64_t at = mit_segment_u(p, sl), s = p.s_lo + sl;
                if (at < 0 || at + N > p.n_u) FAIL("segment outside U: N=%d lead=%d hold=%d n=%lld k=%lld s=%lld at=%lld n_u=%lld\n", N, lead, hold, (long long)n, (long long)k, (long long)s, (long long)at, (long long)p.n_u);
                if (at == 0) *read_w0 = true;   // (u_{j_lo} reaches back to W[0])
                for (int r = 0; r < N; ++r) {
                    if (U[(size_t)(at + r)] != value_of(s * H + r)) FAIL("segment input: s=%lld r=%d\n", (long long)s, r);
                    B[(size_t)(sl * N + r)] = s * H + r;
                }
                const bool fin = s >= p.fin_lo && s < p.fin_hi;
                const bool want = s >= -1 && n - L < s * H + N && s * H + N <= n + k - L;
                if (fin != want) FAIL("finish: N=%d lead=%d n=%lld k=%lld s=%lld fin=%d\n", N, lead, (long long)n, (long long)k, (long long)s, (int)fin);
                if (fin) ++seg_counted[s];
            }
            if (N) {   // a segment that finishes in this push is among those it computes
                for (int64_t s = p.fin_lo; s < p.fin_hi; ++s)
                    if (s < p.s_lo || s >= p.s_lo + p.n_seg) FAIL("finishing segment %lld not computed: n=%lld k=%lld\n", (long long)s, (long long)n, (long long)k);
            } else if (p.n_seg || p.fin_hi != p.fin_lo) FAIL("segments without an excisor\n");
            if (!N) *read_w0 = true;   // (output 0 is U[0], which reaches back to W[0])
            std::vector<int> ring_seen((size_t)capacity, 0);
            for (int64_t i = 0; i < k && k <= capacity; ++i) {
                const int64_t m = mit_output_m(p, i);
                if (m != n + i - L) FAIL("output m\n");
                if (m >= 0) {
                    if (N) {
                        int64_t a, b;
                        mit_output_terms(p, m, &a, &b);
                        const int64_t q = mit_floor_div(m, H);
                        if (q * H > m || (q + 1) * H <= m) FAIL("floor: m=%lld\n", (long long)m);
                        if (a < 0 || b < 0 || a >= p.n_seg * N || b >= p.n_seg * N) FAIL("terms outside B: n=%lld k=%lld m=%lld a=%lld b=%lld\n", (long long)n, (long long)k, (long long)m, (long long)a, (long long)b);
                        if (B[(size_t)a] != m || B[(size_t)b] != m || a / N != q - 1 - p.s_lo || b / N != q - p.s_lo || a % N != m - (q - 1) * H || b % N != m - q * H)
                            FAIL("terms: n=%lld k=%lld m=%lld\n", (long long)n, (long long)k, (long long)m);
                    } else {
                        const int64_t x = mit_output_u(p, m);
                        if (x < 0 || x >= p.n_u || U[(size_t)x] != value_of(m)) FAIL("output u: m=%lld x=%lld\n", (long long)m, (long long)x);
                    }
                }
                const int64_t pos = ddc_ring_pos(ring_offset, i, capacity);
                if (pos < 0 || pos >= capacity || pos != (ring_offset + i) % capacity) FAIL("ring: i=%lld pos=%lld\n", (long long)i, (long long)pos);
                ++ring_seen[(size_t)pos];
            }
            if (k <= capacity)
                for (int64_t s = 0; s < capacity; ++s) {
                    const int64_t rel = s >= ring_offset ? s - ring_offset : s + capacity - ring_offset;
                    if (ring_seen[(size_t)s] != (rel < k ? 1 : 0)) FAIL("window: sample %lld written %d times\n", (long long)s, ring_seen[(size_t)s]);
                }
            for (int64_t j = p.cnt_lo; j < p.cnt_hi; ++j) {
                if (j < p.j_lo || j >= p.j_lo + p.n_u) FAIL("counted u %lld outside U\n", (long long)j);
                ++u_counted[j];
            }
        } else if (p.n_seg || p.fin_hi != p.fin_lo || p.cnt_hi != p.cnt_lo) FAIL("an empty push computes or counts\n");
        // the hand-over
        for (int64_t x = 0; x < K; ++x) state[(size_t)x] = W[(size_t)(k + x)];
        n += k;
        for (int64_t x = 0; x < K; ++x)
            if (state[(size_t)x] != value_of(n - K + x)) FAIL("state: n=%lld x=%lld\n", (long long)n, (long long)x);
        // the counters are functions of n alone
        int64_t want_u = n - L > 0 ? n - L : 0, want_seg = 0;
        for (int64_t s = -1; N && s * H + N <= n - L; ++s) ++want_seg;
        if ((int64_t)u_counted.size() != want_u) FAIL("counted u: n=%lld have %lld want %lld\n", (long long)n, (long long)u_counted.size(), (long long)want_u);
        for (const auto& kv : u_counted)
            if (kv.second != 1 || kv.first < 0 || kv.first >= n - L) FAIL("u %lld counted %d times\n", (long long)kv.first, kv.second);
        if ((int64_t)seg_counted.size() != want_seg || mit_segments_finished(n, N, lead) != want_seg)
            FAIL("finished segments: N=%d lead=%d n=%lld have %lld formula %lld want %lld\n", N, lead, (long long)n, (long long)seg_counted.size(), (long long)mit_segments_finished(n, N, lead), (long long)want_seg);
        for (const auto& kv : seg_counted)
            if (kv.second != 1 || kv.first < -1 || kv.first * H + N > n - L) FAIL("segment %lld counted %d times\n", (long long)kv.first, kv.second);
        ++cases;
    }
    return true;
}

int main() {
    long cases = 0;
    uint64_t rng = 20260019;
    auto next = [&]() {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        return rng >> 33;
    };
    for (int q = -40; q <= 40; ++q)
        for (int d = 1; d <= 9; ++d) {
            const int64_t f = mit_floor_div(q, d);
            if (f * d > q || (f + 1) * d <= q) {
                printf("floor_div %d / %d\n", q, d);
                return 1;
            }
        }
    const int sizes[] = {0, 8, 16};
    for (int N : sizes)
        for (int lead = 0; lead <= 3; ++lead)
            for (int hold = 0; hold <= 3; ++hold) {
                bool read_w0 = mit_state_length(N, lead, hold) == 0;
                for (int64_t capacity = 48; capacity <= 56; capacity += 8)
                    for (int64_t off = 0; off < capacity; off += 7) {
                        // every pair of push lengths 0 .. N + 3 in front of a tail that passes every residue of n mod H
                        for (int64_t a = 0; a <= N + 3; ++a)
                            for (int64_t b = 0; b <= N + 3; ++b)
                                if (!run_stream(N, lead, hold, {a, b, 1, 0, (int64_t)(N / 2), (int64_t)N + 1, 2, (int64_t)(2 * N + 5)}, capacity, off, &read_w0, cases)) return 1;
                        std::vector<int64_t> lens;
                        for (int k = 0; k < 16; ++k) lens.push_back((int64_t)(next() % (uint64_t)(2 * N + 6)));
                        if (!run_stream(N, lead, hold, lens, capacity, off, &read_w0, cases)) return 1;
                    }
                if (!read_w0) {
                    printf("the state is longer than any push needs: N=%d lead=%d hold=%d\n", N, lead, hold);
                    return 1;
                }
            }
    // large indices: 64-bit arithmetic, nothing truncates
    for (int t = 0; t < 100000; ++t) {
        const int N = 64 << (int)(next() % 7), lead = (int)(next() % 1025), hold = (int)(next() % 1025);
        const int64_t n = (int64_t)((next() << 8) ^ next()), k = 1 + (int64_t)(next() % ((uint64_t)1 << 31));
        const MitPlan p = mit_plan(n, k, N, lead, hold);
        const int64_t last = mit_segment_u(p, p.n_seg - 1);
        int64_t a, b;
        mit_output_terms(p, mit_output_m(p, k - 1) >= 0 ? mit_output_m(p, k - 1) : 0, &a, &b);
        if (mit_segment_u(p, 0) < 0 || last + N > p.n_u || (mit_output_m(p, k - 1) >= 0 && (a < 0 || b >= p.n_seg * N))) {
            printf("large: N=%d lead=%d hold=%d n=%lld k=%lld\n", N, lead, hold, (long long)n, (long long)k);
            return 1;
        }
        ++cases;
    }
    printf("ok %ld\n", cases);
    return 0;
}
