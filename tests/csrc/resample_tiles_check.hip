// Host-side proof of the index arithmetic of the rational resampler (sydr_amd/csrc/resample_tiles.h): a stream is cut into
// pushes and every push into tiles the way resample.hip does, over small L, M (1..7 and one pair with gcd > 1), T (1..3L + 2),
// tile sizes, push lengths, ring offsets and capacities.  Checked: the outputs of a push are exactly the m with
// N*L <= m*M < (N + n_in)*L and the tiles cover each of them exactly once; every output gets the statement's (p, q, K_p) --
// u = m*M, q = u div L, p = u mod L, K_p = ceil((T - p) / L) or 0 -- and its taps h[p + k*L] out of the [k][r] table, each
// against input q - k, which the tile fetched from the right place (the push's block inside [0, n_in), or the history inside
// [0, Tp-1)) holding the right absolute sample -- the history being carried from push to push by ddc_tiles.h's ddc_hist_source with Tp in T's place, pushes shorter
// than Tp-1 (and empty ones) included; every output's ring sample lies inside the push's window (ring_offset + i) mod capacity,
// inside the ring, and no two outputs share one.  Then the tile size and LDS span the library chooses for everything
// sdr_ddc_create_rational accepts, and large indices.  Built with `hipcc --cuda-host-only`.
//   usage: resample_tiles_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sydr_amd/csrc/resample_tiles.h"

using namespace sdr;

#define FAIL(...)            \
    do {                     \
        printf(__VA_ARGS__); \
        return false;        \
    } while (0)

// One stream of pushes `lens` through (L, M, T, tile); sample j of the stream has the value j + 1 (0 = before the stream), tap i
// of the prototype the value i + 1 (0 = no such tap).
static bool run_stream(int L, int M, int T, int tile, const std::vector<int64_t>& lens, int64_t capacity, int64_t ring_offset, long& cases) {
    const RsPush shape = rs_push(0, 0, L, M, T);
    const int Tp = shape.Tp, Lp = shape.Lp;
    if (Tp != (T + L - 1) / L || L % Lp || (int64_t)Lp * M % L) FAIL("shape: L=%d M=%d T=%d Tp=%d Lp=%d\n", L, M, T, Tp, Lp);
    std::vector<int> table((size_t)Tp * Lp);
    for (int k = 0; k < Tp; ++k)
        for (int r = 0; r < Lp; ++r) table[(size_t)k * Lp + r] = rs_table_tap(L, M, T, k, r) + 1;
    std::vector<int64_t> hist((size_t)(Tp - 1), 0), next_hist(hist.size());
    int64_t N = 0;
    for (int64_t n_in : lens) {
        std::vector<int64_t> block((size_t)n_in);
        for (int64_t r = 0; r < n_in; ++r) block[(size_t)r] = N + r + 1;
        const RsPush p = rs_push(N, n_in, L, M, T);
        int64_t want_first = 0, want_count = 0;
        for (int64_t m = 0; m * M < (N + n_in) * L; ++m)
            if (m * M >= N * L) {
                if (!want_count) want_first = m;
                ++want_count;
            }
        if (p.n_out != want_count || (want_count && p.m_first != want_first))
            FAIL("outputs: L=%d M=%d N=%lld n_in=%lld first=%lld count=%lld\n", L, M, (long long)N, (long long)n_in, (long long)p.m_first, (long long)p.n_out);
        if (p.n_out <= capacity) {
            std::vector<int> out_seen((size_t)p.n_out, 0), ring_seen((size_t)capacity, 0);
            const int64_t tiles = rs_tiles(p, tile);
            for (int64_t b = 0; b < tiles; ++b) {
                const RsTile t = rs_tile(p, tile, b);
                if (t.count < 1 || t.count > tile || t.i0 + t.count > p.n_out || t.span < Tp || t.span > rs_tile_span_max(L, M, T, tile))
                    FAIL("tile: L=%d M=%d T=%d tile=%d N=%lld n_in=%lld b=%lld count=%d span=%d\n", L, M, T, tile, (long long)N, (long long)n_in, (long long)b, t.count, t.span);
                std::vector<int64_t> z((size_t)t.span);
                for (int i = 0; i < t.span; ++i) {
                    const int64_t j = t.j0 + i, src = rs_source(p, j);
                    int64_t value;
                    if (src >= 0) {
                        if (src >= n_in) FAIL("source past the push: L=%d M=%d T=%d N=%lld n_in=%lld j=%lld\n", L, M, T, (long long)N, (long long)n_in, (long long)j);
                        value = block[(size_t)src];
                    } else {
                        if (~src >= Tp - 1) FAIL("source behind the history: L=%d M=%d T=%d N=%lld j=%lld\n", L, M, T, (long long)N, (long long)j);
                        value = hist[(size_t)~src];
                    }
                    if (value != (j >= 0 ? j + 1 : 0))
                        FAIL("splice: L=%d M=%d T=%d N=%lld n_in=%lld j=%lld holds %lld\n", L, M, T, (long long)N, (long long)n_in, (long long)j, (long long)value);
                    z[(size_t)i] = value;
                }
                for (int o = 0; o < t.count; ++o) {
                    const int64_t m = p.m_first + t.i0 + o;
                    // the statement's own
                    const int64_t u = m * M, q = u / L;
                    const int ph = (int)(u % L), K = ph >= T ? 0 : (T - ph + L - 1) / L;
                    const RsPhase full = rs_phase(p, m);
                    const RsOutput w = rs_output(p, t, o);
                    if (full.q != q || full.p != ph || full.K != K || full.r != (int)(m % Lp) || w.p != ph || w.K != K || w.r != full.r || t.j0 + w.at != q)
                        FAIL("phase: L=%d M=%d T=%d m=%lld p=%d/%d K=%d/%d r=%d at=%d q=%lld\n", L, M, T, (long long)m, w.p, ph, w.K, K, w.r, w.at, (long long)q);
                    if (q < N || q >= N + n_in) FAIL("push rule: L=%d M=%d m=%lld q=%lld N=%lld n_in=%lld\n", L, M, (long long)m, (long long)q, (long long)N, (long long)n_in);
                    for (int k = 0; k < Tp; ++k) {
                        const int tap = table[(size_t)k * Lp + w.r];      // (the kernel's load of tap k; 0: none)
                        if (tap != (k < K ? ph + k * L + 1 : 0)) FAIL("table: L=%d M=%d T=%d m=%lld k=%d holds %d\n", L, M, T, (long long)m, k, tap);
                        if (k >= K) continue;
                        const int at = w.at - k;                           // (the kernel's LDS index of tap k)
                        const int64_t j = q - k;
                        if (at < 0 || at >= t.span || z[(size_t)at] != (j >= 0 ? j + 1 : 0))
                            FAIL("tap: L=%d M=%d T=%d m=%lld k=%d at=%d\n", L, M, T, (long long)m, k, at);
                    }
                    ++out_seen[(size_t)(t.i0 + o)];
                    const int64_t pos = ddc_ring_pos(ring_offset, t.i0 + o, capacity);
                    if (pos < 0 || pos >= capacity || pos != (ring_offset + t.i0 + o) % capacity)
                        FAIL("ring: offset=%lld i=%lld capacity=%lld pos=%lld\n", (long long)ring_offset, (long long)(t.i0 + o), (long long)capacity, (long long)pos);
                    ++ring_seen[(size_t)pos];
                }
                // the tile's last input is its last output's q: nothing is fetched past what some output could need
                if (t.j0 + t.span - 1 != (p.m_first + t.i0 + t.count - 1) * M / L)
                    FAIL("span: L=%d M=%d T=%d tile=%d b=%lld\n", L, M, T, tile, (long long)b);
            }
            for (int64_t i = 0; i < p.n_out; ++i)
                if (out_seen[(size_t)i] != 1) FAIL("cover: L=%d M=%d T=%d tile=%d N=%lld n_in=%lld output %lld seen %d\n", L, M, T, tile, (long long)N, (long long)n_in, (long long)i, out_seen[(size_t)i]);
            for (int64_t s = 0; s < capacity; ++s) {
                const int64_t rel = s >= ring_offset ? s - ring_offset : s + capacity - ring_offset;
                if (ring_seen[(size_t)s] != (rel < p.n_out ? 1 : 0))
                    FAIL("window: offset=%lld n_out=%lld capacity=%lld sample %lld written %d times\n", (long long)ring_offset, (long long)p.n_out, (long long)capacity, (long long)s, ring_seen[(size_t)s]);
            }
        }
        // the history after the push, every element read before any is written (as the kernel's barrier has it)
        for (int i = 0; i < Tp - 1; ++i) {
            const int64_t src = ddc_hist_source(n_in, Tp, i);
            if (src >= 0 ? src >= n_in : ~src >= Tp - 1) FAIL("history source: Tp=%d n_in=%lld i=%d\n", Tp, (long long)n_in, i);
            next_hist[(size_t)i] = src >= 0 ? block[(size_t)src] : hist[(size_t)~src];
        }
        hist.swap(next_hist);
        N += n_in;
        for (int i = 0; i < Tp - 1; ++i) {
            const int64_t j = N - (Tp - 1) + i;
            if (hist[(size_t)i] != (j >= 0 ? j + 1 : 0)) FAIL("history: Tp=%d N=%lld i=%d holds %lld\n", Tp, (long long)N, i, (long long)hist[(size_t)i]);
        }
        ++cases;
    }
    return true;
}

int main() {
    long cases = 0;
    uint64_t state = 20260019;
    auto next = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return state >> 33;
    };
    // L, M in 1..7 and (6, 4) with gcd 2 among them, plus (4, 10) and (12, 8): every T in 1..3L + 2
    std::vector<std::pair<int, int>> ratios;
    for (int L = 1; L <= 7; ++L)
        for (int M = 1; M <= 7; ++M) ratios.push_back({L, M});
    ratios.push_back({4, 10});
    ratios.push_back({12, 8});
    for (const auto& lm : ratios) {
        const int L = lm.first, M = lm.second;
        for (int T = 1; T <= 3 * L + 2; ++T) {
            const int Tp = (T + L - 1) / L;
            for (int tile = 1; tile <= 5; tile += 2)
                for (int64_t capacity = 96; capacity <= 120; capacity += 24)
                    for (int64_t off = 0; off < capacity; off += 59) {
                        // pairs of push lengths 0 .. 3 Tp + 1: every residue of N*L mod M, every history shorter, equal and longer
                        // than the push (tiles of 1 and 3); then a longer random sequence (tiles of 5 too)
                        for (int64_t a = 0; a <= 3 * Tp + 1 && tile < 5; ++a)
                            for (int64_t b = 0; b <= 3 * Tp + 1; b += 1 + a % 3)
                                if (!run_stream(L, M, T, tile, {a, b, 1, (int64_t)Tp - 1, (int64_t)Tp}, capacity, off, cases)) return 1;
                        std::vector<int64_t> lens;
                        for (int k = 0; k < 10; ++k) lens.push_back((int64_t)(next() % (3 * Tp + 3)));
                        if (!run_stream(L, M, T, tile, lens, capacity, off, cases)) return 1;
                    }
        }
    }
    // the library's own tile size: at least one output, the LDS span within the budget, for everything rs_valid accepts (T at
    // both ends of every L's range and in between)
    for (int L = 1; L <= kRsMaxInterpolation; ++L)
        for (int M = 1; M <= kRsMaxDecimation; ++M) {
            const int t_max = L * kRsMaxPhaseTaps < kRsMaxTaps ? L * kRsMaxPhaseTaps : kRsMaxTaps;
            const int Ts[4] = {1, L + 1 < t_max ? L + 1 : t_max, t_max / 2 + 1, t_max};
            for (int T : Ts) {
                const bool want = M <= 64 * L;
                if (rs_valid(L, M, T) != want || rs_valid(L, M, t_max + 1) || rs_valid(L, M, 0)) {
                    printf("valid: L=%d M=%d T=%d\n", L, M, T);
                    return 1;
                }
                if (!want) continue;
                const int tile = rs_tile_outputs(L, M, T);
                if (tile < 1 || tile > kRsMaxTile || rs_tile_span_max(L, M, T, tile) > kRsLdsInputs) {
                    printf("tile size: L=%d M=%d T=%d tile=%d span=%d\n", L, M, T, tile, rs_tile_span_max(L, M, T, tile));
                    return 1;
                }
                ++cases;
            }
        }
    if (rs_valid(0, 1, 1) || rs_valid(1025, 1, 1) || rs_valid(1, 0, 1) || rs_valid(16, 1025, 1) || rs_valid(1, 65, 1) || !rs_valid(1, 64, 512) ||
        rs_valid(1, 64, 513) || !rs_valid(64, 1, 32768) || rs_valid(63, 1, 32768) || rs_valid(1024, 1, 32769)) {
        printf("limits\n");
        return 1;
    }
    // large indices: 64-bit arithmetic, nothing truncates; the range check keeps (N + n_in) * L below 2^62
    for (int k = 0; k < 100000; ++k) {
        const int L = 1 + (int)(next() % 1024);
        int M = 1 + (int)(next() % 1024);
        if (M > 64 * L) M = 64 * L;
        int T = 1 + (int)(next() % 32768);
        if ((T + L - 1) / L > 512) T = 512 * L;
        const int64_t n_in = 1 + (int64_t)(next() % ((uint64_t)1 << 31));
        int64_t N = (int64_t)(((next() << 20) ^ next()) % (uint64_t)(kRsMaxIndex / L));
        if (!rs_in_range(N, n_in, L)) {
            if ((__int128)(N + n_in) * L < (__int128)kRsMaxIndex - L) {
                printf("range: N=%lld n_in=%lld L=%d refused\n", (long long)N, (long long)n_in, L);
                return 1;
            }
            N = 0;
        }
        if ((__int128)(N + n_in) * L >= (__int128)kRsMaxIndex) {
            printf("range: N=%lld n_in=%lld L=%d accepted\n", (long long)N, (long long)n_in, L);
            return 1;
        }
        const RsPush p = rs_push(N, n_in, L, M, T);
        if (p.m_first * M < N * L || (p.m_first - 1) * M >= N * L || (p.n_out && (p.m_first + p.n_out - 1) * M >= (N + n_in) * L) ||
            (p.m_first + p.n_out) * M < (N + n_in) * L) {
            printf("large: N=%lld n_in=%lld L=%d M=%d\n", (long long)N, (long long)n_in, L, M);
            return 1;
        }
        if (p.n_out) {
            const int tile = rs_tile_outputs(L, M, T);
            const int64_t b = rs_tiles(p, tile) - 1;
            const RsTile t = rs_tile(p, tile, b);
            const RsOutput w = rs_output(p, t, t.count - 1);
            const RsPhase full = rs_phase(p, p.m_first + p.n_out - 1);
            if (t.j0 + t.span - 1 >= N + n_in || t.j0 < N - (p.Tp - 1) || rs_source(p, t.j0 + t.span - 1) >= n_in || t.span > rs_tile_span_max(L, M, T, tile) ||
                w.p != full.p || w.K != full.K || w.r != full.r || t.j0 + w.at != full.q || w.at != t.span - 1) {
                printf("large tile: N=%lld n_in=%lld L=%d M=%d T=%d\n", (long long)N, (long long)n_in, L, M, T);
                return 1;
            }
        }
        ++cases;
    }
    printf("ok %ld\n", cases);
    return 0;
}
