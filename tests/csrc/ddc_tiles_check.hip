// Host-side proof of the index arithmetic of the down-converter (sydr_amd/csrc/ddc_tiles.h): a stream is cut into pushes and
// every push into tiles the way ddc.hip does, over small T, D, tile sizes, push lengths, ring offsets and capacities.  Checked:
// the outputs of a push are exactly the m with N <= m*D < N + n_in and the tiles cover each of them exactly once; the inputs a
// tile fetches are exactly m*D - (T-1) .. m*D of its outputs, each fetched once per tile, each from the right place (the
// push's block inside [0, n_in), or the history inside [0, T-1)) and holding the right absolute sample -- the history being
// carried from push to push by ddc_hist_source, pushes shorter than T-1 (and empty ones) included; every output's ring sample
// lies inside the push's window (ring_offset + i) mod capacity, inside the ring, and no two outputs share one.  Then the tile
// size the library chooses for every (T, D) it accepts.  Built with `hipcc --cuda-host-only`.
//   usage: ddc_tiles_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sydr_amd/csrc/ddc_tiles.h"

using namespace sdr;

#define FAIL(...)            \
    do {                     \
        printf(__VA_ARGS__); \
        return false;        \
    } while (0)

// One stream of pushes `lens` through (T, D, tile); sample j of the stream has the value j + 1 (0 = before the stream).
static bool run_stream(int T, int D, int tile, const std::vector<int64_t>& lens, int64_t capacity, int64_t ring_offset, long& cases) {
    std::vector<int64_t> hist((size_t)(T > 1 ? T - 1 : 0), 0), next_hist(hist.size());
    int64_t N = 0;
    for (int64_t n_in : lens) {
        std::vector<int64_t> block((size_t)n_in);
        for (int64_t r = 0; r < n_in; ++r) block[(size_t)r] = N + r + 1;
        const DdcPush p = ddc_push(N, n_in, D, T);
        int64_t want_first = 0, want_count = 0;
        for (int64_t m = 0; m * D < N + n_in; ++m)
            if (m * D >= N) {
                if (!want_count) want_first = m;
                ++want_count;
            }
        if (p.n_out != want_count || (want_count && p.m_first != want_first))
            FAIL("outputs: T=%d D=%d N=%lld n_in=%lld first=%lld count=%lld\n", T, D, (long long)N, (long long)n_in, (long long)p.m_first, (long long)p.n_out);
        if (p.n_out <= capacity) {
            std::vector<int> out_seen((size_t)p.n_out, 0), ring_seen((size_t)capacity, 0);
            const int64_t tiles = ddc_tiles(p, tile);
            for (int64_t b = 0; b < tiles; ++b) {
                const DdcTile t = ddc_tile(p, tile, b);
                if (t.count < 1 || t.count > tile || t.span != (t.count - 1) * D + T || t.i0 + t.count > p.n_out)
                    FAIL("tile: T=%d D=%d tile=%d N=%lld n_in=%lld b=%lld count=%d span=%d\n", T, D, tile, (long long)N, (long long)n_in, (long long)b, t.count, t.span);
                std::vector<int64_t> z((size_t)t.span);
                for (int i = 0; i < t.span; ++i) {
                    const int64_t j = t.j0 + i, src = ddc_source(p, j);
                    int64_t value;
                    if (src >= 0) {
                        if (src >= n_in) FAIL("source past the push: T=%d D=%d N=%lld n_in=%lld j=%lld\n", T, D, (long long)N, (long long)n_in, (long long)j);
                        value = block[(size_t)src];
                    } else {
                        if (~src >= T - 1) FAIL("source behind the history: T=%d D=%d N=%lld j=%lld\n", T, D, (long long)N, (long long)j);
                        value = hist[(size_t)~src];
                    }
                    if (value != (j >= 0 ? j + 1 : 0))
                        FAIL("splice: T=%d D=%d N=%lld n_in=%lld j=%lld holds %lld\n", T, D, (long long)N, (long long)n_in, (long long)j, (long long)value);
                    z[(size_t)i] = value;
                }
                for (int o = 0; o < t.count; ++o) {
                    const int64_t m = p.m_first + t.i0 + o;
                    for (int k = 0; k < T; ++k) {
                        const int at = o * D + (T - 1) - k;            // (the kernel's LDS index of tap k)
                        const int64_t j = m * D - k;
                        if (at < 0 || at >= t.span || z[(size_t)at] != (j >= 0 ? j + 1 : 0))
                            FAIL("tap: T=%d D=%d m=%lld k=%d at=%d\n", T, D, (long long)m, k, at);
                    }
                    ++out_seen[(size_t)(t.i0 + o)];
                    const int64_t pos = ddc_ring_pos(ring_offset, t.i0 + o, capacity);
                    if (pos < 0 || pos >= capacity || pos != (ring_offset + t.i0 + o) % capacity)
                        FAIL("ring: offset=%lld i=%lld capacity=%lld pos=%lld\n", (long long)ring_offset, (long long)(t.i0 + o), (long long)capacity, (long long)pos);
                    ++ring_seen[(size_t)pos];
                }
            }
            for (int64_t i = 0; i < p.n_out; ++i)
                if (out_seen[(size_t)i] != 1) FAIL("cover: T=%d D=%d tile=%d N=%lld n_in=%lld output %lld seen %d\n", T, D, tile, (long long)N, (long long)n_in, (long long)i, out_seen[(size_t)i]);
            for (int64_t s = 0; s < capacity; ++s) {
                const int64_t rel = s >= ring_offset ? s - ring_offset : s + capacity - ring_offset;
                if (ring_seen[(size_t)s] != (rel < p.n_out ? 1 : 0))
                    FAIL("window: offset=%lld n_out=%lld capacity=%lld sample %lld written %d times\n", (long long)ring_offset, (long long)p.n_out, (long long)capacity, (long long)s, ring_seen[(size_t)s]);
            }
        }
        // the history after the push, every element read before any is written (as the kernel's barrier has it)
        for (int i = 0; i < T - 1; ++i) {
            const int64_t src = ddc_hist_source(n_in, T, i);
            if (src >= 0 ? src >= n_in : ~src >= T - 1) FAIL("history source: T=%d n_in=%lld i=%d\n", T, (long long)n_in, i);
            next_hist[(size_t)i] = src >= 0 ? block[(size_t)src] : hist[(size_t)~src];
        }
        hist.swap(next_hist);
        N += n_in;
        for (int i = 0; i < T - 1; ++i) {
            const int64_t j = N - (T - 1) + i;
            if (hist[(size_t)i] != (j >= 0 ? j + 1 : 0)) FAIL("history: T=%d N=%lld i=%d holds %lld\n", T, (long long)N, i, (long long)hist[(size_t)i]);
        }
        ++cases;
    }
    return true;
}

int main() {
    long cases = 0;
    uint64_t state = 20260018;
    auto next = [&]() {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return state >> 33;
    };
    for (int T = 1; T <= 7; ++T)
        for (int D = 1; D <= 5; ++D)
            for (int tile = 1; tile <= 4; ++tile)
                for (int64_t capacity = 8; capacity <= 16; capacity += 8)
                    for (int64_t off = 0; off < capacity; off += 3) {
                        // every pair of push lengths 0..9, the second one exercising every residue of N mod D and every
                        // history shorter, equal and longer than the push; then a longer random sequence
                        for (int64_t a = 0; a <= 9; ++a)
                            for (int64_t b = 0; b <= 9; ++b)
                                if (!run_stream(T, D, tile, {a, b, 1, (int64_t)T - 1, (int64_t)T}, capacity, off, cases)) return 1;
                        std::vector<int64_t> lens;
                        for (int k = 0; k < 12; ++k) lens.push_back((int64_t)(next() % 14));
                        if (!run_stream(T, D, tile, lens, capacity, off, cases)) return 1;
                    }
    // the library's own tile size: fits the LDS budget, at least one output, for everything sdr_ddc_create accepts
    for (int T = 1; T <= kDdcMaxTaps; ++T)
        for (int D = 1; D <= kDdcMaxDecimation; ++D) {
            const int tile = ddc_tile_outputs(D, T);
            if (tile < 1 || tile > kDdcMaxTile || (tile - 1) * D + T > kDdcLdsInputs) {
                printf("tile size: T=%d D=%d tile=%d\n", T, D, tile);
                return 1;
            }
            ++cases;
        }
    // large indices: 64-bit arithmetic, nothing truncates
    for (int k = 0; k < 100000; ++k) {
        const int D = 1 + (int)(next() % 64), T = 1 + (int)(next() % 512);
        const int64_t N = (int64_t)((next() << 9) ^ next()), n_in = 1 + (int64_t)(next() % ((uint64_t)1 << 31));
        const DdcPush p = ddc_push(N, n_in, D, T);
        if (p.m_first * D < N || (p.m_first - 1) * D >= N || (p.n_out && (p.m_first + p.n_out - 1) * D >= N + n_in) || (p.m_first + p.n_out) * D < N + n_in) {
            printf("large: N=%lld n_in=%lld D=%d\n", (long long)N, (long long)n_in, D);
            return 1;
        }
        if (p.n_out) {
            const int tile = ddc_tile_outputs(D, T);
            const DdcTile t = ddc_tile(p, tile, ddc_tiles(p, tile) - 1);
            if (t.j0 + t.span - 1 >= N + n_in || t.j0 < N - (T - 1) || ddc_source(p, t.j0 + t.span - 1) >= n_in) {
                printf("large tile: N=%lld n_in=%lld D=%d T=%d\n", (long long)N, (long long)n_in, D, T);
                return 1;
            }
        }
        ++cases;
    }
    printf("ok %ld\n", cases);
    return 0;
}
