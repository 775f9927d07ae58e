// Index arithmetic of the rational resampler (resample.hip), shared by the host that sizes the launches and builds the tap
// table, the kernels and the host check tests/csrc/resample_tiles_check.hip.  A sibling of ddc_tiles.h; every index that can
// grow with the stream is 64-bit.
//
// Interpolation by L, decimation by M, a prototype filter h[0..T-1] at the up-sampled rate.  Input samples are counted
// j = 0, 1, ... from creation or reset, across pushes; output m has
//   u = m*M    q = u div L    p = u mod L    K_p = ceil((T - p) / L)  (0 when p >= T)
// and is made of the products h[p + k*L] * z_{q-k}, k = 0 .. K_p - 1 (x_j = 0 for j < 0).  With g = gcd(L, M), L' = L/g and
// M' = M/g, outputs L' apart share p and lie M' inputs apart: the PERIOD.  Tp = ceil(T / L) is the longest phase.
// A PUSH of n_in inputs whose first has index N writes the outputs m with N*L <= m*M < (N + n_in)*L (that is N <= q_m < N + n_in):
// m_first = ceil(N*L / M), n_out = ceil((N + n_in)*L / M) - m_first, output m_first + i at ring sample (ring_offset + i) mod capacity.
// A TILE is `tile` consecutive outputs of a push (the last one fewer): one workgroup, which needs the `span` inputs
// j0 .. j0 + span - 1, j0 = q_first - (Tp-1), span = q_last - q_first + Tp.  Input j of a push lies in the push's block at j - N when
// that is >= 0 and in the HISTORY (the last Tp-1 raw inputs before the push, oldest first) at (Tp-1) + (j - N) otherwise; a tile
// never reaches behind the history nor past the push.  After the push the history is the last Tp-1 inputs again: ddc_tiles.h's
// splice with Tp in T's place (ddc_hist_source), as the ring position is ddc_tiles.h's own (ddc_ring_pos).
// The TAP TABLE is laid out [k][r], r = m mod L' the output's index within the period: table[k*L' + r] = h[p_r + k*L] where that
// exists and 0 behind it, p_r = (r*M) mod L -- for a fixed k the loads of consecutive outputs are one contiguous run (a wrap at
// L' aside).
#pragma once

#include <cstdint>

#include "ddc_tiles.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDR_RS_HD __host__ __device__
#else
#define SDR_RS_HD
#endif

namespace sdr {

constexpr int kRsMaxInterpolation = 1024;
constexpr int kRsMaxDecimation = 1024;
constexpr int kRsMaxRatio = 64;            // M <= 64 L
constexpr int kRsMaxTaps = 32768;          // of the prototype
constexpr int kRsMaxPhaseTaps = kDdcMaxTaps; // Tp = ceil(T / L) at most: the history is the integer converter's, saved by its kernel
constexpr int kRsThreads = 256;
// Mixed inputs (16 bytes each) a workgroup keeps in LDS: 63 KiB, two workgroups per CU of 160 KiB with room to spare.
constexpr int kRsLdsInputs = 4032;
constexpr int kRsMaxTile = 1024;           // outputs per workgroup at most (four per lane)
constexpr int64_t kRsMaxIndex = (int64_t)1 << 62;   // (N + n_in) * L stays below

SDR_RS_HD inline int rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b, b = t;
    }
    return a;
}

SDR_RS_HD inline int rs_phase_taps(int L, int T) { return (T + L - 1) / L; }

// What sdr_ddc_create_rational accepts.
SDR_RS_HD inline bool rs_valid(int L, int M, int T) {
    return L >= 1 && L <= kRsMaxInterpolation && M >= 1 && M <= kRsMaxDecimation && M <= kRsMaxRatio * L && T >= 1 && T <= kRsMaxTaps &&
           rs_phase_taps(L, T) <= kRsMaxPhaseTaps;
}

// Whether n_in more inputs keep (N + n_in) * L below 2^62 (N, n_in >= 0).
SDR_RS_HD inline bool rs_in_range(int64_t n_seen, int64_t n_in, int L) { return n_in <= kRsMaxIndex / L - 1 - n_seen; }

struct RsPush {
    int64_t n_seen;    // N: inputs before this push
    int64_t n_in;
    int64_t m_first;   // first output of the push
    int64_t n_out;
    int L, M, T;
    int Tp;            // ceil(T / L)
    int Lp;            // L' = L / gcd(L, M): the period in outputs
};

SDR_RS_HD inline RsPush rs_push(int64_t n_seen, int64_t n_in, int L, int M, int T) {
    RsPush p;
    p.n_seen = n_seen, p.n_in = n_in, p.L = L, p.M = M, p.T = T;
    p.Tp = rs_phase_taps(L, T);
    p.Lp = L / rs_gcd(L, M);
    p.m_first = ddc_ceil_div(n_seen * L, M);
    p.n_out = ddc_ceil_div((n_seen + n_in) * L, M) - p.m_first;
    return p;
}

// The phase of output m: u = m*M, q = u div L, p = u mod L, K_p, and r = m mod L' (the statement's own, 64-bit).
struct RsPhase {
    int64_t q;
    int p, K, r;
};

SDR_RS_HD inline int rs_taps_of_phase(int p, int L, int T) { return p >= T ? 0 : (T - p + L - 1) / L; }

SDR_RS_HD inline RsPhase rs_phase(const RsPush& push, int64_t m) {
    RsPhase w;
    const int64_t u = m * push.M;
    w.q = u / push.L;
    w.p = (int)(u % push.L);
    w.K = rs_taps_of_phase(w.p, push.L, push.T);
    w.r = (int)(m % push.Lp);
    return w;
}

// Outputs per workgroup: as many as kRsLdsInputs mixed inputs make -- n outputs span at most ceil((n-1) M / L) + Tp inputs --,
// kRsMaxTile at most (>= 56 for everything rs_valid accepts).
SDR_RS_HD inline int rs_tile_outputs(int L, int M, int T) {
    const int t = (kRsLdsInputs - rs_phase_taps(L, T)) * L / M + 1;
    return t < kRsMaxTile ? t : kRsMaxTile;
}

// Inputs a tile of `tile` outputs spans at most, whatever its first phase: what the launch sizes the LDS by.
SDR_RS_HD inline int rs_tile_span_max(int L, int M, int T, int tile) { return ((tile - 1) * M + L - 1) / L + rs_phase_taps(L, T); }

struct RsTile {
    int64_t i0;     // first output of the tile, counted from the push's first
    int64_t j0;     // first input it needs (absolute; may be negative: before the stream began)
    int count;      // outputs
    int span;       // inputs
    int p0;         // phase of the first output
    int r0;         // its index within the period
};

SDR_RS_HD inline int64_t rs_tiles(const RsPush& p, int tile) { return ddc_ceil_div(p.n_out, tile); }

SDR_RS_HD inline RsTile rs_tile(const RsPush& p, int tile, int64_t b) {
    RsTile t;
    t.i0 = b * tile;
    const int64_t left = p.n_out - t.i0;
    t.count = (int)(left < tile ? left : tile);
    const RsPhase first = rs_phase(p, p.m_first + t.i0);
    t.p0 = first.p, t.r0 = first.r;
    t.j0 = first.q - (p.Tp - 1);
    t.span = (t.p0 + (t.count - 1) * p.M) / p.L + p.Tp;       // (below 2^21: 32-bit)
    return t;
}

// Output o of a tile: its phase, its taps, its column of the tap table, and `at`, the tile's index of input q -- tap k meets the
// tile's input at - k, k < K <= Tp.  (p0 + o*M < 2^21: 32-bit arithmetic, from the tile's first output.)
struct RsOutput {
    int p, K, r, at;
};

SDR_RS_HD inline RsOutput rs_output(const RsPush& push, const RsTile& t, int o) {
    RsOutput w;
    const int u = t.p0 + o * push.M;
    w.p = u % push.L;
    w.K = rs_taps_of_phase(w.p, push.L, push.T);
    w.r = (t.r0 + o) % push.Lp;
    w.at = u / push.L + (push.Tp - 1);
    return w;
}

// Where input j (absolute) of a tile lies: >= 0 -- sample of the push's block; < 0 -- ~value is the history element.
SDR_RS_HD inline int64_t rs_source(const RsPush& p, int64_t j) {
    const int64_t rel = j - p.n_seen;
    return rel >= 0 ? rel : ~((int64_t)(p.Tp - 1) + rel);
}

// Entry [k][r] of the tap table: the prototype's index, or -1 where phase p_r has no tap k (the table holds 0 there).
SDR_RS_HD inline int rs_table_tap(int L, int M, int T, int k, int r) {
    const int p = (int)(((int64_t)r * M) % L);
    const int at = p + k * L;
    return at < T ? at : -1;
}

}  // namespace sdr
