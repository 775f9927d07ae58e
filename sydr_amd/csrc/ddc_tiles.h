// Index arithmetic of the down-converter (ddc.hip), shared by the host that sizes the launches, the kernels and the host
// check tests/csrc/ddc_tiles_check.hip.
//
// Input samples are counted j = 0, 1, ... from creation or reset, across pushes; output m is made of inputs m*D - (T-1) .. m*D
// (x_j = 0 for j < 0).  A PUSH of n_in inputs whose first has index N writes the outputs m with N <= m*D < N + n_in:
// m_first = ceil(N / D), n_out = ceil((N + n_in) / D) - m_first, output m_first + i at ring sample (ring_offset + i) mod capacity.
// A TILE is `tile` consecutive outputs of a push (the last one fewer): one workgroup, which needs the `span` inputs
// j0 .. j0 + span - 1, j0 = m0*D - (T-1), span = (count-1)*D + T.  Input j of a push lies in the push's block at j - N when that is
// >= 0 and in the HISTORY (the last T-1 raw inputs before the push, oldest first) at (T-1) + (j - N) otherwise; a tile never
// reaches behind the history nor past the push.  After the push the history is the last T-1 inputs again: element i is block
// sample n_in - (T-1) + i, or -- a push shorter than T-1 -- the old history's element i + n_in.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDR_DDC_HD __host__ __device__
#else
#define SDR_DDC_HD
#endif

namespace sdr {

constexpr int kDdcMaxTaps = 512;
constexpr int kDdcMaxDecimation = 64;
constexpr int kDdcThreads = 256;
// Mixed inputs (16 bytes each) a workgroup keeps in LDS: 63 KiB, two workgroups per CU of 160 KiB with room to spare.
constexpr int kDdcLdsInputs = 4032;
constexpr int kDdcMaxTile = 1024;   // outputs per workgroup at most (four per lane)

struct DdcPush {
    int64_t n_seen;    // N: inputs before this push
    int64_t n_in;
    int64_t m_first;   // first output of the push
    int64_t n_out;
    int D, T;
};

SDR_DDC_HD inline int64_t ddc_ceil_div(int64_t a, int64_t d) { return (a + d - 1) / d; }   // a >= 0

SDR_DDC_HD inline DdcPush ddc_push(int64_t n_seen, int64_t n_in, int D, int T) {
    DdcPush p;
    p.n_seen = n_seen, p.n_in = n_in, p.D = D, p.T = T;
    p.m_first = ddc_ceil_div(n_seen, D);
    p.n_out = ddc_ceil_div(n_seen + n_in, D) - p.m_first;
    return p;
}

// Outputs per workgroup: as many as kDdcLdsInputs mixed inputs make, kDdcMaxTile at most (>= 56 for T <= 512, D <= 64).
SDR_DDC_HD inline int ddc_tile_outputs(int D, int T) {
    const int t = (kDdcLdsInputs - T) / D + 1;
    return t < kDdcMaxTile ? t : kDdcMaxTile;
}

struct DdcTile {
    int64_t i0;     // first output of the tile, counted from the push's first
    int64_t j0;     // first input it needs (absolute; may be negative: before the stream began)
    int count;      // outputs
    int span;       // inputs
};

SDR_DDC_HD inline int64_t ddc_tiles(const DdcPush& p, int tile) { return ddc_ceil_div(p.n_out, tile); }

SDR_DDC_HD inline DdcTile ddc_tile(const DdcPush& p, int tile, int64_t b) {
    DdcTile t;
    t.i0 = b * tile;
    const int64_t left = p.n_out - t.i0;
    t.count = (int)(left < tile ? left : tile);
    t.j0 = (p.m_first + t.i0) * p.D - (p.T - 1);
    t.span = (t.count - 1) * p.D + p.T;
    return t;
}

// Where input j (absolute) of a tile lies: >= 0 -- sample of the push's block; < 0 -- ~value is the history element.
SDR_DDC_HD inline int64_t ddc_source(const DdcPush& p, int64_t j) {
    const int64_t rel = j - p.n_seen;
    return rel >= 0 ? rel : ~((int64_t)(p.T - 1) + rel);
}

// Where element i (0 <= i < T-1) of the history AFTER a push of n_in comes from: same encoding, the history being the old one.
SDR_DDC_HD inline int64_t ddc_hist_source(int64_t n_in, int T, int i) {
    const int64_t rel = n_in - (T - 1) + i;
    return rel >= 0 ? rel : ~((int64_t)i + n_in);
}

// Ring sample of output i of a push (0 <= ring_offset < capacity, i < n_out <= capacity).
SDR_DDC_HD inline int64_t ddc_ring_pos(int64_t ring_offset, int64_t i, int64_t capacity) {
    const int64_t pos = ring_offset + i;
    return pos >= capacity ? pos - capacity : pos;
}

}  // namespace sdr
