// Window arithmetic of sdr_iq_probe (probe.hip), shared by the host that sizes the launches, the kernels that walk the
// window and the host check tests/csrc/probe_window_check.hip.
//
// A window of n samples that starts at ring sample `base` (0 <= base < capacity, 1 <= n <= capacity) is one or two PIECES of
// consecutive ring samples [lo, hi): the second exists when the window crosses the ring's end and starts at sample 0.  The
// moments kernel reads whole 16-byte GRANULES (spg = 16 / bytes per sample of them; the ring is a whole number of granules
// and starts on a granule boundary): a piece is covered by granules first .. first + count - 1, of which the first and the
// last may hold samples outside [lo, hi) -- the ragged head and tail, which the kernel masks sample by sample.  The granules
// of both pieces are numbered 0 .. total - 1, piece 0 first: what the kernel's grid strides over.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDR_PROBE_HD __host__ __device__
#else
#define SDR_PROBE_HD
#endif

namespace sdr {

struct ProbePiece {
    int64_t lo, hi;         // ring samples [lo, hi) of the window (lo == hi: no such piece)
    int64_t first, count;   // granules that cover them
};

struct ProbeWindow {
    ProbePiece piece[2];
    int64_t total;          // granules of both pieces
};

SDR_PROBE_HD inline ProbeWindow probe_window(int64_t base, int64_t n, int64_t capacity, int spg) {
    ProbeWindow w;
    const int64_t end = base + n;   // (<= 2 * capacity: no overflow for any ring that fits a GPU)
    w.piece[0].lo = base;
    w.piece[0].hi = end < capacity ? end : capacity;
    w.piece[1].lo = 0;
    w.piece[1].hi = end > capacity ? end - capacity : 0;
    w.total = 0;
    for (int p = 0; p < 2; ++p) {
        ProbePiece& q = w.piece[p];
        q.first = q.lo / spg;
        q.count = q.hi > q.lo ? (q.hi + spg - 1) / spg - q.first : 0;
        w.total += q.count;
    }
    return w;
}

// Granule number i (0 <= i < total) of the window: the ring granule it is, and the ring samples [*lo, *hi) of it that belong
// to the window (at least one).
SDR_PROBE_HD inline int64_t probe_granule(const ProbeWindow& w, int64_t i, int spg, int64_t* lo, int64_t* hi) {
    const ProbePiece& q = i < w.piece[0].count ? w.piece[0] : w.piece[1];
    const int64_t g = q.first + (i < w.piece[0].count ? i : i - w.piece[0].count);
    const int64_t s0 = g * spg, s1 = s0 + spg;
    *lo = s0 > q.lo ? s0 : q.lo;
    *hi = s1 < q.hi ? s1 : q.hi;
    return g;
}

// Welch segments of nfft samples, hop nfft / 2, inside a window of n samples (0 when the window is shorter than one).
SDR_PROBE_HD inline int64_t probe_segments(int64_t n, int nfft) { return n < nfft ? 0 : (n - nfft) / (nfft / 2) + 1; }

// Ring sample of sample j of segment s.
SDR_PROBE_HD inline int64_t probe_segment_sample(int64_t base, int64_t capacity, int64_t s, int nfft, int j) {
    const int64_t pos = base + s * (nfft / 2) + j;   // < 2 * capacity
    return pos >= capacity ? pos - capacity : pos;
}

}  // namespace sdr
