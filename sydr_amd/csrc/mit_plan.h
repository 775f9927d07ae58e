// Index arithmetic of the mitigator (mitigate.hip: pulse blanker and narrow-band excisor behind the down-converter),
// shared by the host that sizes the launches, the kernels and the host check tests/csrc/mit_plan_check.hip.
//
// The converter's outputs are counted m = 0, 1, ... from creation or reset, across pushes: v_m (0 for m < 0), blanked u_m
// (u_m needs v_{m-hold} .. v_{m+lead}), excised y_m (H = N / 2; y_m is the sum of one sample of segment q - 1 and one of
// segment q, q = floor(m / H); segment s is made of u[s H .. s H + N)).  Stream output i is y_{i - L}, L = N + lead (lead
// without the excisor: N = 0), and zero for i < L.  A PUSH brings v_n .. v_{n+k-1} behind n earlier ones and delivers the
// outputs i = n .. n + k - 1.  The oldest v that takes is that of i = n:
//   m = n - L, segment floor(m / H) - 1, whose first u has the index (floor(m / H) - 1) H >= m - (H - 1) - H = n - L - N + 1
//   (equality when m = H - 1 mod H), whose blanker reaches `hold` further back: v_{n - K}, K = 2 N - 1 + lead + hold
// (K = lead + hold without the excisor).  The STATE is therefore the last K values of v, and the push works on the linear
// buffer W = [state, the push's v]: W[x] = v_{n - K + x}.  Of it are made
//   U[x] = u_{j_lo + x}, j_lo = n - K + hold, n_u = K + k - hold - lead of them (every u whose v lie inside W),
//   the segments s_lo .. s_lo + n_seg - 1, s_lo = floor((n - L) / H) - 1, the last one floor((n + k - 1 - L) / H),
// and of those the k outputs.  After the push the state is W[k .. k + K).  Counted by a push, so that every index is counted
// once whatever the cut: the triggers and blanked samples of the u it delivers, indices [cnt_lo, cnt_hi) = [max(0, n - L),
// n + k - L), and the excised bins of the segments that FINISH in it, fin_lo <= s < fin_hi: those with s >= -1 and
// n - L < s H + N <= n + k - L (segments before -1 hold nothing but zeros and feed only outputs i < L).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDR_MIT_HD __host__ __device__
#else
#define SDR_MIT_HD
#endif

namespace sdr {

constexpr int kMitMaxReach = 1024;   // blank_lead, blank_hold at most
constexpr int kMitThreads = 256;
constexpr int kMitBlankTile = 1024;  // outputs of a blanker workgroup (its halo: lead + hold <= 2048 more triggers in LDS)

SDR_MIT_HD inline int64_t mit_floor_div(int64_t a, int64_t d) {   // d > 0
    const int64_t q = a / d;
    return (a % d != 0 && a < 0) ? q - 1 : q;
}

SDR_MIT_HD inline int64_t mit_delay(int N, int lead) { return (int64_t)N + lead; }
SDR_MIT_HD inline int64_t mit_state_length(int N, int lead, int hold) { return (N ? 2 * (int64_t)N - 1 : 0) + lead + hold; }

// Segments s >= -1 whose last sample has been delivered once n outputs have: s H + N <= n - L.
SDR_MIT_HD inline int64_t mit_segments_finished(int64_t n, int N, int lead) {
    if (!N) return 0;
    const int64_t H = N / 2, d = n - mit_delay(N, lead);
    return d < H ? 0 : mit_floor_div(d - N, H) + 2;
}

struct MitPlan {
    int64_t n, k;          // outputs before this push, outputs (= values of v) of this push
    int N, H, lead, hold;  // N = 0: no excisor
    int64_t L, K;
    int64_t j_lo, n_u;     // U[x] = u_{j_lo + x}; made of W[x .. x + hold + lead]
    int64_t s_lo, n_seg;   // segments computed (n_seg = 0 without the excisor or when k = 0)
    int64_t fin_lo, fin_hi;   // ... of which these finish in this push (absolute segment numbers, fin_lo >= -1)
    int64_t cnt_lo, cnt_hi;   // u indices whose triggers / blanked samples this push counts
};

SDR_MIT_HD inline MitPlan mit_plan(int64_t n, int64_t k, int N, int lead, int hold) {
    MitPlan p;
    p.n = n, p.k = k, p.N = N, p.H = N / 2, p.lead = lead, p.hold = hold;
    p.L = mit_delay(N, lead);
    p.K = mit_state_length(N, lead, hold);
    p.j_lo = n - p.K + hold;
    p.n_u = p.K + k - hold - lead;
    p.cnt_lo = n - p.L > 0 ? n - p.L : 0;
    p.cnt_hi = n + k - p.L > p.cnt_lo ? n + k - p.L : p.cnt_lo;
    p.s_lo = p.n_seg = p.fin_lo = p.fin_hi = 0;
    if (N && k > 0) {
        p.s_lo = mit_floor_div(n - p.L, p.H) - 1;
        p.n_seg = mit_floor_div(n + k - 1 - p.L, p.H) - p.s_lo + 1;
        // s H + N > n - L  <=>  s >= floor((n - L - N) / H) + 1;   s H + N <= n + k - L  <=>  s <= floor((n + k - L - N) / H)
        p.fin_lo = mit_floor_div(n - p.L - N, p.H) + 1;
        if (p.fin_lo < -1) p.fin_lo = -1;
        p.fin_hi = mit_floor_div(n + k - p.L - N, p.H) + 1;
        if (p.fin_hi < p.fin_lo) p.fin_hi = p.fin_lo;
    }
    return p;
}

// Where in U segment number s_lo + sl begins (its N inputs follow).
SDR_MIT_HD inline int64_t mit_segment_u(const MitPlan& p, int64_t sl) { return (p.s_lo + sl) * p.H - p.j_lo; }

// Output i of the push (0 <= i < k): the y it is (negative: the stream's first L outputs, which are zero) ...
SDR_MIT_HD inline int64_t mit_output_m(const MitPlan& p, int64_t i) { return p.n + i - p.L; }
// ... with the excisor the sum of B[*a] and B[*b], B = [n_seg][N] the segments' inverse transforms (m >= 0),
SDR_MIT_HD inline void mit_output_terms(const MitPlan& p, int64_t m, int64_t* a, int64_t* b) {
    const int64_t q = mit_floor_div(m, p.H);
    *a = (q - 1 - p.s_lo) * p.N + (m - (q - 1) * p.H);
    *b = (q - p.s_lo) * p.N + (m - q * p.H);
}
// ... without it U[this].
SDR_MIT_HD inline int64_t mit_output_u(const MitPlan& p, int64_t m) { return m - p.j_lo; }

}  // namespace sdr
