// The plan of one acquisition search (sdr_pcps, sdr_pcps_spectra, sdr_pcps_signal; the deep search takes the map route's): which of the four
// routes it takes, how one transform is done, how many PRNs go into one inverse sweep, whether two streams alternate, how many
// class spectra are shared, the chirp-z length and every buffer size -- and the layout of the result block the searches and
// the peak comparisons hand their results over in.  Host arithmetic only, no HIP runtime and no engine in sight:
// tests/csrc/pcps_plan_check.hip compiles it alone (`make check-sanitize`, tests/test_pcps_plan.py).
//
// The constants the planner shares with the kernels are defined HERE, once; the kernel headers (pcps_fft.h, pcps_peak.h,
// pcps_fast.h, pcps_fastn.h) take them from here, and engine_internal.h the two record sizes of the fused searches.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pcps_fused_work.h"

// pcps_fused.hip: (value, index) records the fused sweep leaves per unit of work, one per wave; pcps_fused10k.h: bytes of
// scratch per (PRN, bin) of the fused 10 MHz search
#define SDR_PCPS_FUSED_RECORDS 8
#define SDR_PCPS_FUSED10K_RECORD_BYTES 32
// Infinity Cache budget (MB) of the intermediates of two inverse sweeps alive at a time (plan_pcps)
#ifndef SDR_PCPS_OVERLAP_MB
#define SDR_PCPS_OVERLAP_MB 100ll
#endif
// Tile widths of the four-step pair: 8 columns for kernel A (128-byte runs), 4 rows for kernel B -- its LDS footprint is the
// larger one (N2 >= N1) and halving it (5 instead of 2 workgroups per CU at N = 25000) measured 9 % faster than 8.
#ifndef SDR_PCPS_ROW_TILE
#define SDR_PCPS_ROW_TILE 4
#endif
#ifndef SDR_PCPS_COL_TILE
#define SDR_PCPS_COL_TILE 8
#endif
// rows per workgroup of the register-resident row kernels (pcps_fast.h): 120 of 128 threads hold 20 points each
#ifndef SDR_PCPS_FAST_ROWT
#define SDR_PCPS_FAST_ROWT 12
#endif

namespace pcps {

static_assert(SDR_PCPS_FUSED_RECORDS == fusedwork::kRecordsPerUnit, "one record per wave of a unit");

constexpr int kThreads = 256;          // threads of a workgroup of the general transform and peak kernels
constexpr int kPeakParts = 64;         // parts a PRN's map is cut into for its first maximum (argmax_part_kernel)
constexpr size_t kBestBytes = 16;      // sizeof(Best): a (value, index) record (pcps_codelets.h)
constexpr int kRowTile = SDR_PCPS_ROW_TILE;
constexpr int kMaxGenericRadix = 64;   // largest prime the O(R^2) radix pass takes

// the register-resident kernels' geometry: N = 125 x 200 (pcps_fast.h) and N = N1 x 200 (pcps_fastn.h)
namespace fast25k {
constexpr int N1 = 125, N2 = 200, N = 25000;
constexpr int kRowT = SDR_PCPS_FAST_ROWT;
constexpr int kRowThreads = (10 * kRowT + 63) / 64 * 64;
constexpr int kRowTiles = (N1 + kRowT - 1) / kRowT;
constexpr int kRecordsPerTransform = kRowTiles * (kRowThreads / 64);
}  // namespace fast25k
namespace fastn {
constexpr int N2 = 200;
constexpr int kRowT = fast25k::kRowT;
constexpr int kRowThreads = fast25k::kRowThreads;
constexpr int row_tiles(int n1) { return (n1 + kRowT - 1) / kRowT; }
constexpr int records_per_transform(int n1) { return row_tiles(n1) * (kRowThreads / 64); }
inline bool handles(int N) { return N == 4000 || N == 10000 || N == 50000; }
inline int records(int N) { return records_per_transform(N / N2); }
}  // namespace fastn

// ---- the result block: [bin][code][ratio](+value) per PRN, then the slot numbers, then the done words -- on the device
// (pcps_res) or page-locked; the searches, sdr_two_peak_compare and sdr_two_peak_compare_ss lay theirs out with this alone.
struct ResultBlock {
    long long *bin = nullptr, *code = nullptr;
    double *ratio = nullptr, *value = nullptr;    // value: the deep search's peak value column
    int32_t* slots = nullptr;
    unsigned* done = nullptr;
    size_t bytes = 0;
};
// (base == nullptr: the size alone)
inline ResultBlock result_block(int n_prn, bool value, bool slots, bool done, void* base) {
    ResultBlock r;
    const size_t n = (size_t)n_prn;
    const size_t cols = n * (value ? 4 : 3) * sizeof(double);
    r.bytes = cols + (slots ? n * sizeof(int32_t) : 0) + (done ? n * sizeof(unsigned) : 0);
    if (!base) return r;
    r.bin = (long long*)base;
    r.code = r.bin + n;
    r.ratio = (double*)(r.code + n);
    if (value) r.value = r.ratio + n;
    char* behind = (char*)base + cols;
    if (slots) r.slots = (int32_t*)behind, behind += n * sizeof(int32_t);
    if (done) r.done = (unsigned*)behind;
    return r;
}

// The engine's switches the planner reads (pcps.hip fills one from the engine: pcps_switches).
struct PcpsSwitches {
    bool fused = true;               // "pcps_fused"
    bool no_fast = false;            // "pcps_no_fast"
    bool force_map = false;          // "pcps_force_map"
    bool no_overlap = false;         // "pcps_no_overlap"
    bool no_shared_spectra = false;  // "pcps_no_shared_spectra"
    int prn_chunk = 0;               // "pcps_prn_chunk": PRNs per inverse sweep (0 = as many as the work buffers hold)
    bool prof = false;               // the per-stage profiling scopes record: the search stays on one stream
};

inline std::vector<int> factor_radices(int64_t N) {
    std::vector<int> r;
    int64_t n = N;
    while (n % 5 == 0) { r.push_back(5); n /= 5; }
    while (n % 3 == 0) { r.push_back(3); n /= 3; }
    while (n % 8 == 0) { r.push_back(8); n /= 8; }
    while (n % 4 == 0) { r.push_back(4); n /= 4; }
    while (n % 2 == 0) { r.push_back(2); n /= 2; }
    for (int p = 7; (int64_t)p <= n && p <= kMaxGenericRadix; p += 2)
        while (n % p == 0) { r.push_back(p); n /= p; }
    if (n != 1) r.clear();
    return r;
}

struct Radices {
    int n;
    int r[10];
};

// Four-step transform: N = N1*N2, both sub-transforms done in LDS (pcps_fft.h)
struct FourStep {
    bool ok = false;
    int N1 = 0, N2 = 0;
    Radices rad1{}, rad2{};
};

inline FourStep plan_four_step(int N) {
    FourStep f;
    int best = 0;
    for (int d = 2; (int64_t)d * d <= N; ++d)
        if (N % d == 0) best = d;  // largest divisor <= sqrt(N)
    if (best < 4 || N / best > 512) return f;
    std::vector<int> r1 = factor_radices(best), r2 = factor_radices(N / best);
    if (r1.empty() || r2.empty() || r1.size() > 10 || r2.size() > 10) return f;
    f.N1 = best;
    f.N2 = N / best;
    f.rad1.n = (int)r1.size();
    f.rad2.n = (int)r2.size();
    for (size_t i = 0; i < r1.size(); ++i) f.rad1.r[i] = r1[i];
    for (size_t i = 0; i < r2.size(); ++i) f.rad2.r[i] = r2[i];
    f.ok = true;
    return f;
}

// How a transform of length N is done: the four-step pair where the planner splits N, else one kernel per radix pass
// (plan_pcps).  `fast`: the register-resident kernels of either header run the inverse transforms of a search at 4 / 10 /
// 25 / 50 MHz instead (they split N as N1 x 200 themselves).
enum FastKernels { FAST_NONE = 0, FAST_25K, FAST_N };
struct Xform {
    std::vector<int> radices;
    FourStep four;
    FastKernels fast = FAST_NONE;
};
// per-wave records one map-free inverse sweep leaves per transform
inline int records_per_transform(const FourStep& f) { return ((f.N1 + kRowTile - 1) / kRowTile) * (kThreads / 64); }

// ---- shared spectra (round 5).  x mixed with exp(-2 pi i (f - q / T) t) is x mixed with f, times exp(+2 pi i q n / N): its
// spectrum is the other's, circularly shifted by q elements.  Bins P apart whose distance P * step is a whole number q of
// transform bins (1 / T = fs / N: 250 Hz steps over 1 ms -> P = 4, q = 1; 300 Hz -> P = 10, q = 3) therefore share ONE
// forward transform: a search transforms its first P bins and reads bin c + P j as the spectrum of bin c shifted by j q
// (acquisition.py:42-59 transforms every bin; the values agree to rounding, ~1e-15 relative, like any two orders of the same
// additions).  4 forward transforms instead of 41 for the headline grid, and the spectra side of the inverse sweep's operands
// is 4 arrays.  The class spectra are written with the row's last H elements in front of it (PassArgs::halo), so that a
// shift is a contiguous read H - j q elements into the row.
struct SharedSpectra {
    int P = 0, q = 0, H = 0;            // P == 0: every bin has its own transform
};
inline SharedSpectra plan_shared_spectra(const PcpsSwitches& e, int nbins, int N, double fs, double bin_delta) {
    SharedSpectra s;
    if (e.no_shared_spectra || !(bin_delta > 0.0)) return s;
    for (int P = 1; P <= 64 && 2 * P <= nbins; ++P) {
        const double v = (double)P * bin_delta * (double)N / fs, r = std::nearbyint(v);
        if (r >= 1.0 && std::fabs(v - r) <= 1e-9 * r && r * (double)((nbins - 1) / P) <= 4096.0) {
            s.P = P, s.q = (int)r;
            s.H = s.q * ((nbins - 1) / P);
            break;
        }
    }
    return s;
}

// ---- one search, planned once: its route, how one transform is done, how the PRNs are cut and every buffer size
enum Route {
    ROUTE_FUSED10K,  // N = 10 000, indices and ratio only: the forward transforms, then one launch for the rest (pcps_fused10k.h)
    ROUTE_FUSED,     // map-free at N = 25 000 / 50 000, a round of 256 transforms or more: fused sweep + fused second sweep
    ROUTE_SWEEPS,    // map-free: inverse sweeps that leave per-wave records, then the winning row of every PRN again
    ROUTE_MAP,       // the map accumulated over the blocks, then its peaks (also every radix-pass and chirp-z length)
};
struct PcpsPlan {
    int N = 0, spc = 0, nbins = 0, coh = 1, noncoh = 1, n_prn = 0;
    double fs = 0.0, bin_start = 0.0, bin_delta = 0.0;
    // sdr_pcps_signal: N is the transform length T; the map keeps the first `cols` lags of every transform at row pitch
    // `cols`, and the blocks of the window advance by `cols` samples (cols == N: the circular search, all of the above alike);
    // chip_rate is what the replica is resampled with
    int cols = 0;
    double chip_rate = 1.023e6;
    Xform xf;                  // the length-N transform
    int M = 0;                 // chirp-z (Bluestein) length, 0 = none; xm its transform (plain loads: never `fast`)
    Xform xm;
    Route route = ROUTE_MAP;
    int terms = 0;             // ROUTE_FUSED: operand terms per point (pcps_fused.h)
    int prn_chunk = 0;         // PRNs per inverse sweep
    bool overlap = false;      // ROUTE_SWEEPS: the sweeps alternate between two streams
    SharedSpectra sh;          // (ROUTE_FUSED10K, ROUTE_FUSED only)
    bool done_words = false;   // the search ends in a kernel that raises a done word per PRN behind its results
    int records_sweep = 0;     // per-wave records a transform of the main inverse sweep leaves
    int records_per_prn = 0;   // ... the first sweep leaves per PRN (map-free routes)
    int records_second = 0;    // ... a transform of the second sweep leaves
    size_t tbytes = 0, fwd_bytes = 0, work_bytes = 0, code_bytes = 0, code2_bytes = 0, map_bytes = 0, csum_bytes = 0,
           part_bytes = 0, res_bytes = 0, pinned_bytes = 0, blu_bytes = 0, blu_work_bytes = 0;
};

// operand terms per point of the one-workgroup-per-transform sweep: 1 at N = 25 000, 2 at N = 50 000 (a radix-2 step in
// front of two 25 000-point transforms, pcps_fused.h), 0 = the sweep does not serve this length
inline int fused_terms(const PcpsSwitches& e, const FourStep& f) {
    if (!e.fused || !f.ok || e.no_fast) return 0;
    if (f.N1 == fast25k::N1 && f.N2 == fast25k::N2) return 1;
    return f.N1 * f.N2 == 2 * fast25k::N ? 2 : 0;
}
// The fused sweep takes a map-free search whole when it fills at least one round of its 256 persistent workgroups (a
// smaller search is quicker through the two-kernel path: ~8 us + 0.19 us per transform against ~35 us per round).
inline bool fused_takes(const PcpsSwitches& e, const FourStep& f, int n_prn, int nbins) {
    return fused_terms(e, f) * n_prn * nbins >= 256;
}
inline Xform plan_xform(const PcpsSwitches& e, int N) {
    Xform t;
    t.radices = factor_radices(N);
    t.four = plan_four_step(N);
    // (the register-resident kernels of either header serve this length: they split it as N1 x 200 themselves)
    if (t.four.ok && !e.no_fast)
        t.fast = t.four.N1 == fast25k::N1 && t.four.N2 == fast25k::N2 ? FAST_25K : fastn::handles(N) ? FAST_N : FAST_NONE;
    return t;
}
// A code length the mixed-radix planner cannot factor (prime factor above 64) goes through the chirp-z transform with
// M = the next 2^a 3^b 5^c >= 2N-1.
inline int chirpz_length(int N) {
    for (int64_t m = 2 * (int64_t)N - 1;; ++m) {
        int64_t q = m;
        for (int f : {2, 3, 5})
            while (q % f == 0) q /= f;
        if (q == 1) return (int)m;
    }
}

// The request (samples per code N and per chip spc, Doppler grid, integration, PRNs, map wanted) and the engine's switches ->
// the plan.  The zero-padded search of sdr_pcps_signal hands in the transform length as N and the samples per code as `cols`
// (0: N), and takes the map route: its last inverse pass stores the first `cols` lags alone.
inline PcpsPlan plan_pcps(const PcpsSwitches& e, int N, int spc, double fs, int nbins, double bin_start, double bin_delta, int coh,
                          int noncoh, int n_prn, bool want_map, int cols = 0, double chip_rate = 1.023e6) {
    const size_t kComplexBytes = 2 * sizeof(double);
    PcpsPlan p;
    p.N = N, p.fs = fs, p.nbins = nbins, p.bin_start = bin_start, p.bin_delta = bin_delta;
    p.coh = coh, p.noncoh = noncoh, p.n_prn = n_prn;
    p.spc = spc;
    p.cols = cols > 0 ? cols : N;
    p.chip_rate = chip_rate;
    const bool padded = p.cols != N;
    p.xf = plan_xform(e, N);
    const FourStep& four = p.xf.four;
    if (p.xf.radices.empty()) {
        p.M = chirpz_length(N);
        p.xm = plan_xform(e, p.M);
    }

    // Work-buffer sizing: transforms in flight per inverse sweep are capped at 8 GiB per buffer.
    const size_t tbytes = (size_t)N * kComplexBytes;
    const size_t mbytes = (size_t)p.M * kComplexBytes;  // (0 without the chirp-z path)
    int prn_chunk = (int)std::min<int64_t>(n_prn, std::max<int64_t>(1, (int64_t)((8ull << 30) / (std::max(tbytes, mbytes) * nbins))));
    if ((int64_t)prn_chunk * nbins > 65535) prn_chunk = std::max(1, 65535 / nbins);
    // Indices and ratio only, one block, four-step transform available: the map is never materialised.
    const bool map_free = !want_map && coh == 1 && noncoh == 1 && !p.M && four.ok && !e.force_map && !padded;
    // The column kernel of an inverse sweep writes 16 N bytes per (PRN, bin) and the row kernel reads them back: as
    // many PRNs per sweep as keep that intermediate inside the 256 MB Infinity Cache (a 200 MB budget), in sweeps of
    // equal size -- 32 PRNs x 41 bins x 25 000: three sweeps of 11 / 11 / 10 PRNs instead of one of 525 MB, measured
    // 0.40 -> 0.34 ms per acquisition (tools/pcps_breakdown.py <chunk>: 12: 0.341, 11: 0.339, 10: 0.348, 8: 0.357,
    // 16: 0.379, 6: 0.392 -- the smaller the sweep, the larger the share of its partial last round of workgroups).
    if (map_free && e.prn_chunk == 0) {
        const int64_t per_prn = (int64_t)tbytes * nbins;
        // (two sweeps alive at a time where they alternate between two streams: pcps.hip run_sweeps)
        const bool two_alive = p.xf.fast && !e.prof && !e.no_overlap;
        const int fit = (int)std::max<int64_t>(1, ((two_alive ? SDR_PCPS_OVERLAP_MB : 200ll) << 20) / per_prn);
        if (fit < prn_chunk) {
            const int sweeps = (n_prn + fit - 1) / fit;
            prn_chunk = (n_prn + sweeps - 1) / sweeps;
        }
    }
    if (e.prn_chunk > 0) prn_chunk = std::min(prn_chunk, e.prn_chunk);
    p.prn_chunk = prn_chunk;
    // (32 units and more: below that the two-kernel path's many small workgroups finish sooner than one unit per CU)
    const bool fused10k = !want_map && coh == 1 && N == 10000 && !p.M && four.ok && !e.force_map && e.fused &&
                          !e.no_fast && (int64_t)n_prn * nbins >= 32 && !padded;
    const bool fused = map_free && fused_takes(e, four, n_prn, nbins);
    p.route = fused10k ? ROUTE_FUSED10K : fused ? ROUTE_FUSED : map_free ? ROUTE_SWEEPS : ROUTE_MAP;
    p.terms = fused ? fused_terms(e, four) : 0;
    p.overlap = p.route == ROUTE_SWEEPS && p.xf.fast && n_prn > prn_chunk && !e.prof && !e.no_overlap;
    // (shared spectra: the shipped 300 Hz grid at 10 MHz has ten classes -- 10 transforms per block instead of 34)
    if (fused10k || fused) p.sh = plan_shared_spectra(e, nbins, N, fs, bin_delta);
    // the searches that end in the fused second sweep or the fused 10 MHz search raise a word per PRN behind its results:
    // those are waited for instead of the stream's signal, which follows the last store by ~9 us (the receiver tick's finding)
    p.done_words = fused10k || fused;
    // (per-wave records a transform of the main sweep leaves: it may run the register-resident kernels)
    p.records_sweep = p.xf.fast == FAST_25K ? fast25k::kRecordsPerTransform
                      : p.xf.fast ? fastn::records(N) : records_per_transform(four);
    p.records_per_prn = fused ? fusedwork::fused_records_per_prn(n_prn, nbins, p.terms) : nbins * p.records_sweep;
    p.records_second = records_per_transform(four);

    p.tbytes = tbytes;
    p.work_bytes = tbytes * (size_t)std::max(fused10k ? nbins * noncoh : prn_chunk * nbins, std::max(n_prn, nbins));
    p.fwd_bytes = tbytes * (size_t)std::max(fused10k ? nbins * noncoh : nbins, n_prn);
    p.code_bytes = tbytes * n_prn;
    p.code2_bytes = p.terms == 2 ? 2 * tbytes * n_prn : 0;
    // (the fused sweep leaves at most 5 x SDR_PCPS_FUSED_RECORDS records per transform, twice that at N = 50 000)
    const size_t n_records = map_free ? (size_t)n_prn * (nbins + 1) * std::max(std::max(p.records_second, p.records_sweep), 10 * SDR_PCPS_FUSED_RECORDS) + n_prn : 0;
    p.map_bytes = (size_t)n_prn * ((map_free || fused10k) ? 1 : nbins) * p.cols * sizeof(double);
    p.csum_bytes = coh > 1 ? (size_t)n_prn * nbins * tbytes : 0;
    p.part_bytes = std::max(std::max((size_t)n_prn * kPeakParts, n_records) * kBestBytes,
                            fused10k ? (size_t)n_prn * nbins * SDR_PCPS_FUSED10K_RECORD_BYTES : 0);
    // [results: bin, code, ratio per PRN][slot numbers] on the device; page-locked: the same and the done words
    p.res_bytes = result_block(n_prn, false, true, false, nullptr).bytes;
    p.pinned_bytes = result_block(n_prn, false, true, true, nullptr).bytes;
    if (p.M) {
        p.blu_bytes = tbytes + 3 * mbytes;
        p.blu_work_bytes = mbytes * (size_t)std::max(2, std::max(prn_chunk * nbins, std::max(n_prn, nbins)));
    }
    return p;
}

}  // namespace pcps
