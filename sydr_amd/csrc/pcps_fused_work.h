// How the fused map-free PCPS sweep (pcps_fused.h) cuts a search into units of work: the plan (whole transforms and left-over
// rounds), the work list in processing order with its record slots, and the KEY of that list -- everything the list and the
// XCDs' shares of it are a function of, which is what sdr_pcps_fused_sweep compares before it re-uses the list it has on the
// device.  Host arithmetic only, no kernel in sight: tests/csrc/fused_work_check.hip compiles it alone (`make check-sanitize`).
#pragma once

#include <vector>

namespace fusedwork {

constexpr int kSlotsPerXcd = 32;              // persistent workgroups of an XCD: one step of its share of the list
constexpr int kWorkgroups = 8 * kSlotsPerXcd; // ... and of the launch: one round of transforms
constexpr int kRecordsPerUnit = 8;            // (value, index) records a unit leaves: one per wave (SDR_PCPS_FUSED_RECORDS)

// One unit of work of a persistent workgroup: a whole (PRN, bin) transform, or -- for the transforms left over when the
// search is not a whole number of rounds of 256 -- ONE of a transform's five rounds: the column stage then computes that
// round's fifth of its outputs only (all operands are still read), so that the tail of the launch is a fifth of a round
// on 5 x as many compute units.  `record`: where its records go (PRN-major for the peak kernel).
struct WorkItem {
    int prn, bin, round, record;
};

// units a left-over transform is cut into: its five rounds at N = 25 000; rounds {0, 1}, {2, 3}, {4} at N = 50 000
inline int fused_pieces(int terms) { return terms == 2 ? 3 : 5; }

// How the fused sweep cuts a search of n_prn x nbins transforms: whole transforms for the bins that fill whole rounds of
// its 256 workgroups, single rounds for the rest (returns the units, and so the record sets, per PRN the sweep leaves).
// (nbins: virtual bins -- terms x the Doppler bins, a unit at N = 50 000 being one parity of a transform)
inline int fused_plan(int n_prn, int nbins, int* bins_whole, int pieces) {
    const int rounds = (n_prn * nbins) / kWorkgroups;
    int bw = rounds > 0 ? (kWorkgroups * rounds) / n_prn : 0;
    if (bw > nbins) bw = nbins;
    // (more than a round's worth left over -- few PRNs, many bins -- : cutting buys nothing, whole transforms throughout)
    if (n_prn * (nbins - bw) > kWorkgroups) bw = nbins;
    *bins_whole = bw;
    return bw + pieces * (nbins - bw);
}

// records per PRN the sweep leaves (pcps_plan.h records_per_prn: what the second sweep reads a PRN's records with)
inline int fused_records_per_prn(int n_prn, int nbins, int terms) {
    int bw;
    return fused_plan(n_prn, terms * nbins, &bw, fused_pieces(terms)) * kRecordsPerUnit;
}

// What a work list and its first[9] are a function of (bins_whole follows from n_prn, vbins and pieces: fused_plan).  Two
// searches may share a list exactly when their keys are equal: a member left out here is a list re-used where it is wrong
// (pieces was: 25 MHz over 2 B bins and 50 MHz over B bins have the same vbins, and without shared spectra the same block).
struct WorkKey {
    int n_prn = 0;        // 0: no list yet
    int vbins = 0;        // terms x Doppler bins
    int block_bins = 0;   // bins of a block of 32 whole transforms
    int pieces = 0;       // units of a left-over transform
    bool operator==(const WorkKey& o) const {
        return n_prn == o.n_prn && vbins == o.vbins && block_bins == o.block_bins && pieces == o.pieces;
    }
    bool operator!=(const WorkKey& o) const { return !(*this == o); }
};
// (shared spectra: see make_work_list.  Measured, ms of kernels per 32-PRN x 41-bin call with blocks of 4 / 8 / 16 / 32 bins:
// N = 25 000 0.2165 / 0.2116 / 0.2118 / 0.2144, N = 50 000 0.4834 / 0.4790 / 0.4705 / 0.4665)
inline WorkKey fused_work_key(int n_prn, int nbins, int terms, bool shared_spectra) {
    WorkKey k;
    k.n_prn = n_prn;
    k.vbins = terms * nbins;
    k.block_bins = shared_spectra ? (terms == 2 ? 32 : 16) : 4;
    k.pieces = fused_pieces(terms);
    return k;
}

// Processing order and record slots of a search over bins [0, nbins) x n_prn PRNs.  The first `bins_whole` bins are done
// as whole transforms: blocks of 4 bins x 8 PRNs (32 transforms = one round of an XCD's 32 workgroups, so that the
// operands an XCD has in flight mostly sit in its L2), dealt to the XCDs in contiguous eighths; the transforms of the
// remaining bins are cut into their five rounds, dealt out behind the whole ones (a workgroup's last, short unit).
// Record slots are PRN-major: PRN p owns slots [p * per_prn, (p + 1) * per_prn), per_prn = bins_whole + 5 (nbins - bins_whole).
// (every argument is stated: the library builds its list from a WorkKey alone, below)
inline int make_work_list(int n_prn, int nbins, int bins_whole, std::vector<WorkItem>& order, int first[9], int pieces,
                          int block_bins) {
    // block_bins: bins of a block of 32 whole transforms (x 32 / block_bins PRNs).  4 x 8 shares 4 spectra + 8 code spectra;
    // with SHARED spectra (pcps_plan.h: a handful of class arrays serve every bin, and stay in the L2s) 16 x 2 shares the classes
    // + 2 code spectra, 32 x 1 the classes + 1: half the operand arrays an XCD has in flight, or fewer.
    const int block_prns = kSlotsPerXcd / block_bins;
    // pieces: 5 = one unit per round; 3 = rounds {0, 1}, {2, 3}, {4} (N = 50 000: the operand stage of a unit costs what four
    // rounds do, and 64 left-over transforms x 3 fit ONE wave of workgroups where x 5 need a wave and a quarter)
    const int per_prn = bins_whole + pieces * (nbins - bins_whole);
    std::vector<WorkItem> whole, parts;
    for (int b0 = 0; b0 < bins_whole; b0 += block_bins)
        for (int p0 = 0; p0 < n_prn; p0 += block_prns)
            for (int b = b0; b < b0 + block_bins && b < bins_whole; ++b)
                for (int p = p0; p < p0 + block_prns && p < n_prn; ++p) whole.push_back({p, b, -1, p * per_prn + b});
    for (int b = bins_whole; b < nbins; ++b)
        for (int p = 0; p < n_prn; ++p)
            for (int u = 0; u < pieces; ++u) {
                const int rounds = pieces == 5 ? (u | 15 << 4) : (u == 2 ? (4 | 15 << 4) : (2 * u | (2 * u + 1) << 4));
                parts.push_back({p, b, rounds, p * per_prn + bins_whole + pieces * (b - bins_whole) + u});
            }
    // XCD x: its eighth of the short units, then its eighth of the whole transforms (its workgroups walk the list in steps
    // of 32)
    order.clear();
    const int nw = (int)whole.size(), np = (int)parts.size();
    first[0] = 0;
    // The short units go FIRST (round 5): three workgroups in four start with one and run the rest of the launch ~3/4 of a
    // unit out of step with the others -- the operand stages of an XCD's 32 workgroups no longer all fall into the same
    // moments -- and no workgroup is left holding a short unit while the others have finished.  Measured, one box, ms of
    // kernels per 32-PRN call: N = 50 000 0.532 -> 0.511, N = 25 000 0.235 -> 0.228.
    constexpr bool parts_first = true;
    for (int x = 0; x < 8; ++x) {
        const int p_lo = (int)(((long long)np * x) / 8), p_hi = (int)(((long long)np * (x + 1)) / 8);
        const int w_lo = (int)(((long long)nw * x) / 8), w_hi = (int)(((long long)nw * (x + 1)) / 8);
        if (parts_first) {
            for (int i = p_lo; i < p_hi; ++i) order.push_back(parts[i]);
            // the XCD's 32 workgroups walk the list 32 items at a time, and the whole transforms come in blocks of 32 that share
            // their operand arrays: the step the short units leave incomplete is filled with the LAST whole transforms, so that
            // every later step is one block again (with the blocks straddling two steps the launch fetched 1.34 instead of
            // 0.87 GB through the fabric at N = 50 000)
            int pad = (kSlotsPerXcd - (p_hi - p_lo) % kSlotsPerXcd) % kSlotsPerXcd;
            if (pad > w_hi - w_lo) pad = w_hi - w_lo;
            for (int i = w_hi - pad; i < w_hi; ++i) order.push_back(whole[i]);
            for (int i = w_lo; i < w_hi - pad; ++i) order.push_back(whole[i]);
        } else {
            for (int i = w_lo; i < w_hi; ++i) order.push_back(whole[i]);
            for (int i = p_lo; i < p_hi; ++i) order.push_back(parts[i]);
        }
        first[x + 1] = (int)order.size();
    }
    return per_prn;
}

// The list of a key (what sdr_pcps_fused_sweep puts on the device); returns the units per PRN.
inline int make_work_list(const WorkKey& k, std::vector<WorkItem>& order, int first[9]) {
    int bins_whole;
    fused_plan(k.n_prn, k.vbins, &bins_whole, k.pieces);
    return make_work_list(k.n_prn, k.vbins, bins_whole, order, first, k.pieces, k.block_bins);
}

}  // namespace fusedwork
