// Host-side proof of the work list of the fused map-free PCPS sweep and of the key sdr_pcps_fused_sweep re-uses it by
// (sydr_amd/csrc/pcps_fused_work.h), built with `hipcc --cuda-host-only` under the address and undefined-behaviour sanitizers
// (`make check-sanitize`).  Exhaustive over n_prn 1..40, Doppler bins 1..90, terms 1 (N = 25 000) and 2 (N = 50 000), blocks of
// 4, 16 and 32 bins:
//  (a) the key: two searches whose keys compare equal have the same list and the same first[9] -- a key that leaves out
//      something the list depends on fails here -- and two different requests never have equal keys;
//  (b) every (PRN, virtual bin) is covered by ONE whole unit, or by units whose rounds are exactly {0, 1, 2, 3, 4}, each once;
//  (c) the record slots are a permutation of [0, n_prn * per_prn), PRN p's in [p * per_prn, (p + 1) * per_prn), and
//      per_prn * SDR_PCPS_FUSED_RECORDS is what the second sweep reads a PRN's records with (fused_records_per_prn);
//  (d) first[] starts at 0, never decreases and ends at the list's length.
//   usage: fused_work_check              -> "ok <cases>" and exit status 0, or the first mismatch and 1
//          fused_work_check three-int    -> part (a) alone with the key as it was before WorkKey -- (n_prn, vbins, block_bins):
//                                           prints the pairs it wrongly holds equal and exits 1 (the proof that (a) bites)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sydr_amd/csrc/pcps_fused_work.h"

using namespace fusedwork;

struct Request {
    int n_prn, nbins, terms, block_bins;
    WorkKey key;
    std::vector<WorkItem> order;
    int first[9];
    int per_prn;
};

static bool same_list(const Request& a, const Request& b) {
    if (a.order.size() != b.order.size() || a.per_prn != b.per_prn) return false;
    for (size_t i = 0; i < a.order.size(); ++i)
        if (a.order[i].prn != b.order[i].prn || a.order[i].bin != b.order[i].bin || a.order[i].round != b.order[i].round ||
            a.order[i].record != b.order[i].record)
            return false;
    for (int x = 0; x < 9; ++x)
        if (a.first[x] != b.first[x]) return false;
    return true;
}

static bool key_three_int(const WorkKey& a, const WorkKey& b) { return a.n_prn == b.n_prn && a.vbins == b.vbins && a.block_bins == b.block_bins; }
static bool key_whole(const WorkKey& a, const WorkKey& b) { return a == b; }

static int check_list(const Request& r) {
    const int n_prn = r.n_prn, vbins = r.terms * r.nbins, pieces = fused_pieces(r.terms);
    const std::vector<WorkItem>& order = r.order;
#define FAIL(...) return printf("n_prn %d bins %d terms %d block %d: ", n_prn, r.nbins, r.terms, r.block_bins), printf(__VA_ARGS__), printf("\n"), 1
    // (d)
    if (r.first[0] != 0 || r.first[8] != (int)order.size()) FAIL("first[] spans [%d, %d) of %zu", r.first[0], r.first[8], order.size());
    for (int x = 0; x < 8; ++x)
        if (r.first[x + 1] < r.first[x]) FAIL("first[%d] = %d > first[%d] = %d", x, r.first[x], x + 1, r.first[x + 1]);
    // (b): per (PRN, virtual bin) the whole units and a count per round
    std::vector<int> whole((size_t)n_prn * vbins, 0), rounds((size_t)n_prn * vbins * 5, 0);
    // (c)
    if (r.per_prn * kRecordsPerUnit != fused_records_per_prn(n_prn, r.nbins, r.terms))
        FAIL("per_prn %d x %d records, the second sweep reads %d", r.per_prn, kRecordsPerUnit, fused_records_per_prn(n_prn, r.nbins, r.terms));
    std::vector<int> slot((size_t)n_prn * r.per_prn, 0);
    for (const WorkItem& w : order) {
        if (w.prn < 0 || w.prn >= n_prn || w.bin < 0 || w.bin >= vbins) FAIL("unit (%d, %d) outside the search", w.prn, w.bin);
        const size_t cell = (size_t)w.prn * vbins + w.bin;
        if (w.round < 0) {
            if (w.round != -1) FAIL("round code %d", w.round);
            ++whole[cell];
        } else {
            const int r0 = w.round & 15, r1 = w.round >> 4;      // (pcps_fused.h one_unit: r1 = 15 -- one round only)
            if (r0 > 4 || (r1 > 4 && r1 != 15) || r1 == r0) FAIL("round code %d", w.round);
            ++rounds[cell * 5 + r0];
            if (r1 != 15) ++rounds[cell * 5 + r1];
        }
        if (w.record < w.prn * r.per_prn || w.record >= (w.prn + 1) * r.per_prn) FAIL("slot %d of PRN %d, per_prn %d", w.record, w.prn, r.per_prn);
        ++slot[w.record];
    }
    for (size_t i = 0; i < slot.size(); ++i)
        if (slot[i] != 1) FAIL("record slot %zu used %d times", i, slot[i]);
    int units = 0;
    for (size_t cell = 0; cell < whole.size(); ++cell) {
        int each_once = 1, none = 1;
        for (int q = 0; q < 5; ++q) each_once &= rounds[cell * 5 + q] == 1, none &= rounds[cell * 5 + q] == 0;
        if (!((whole[cell] == 1 && none) || (whole[cell] == 0 && each_once)))
            FAIL("(PRN %zu, bin %zu): %d whole units, rounds %d %d %d %d %d", cell / vbins, cell % vbins, whole[cell], rounds[cell * 5],
                 rounds[cell * 5 + 1], rounds[cell * 5 + 2], rounds[cell * 5 + 3], rounds[cell * 5 + 4]);
        units += whole[cell] ? 1 : pieces;
    }
    if (units != (int)order.size() || units != n_prn * r.per_prn) FAIL("%d units, list of %zu, %d slots", units, order.size(), n_prn * r.per_prn);
#undef FAIL
    return 0;
}

int main(int argc, char** argv) {
    const bool three_int = argc > 1 && !strcmp(argv[1], "three-int");
    bool (*const same_key)(const WorkKey&, const WorkKey&) = three_int ? key_three_int : key_whole;
    long cases = 0, wrong = 0;
    bool named_pair = false;
    const int blocks[3] = {4, 16, 32};
    for (int n_prn = 1; n_prn <= 40; ++n_prn) {
        // every request of this PRN count (keys of different PRN counts differ under either comparison)
        std::vector<Request> reqs;
        for (int nbins = 1; nbins <= 90; ++nbins)
            for (int terms = 1; terms <= 2; ++terms)
                for (int block_bins : blocks) {
                    Request r;
                    r.n_prn = n_prn, r.nbins = nbins, r.terms = terms, r.block_bins = block_bins;
                    r.key.n_prn = n_prn, r.key.vbins = terms * nbins, r.key.block_bins = block_bins, r.key.pieces = fused_pieces(terms);
                    // the list as the plan states it, and as the sweep makes it from the key: one and the same
                    int bins_whole;
                    const int units = fused_plan(n_prn, terms * nbins, &bins_whole, fused_pieces(terms));
                    r.per_prn = make_work_list(n_prn, terms * nbins, bins_whole, r.order, r.first, fused_pieces(terms), block_bins);
                    Request k = r;
                    k.per_prn = make_work_list(r.key, k.order, k.first);
                    if (units != r.per_prn || !same_list(r, k)) return printf("n_prn %d bins %d terms %d block %d: the key's list differs\n", n_prn, nbins, terms, block_bins), 1;
                    // the key the sweep computes (shared spectra or not) is one of these
                    if (block_bins == 4 && !(fused_work_key(n_prn, nbins, terms, false) == r.key)) return printf("fused_work_key, no classes\n"), 1;
                    if (block_bins == (terms == 2 ? 32 : 16) && !(fused_work_key(n_prn, nbins, terms, true) == r.key)) return printf("fused_work_key, classes\n"), 1;
                    if (!three_int && check_list(r)) return 1;
                    reqs.push_back(std::move(r));
                    ++cases;
                }
        // (a) every pair of requests
        for (size_t i = 0; i < reqs.size(); ++i)
            for (size_t j = i + 1; j < reqs.size(); ++j, ++cases) {
                const Request &a = reqs[i], &b = reqs[j];
                if ((a.key == b.key) != !(a.key != b.key)) return printf("== and != disagree\n"), 1;
                // keys that differ in any one member are unequal, whatever the lists
                const bool differ = a.key.n_prn != b.key.n_prn || a.key.vbins != b.key.vbins || a.key.block_bins != b.key.block_bins || a.key.pieces != b.key.pieces;
                if (differ == (a.key == b.key)) return printf("operator== misses a member\n"), 1;
                if (!same_key(a.key, b.key) || same_list(a, b)) continue;
                if (!three_int) return printf("n_prn %d: (bins %d, terms %d, block %d) and (bins %d, terms %d, block %d): equal keys, different lists\n", n_prn,
                                              a.nbins, a.terms, a.block_bins, b.nbins, b.terms, b.block_bins), 1;
                ++wrong;
                const bool named = n_prn == 4 && a.block_bins == 4 && b.block_bins == 4 &&
                                   ((a.terms == 1 && a.nbins == 82 && b.terms == 2 && b.nbins == 41) || (a.terms == 2 && a.nbins == 41 && b.terms == 1 && b.nbins == 82));
                if (named || wrong <= 3)
                    printf("equal keys, different lists: n_prn %d block %d: (terms %d, %d bins: %d units per PRN) and (terms %d, %d bins: %d units per PRN)\n", n_prn,
                           a.block_bins, a.terms, a.nbins, a.per_prn, b.terms, b.nbins, b.per_prn);
                named_pair |= named;
            }
    }
    if (three_int) {
        printf("three-int key: %ld pairs of requests share a key and differ in their lists; (n_prn 4, terms 1, 82 bins) / (n_prn 4, terms 2, 41 bins) %s\n",
               wrong, named_pair ? "among them" : "NOT among them");
        return 1;
    }
    printf("ok %ld\n", cases);
    return 0;
}
