// Host-side proof of what sdr_iq_cancel checks and derives before it launches (sydr_amd/csrc/cancel_plan.h), built with
// `hipcc --cuda-host-only` under the address and undefined-behaviour sanitizers (`make check-sanitize`):
//  - cancel_mod_diff and cancel_windows_overlap against brute force on small rings, and on indices near 2^62;
//  - cancel_plan fed seeded hostile lists (NaN / Inf / huge parameters, negative and absurd starts and lengths, slots out of
//    range, overlapping and descending epochs, padding anywhere): whatever it accepts lies wholly inside the window, ascends
//    without overlap within a channel, indexes a staged slot (a chip line whose step underflows to 0 is served: one chip), and is exactly the list's non-padding items in order; a list
//    built to be valid is accepted with every item at the offset a plain loop gives it.
//   usage: cancel_plan_check   -> "ok <cases>" and exit status 0, or the first mismatch and 1
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../sydr_amd/csrc/cancel_plan.h"

using namespace sdr;

static uint64_t state = 20260018;
static uint64_t next() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 11;
}

static double hostile_double() {
    const double table[] = {0.0, -0.0, 1.0, -1.0, 0.25575, 1e-300, 1e300, -1e300, 2e9, -2e9, 1e18,
                            std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                            std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::max(), 5e-324};
    return table[next() % (sizeof table / sizeof table[0])];
}

int main() {
    long cases = 0;
    // ---- the modular helpers
    for (int64_t cap = 1; cap <= 12; ++cap)
        for (int64_t a = 0; a < 3 * cap; ++a)
            for (int64_t b = 0; b < 3 * cap; ++b) {
                int64_t want = (a - b) % cap;
                if (want < 0) want += cap;
                if (cancel_mod_diff(a, b, cap) != want) return printf("mod_diff %lld %lld %lld\n", (long long)a, (long long)b, (long long)cap), 1;
                for (int64_t W = 1; W <= cap; ++W) {
                    bool share = false;
                    for (int64_t i = 0; i < W && !share; ++i)
                        for (int64_t j = 0; j < W; ++j)
                            if ((a + i) % cap == (b + j) % cap) share = true;
                    if (cancel_windows_overlap(a % cap, b % cap, W, cap) != share)
                        return printf("overlap %lld %lld %lld %lld\n", (long long)a, (long long)b, (long long)W, (long long)cap), 1;
                    ++cases;
                }
            }
    {
        const int64_t big = (int64_t)1 << 62, cap = ((int64_t)1 << 33) + 8;
        if (cancel_mod_diff(big, big - 5, cap) != 5 || cancel_mod_diff(big - 5, big, cap) != cap - 5) return printf("mod_diff near 2^62\n"), 1;
    }
    // ---- hostile lists
    const int32_t code_len[4] = {1023, 0, 31, 4092};
    CancelPlan plan;
    long accepted = 0;
    for (int round = 0; round < 200000; ++round) {
        const int n_ch = 1 + (int)(next() % 3), n_ep = 1 + (int)(next() % 5);
        const int64_t cap = 8 * (1 + (int64_t)(next() % 64)), W = 1 + (int64_t)(next() % (uint64_t)cap);
        const int64_t w0 = (next() % 4 == 0) ? (int64_t)(next() % ((uint64_t)1 << 62)) : (int64_t)(next() % (uint64_t)(2 * cap));
        std::vector<sdr_epl_item> items((size_t)n_ch * n_ep);
        std::vector<double> amps(items.size() * 2);
        const bool tidy = round % 2 == 0;   // built to be valid, then (sometimes) spoilt in one place
        for (int ch = 0; ch < n_ch; ++ch) {
            int64_t off = 0;
            for (int k = 0; k < n_ep; ++k) {
                sdr_epl_item& it = items[(size_t)ch * n_ep + k];
                double* a = &amps[2 * ((size_t)ch * n_ep + k)];
                if (tidy) {
                    off += (int64_t)(next() % 3);
                    const int64_t room = W - off;
                    const int64_t n = room > 0 ? (int64_t)(next() % (uint64_t)(room + 1)) % 40 : 0;
                    it = sdr_epl_item{(int32_t)(next() % 2 ? 0 : 2), (int32_t)n, w0 + off, 1500.0, 0.5, 0.25, 0.25575};
                    if (w0 + off < 0) it.n_samples = 0;
                    off += n;
                    a[0] = 1.618, a[1] = -0.5;
                } else {
                    it.code_slot = (int32_t)(next() % 7) - 1;
                    it.n_samples = next() % 8 == 0 ? (int32_t)(next() % 0xffffffffu) : (int32_t)(next() % 50) - 2;
                    it.start_sample = next() % 8 == 0 ? (int64_t)next() - ((int64_t)1 << 40) : w0 + (int64_t)(next() % (uint64_t)(W + 4)) - 2;
                    it.carrier_hz = next() % 3 ? 1500.0 : hostile_double();
                    it.rem_carrier = next() % 3 ? 0.5 : hostile_double();
                    it.rem_code = next() % 3 ? 0.25 : hostile_double();
                    it.code_step = next() % 3 ? 0.25575 : hostile_double();
                    a[0] = next() % 4 ? 1.618 : hostile_double(), a[1] = next() % 4 ? -0.5 : hostile_double();
                }
            }
        }
        const int rc = cancel_plan(items.data(), amps.data(), n_ch, n_ep, w0, W, cap, 4, code_len, &plan);
        ++cases;
        if (tidy && rc != CANCEL_OK) return printf("a valid list was refused (%d): %s\n", rc, plan.text), 1;
        if (rc != CANCEL_OK) {
            if (!plan.text[0]) return printf("refused without a text\n"), 1;
            continue;
        }
        ++accepted;
        for (int ch = 0; ch < n_ch; ++ch) {
            int64_t end = 0;
            int used = 0;
            for (int k = 0; k < n_ep; ++k) {
                const sdr_epl_item& it = items[(size_t)ch * n_ep + k];
                if (it.n_samples == 0) continue;
                const CancelItemDev& d = plan.items[(size_t)ch * n_ep + used++];
                int64_t off = (it.start_sample % cap - w0 % cap) % cap;
                if (off < 0) off += cap;
                if (d.off != off || d.n != it.n_samples || d.slot != it.code_slot || d.L != code_len[it.code_slot] || d.L <= 0 || d.n < 0 ||
                    d.off < end || d.off + d.n > W || !(d.step >= 0.0) || !std::isfinite(d.w) || !std::isfinite(d.a_re) || !std::isfinite(d.a_im))
                    return printf("accepted item wrong: round %d ch %d k %d: off %lld (%lld) n %d end %lld W %lld step %a w %a\n", round, ch, k,
                                  (long long)d.off, (long long)off, d.n, (long long)end, (long long)W, d.step, d.w), 1;
                const double last = std::ceil((double)(d.n - 1) * d.step + d.shift);
                if (!(last <= 1073741824.0) || !(std::ceil(d.shift) >= -1073741824.0)) return printf("chip index out of range: round %d\n", round), 1;
                end = d.off + d.n;
            }
            if (used != plan.count[(size_t)ch]) return printf("count: round %d ch %d\n", round, ch), 1;
        }
    }
    if (accepted < 50000) return printf("only %ld lists accepted\n", accepted), 1;
    printf("ok %ld\n", cases);
    return 0;
}
