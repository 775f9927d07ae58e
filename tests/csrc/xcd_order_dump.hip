// Host build of the E/P/L kernels' workgroup order (sydr_amd/csrc/xcd_order.h): for the run length R of argv[1] and every
// launch size n = 0 .. argv[2], xcd_order(b, n, R) of b = 0 .. n - 1 as raw uint32 on stdout, launch after launch.
// Test infrastructure (tests/test_xcd_order_map.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sydr_amd/csrc/xcd_order.h"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const unsigned R = (unsigned)strtoul(argv[1], nullptr, 10), n_max = (unsigned)strtoul(argv[2], nullptr, 10);
    std::vector<uint32_t> row;
    for (unsigned n = 0; n <= n_max; ++n) {
        row.resize(n);
        for (unsigned b = 0; b < n; ++b) row[b] = sdr::xcd_order(b, n, R);
        if (n && fwrite(row.data(), sizeof(uint32_t), n, stdout) != n) return 1;
    }
    return 0;
}
