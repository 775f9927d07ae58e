// Which item of a launch a workgroup takes, so that neighbouring items run on ONE XCD.  The hardware deals the workgroups
// of a launch to the chip's XCDs round-robin by linear id (docs/notes/K2-K6.md: blockIdx % 8 is the XCD), each XCD with an L2
// of its own: in linear order the channels of one millisecond of an epoch-major list land on every XCD, and every L2 fetches
// the whole stream for itself.  Here the ids are taken in tiles of kXcds * R: inside a tile XCD x = b % kXcds walks the R
// consecutive items  t * T + x * R .. + R - 1  in ascending order.  A permutation of [0, n): nothing but the placement changes.
// Host and device (tests/test_xcd_order_map.py builds it for the host).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SDR_XCD_HD __host__ __device__
#else
#define SDR_XCD_HD
#endif

namespace sdr {

constexpr int kXcds = 8;   // XCDs of the device: the `& 7` / `>> 3` of the PCPS workgroup mappings (pcps_fft.h, pcps_fast.h, pcps_fused.h)

// b: linear workgroup id, n: workgroups of the launch, R: run length (0: linear order).  The partial last tile keeps the
// linear order.  One division by a run-time value, the rest shifts and selects -- no branch: in a kernel the loads of its
// other arguments need not wait behind one.
SDR_XCD_HD inline unsigned xcd_order(unsigned b, unsigned n, unsigned R) {
    const unsigned T = R ? kXcds * R : 1u;
    const unsigned first = (b / T) * T, r = b - first;
    // (b's tile is a whole one: b < (n / T) * T; first <= b < n: no wrap)
    const unsigned whole = (unsigned)(R != 0) & (unsigned)(n - first >= T);
    const unsigned moved = (r % kXcds) * R + r / kXcds;     // its place in the tile
    return b + ((moved - r) & (0u - whole));
}

}  // namespace sdr
