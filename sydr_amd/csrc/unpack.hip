// Packed 1-, 2- and 4-bit I,Q recordings: carried packed over the host link, widened into the ci8 ring on the device
// (sdr_iq_upload_packed / _begin / _queue).  Nothing downstream of the ring knows: after a packed upload the ring holds, byte
// for byte, what the host's unpack followed by sdr_iq_upload would have left there.
#include "engine_internal.h"
#include "unpack_lanes.h"

#include <cstring>

using namespace sdr;

// The granule path: destination on a 16-byte granule and whole granules long (every slab a receiver feeds: ring sizes and
// milliseconds are multiples of 8 samples).  A lane turns the 2 / 4 / 8 packed bytes of a granule into its 16 ring bytes
// (unpack_lanes.h) and stores them with one dwordx4; `first` = the destination's first granule, taken modulo the ring.
template <int BITS>
__global__ __launch_bounds__(256) void unpack_kernel(const void* __restrict__ src, uint4* __restrict__ ring, size_t n16, size_t first,
                                                     size_t ring16, UnpackTable tab, int msb) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        uint64_t packed;
        if (BITS == 1) packed = ((const uint16_t*)src)[i];
        else if (BITS == 2) packed = ((const uint32_t*)src)[i];
        else packed = ((const uint64_t*)src)[i];
        uint32_t o[4];
        unpack_granule<BITS>(packed, tab, msb != 0, o);
        size_t d = first + i;
        if (d >= ring16) d -= ring16;
        ring[d] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// Any other destination (odd offsets, lengths that are not whole granules): sample by sample, two bytes per store -- exactly
// right, not fast.
__global__ __launch_bounds__(256) void unpack_plain_kernel(const uint8_t* __restrict__ src, uint16_t* __restrict__ ring, int64_t n, int64_t off,
                                                           int64_t cap, UnpackTable tab, int bits, int msb) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        int64_t d = off + k;
        if (d >= cap) d -= cap;
        ring[d] = (uint16_t)unpack_sample(src, k, bits, msb != 0, tab);
    }
}

static int64_t packed_bytes_of(const sdr_iq_packing* pk, int64_t n_samples) {
    if (!pk) return sdr_fail(SDR_ERR_INVALID, "packing is NULL");
    if (pk->bits != 1 && pk->bits != 2 && pk->bits != 4) return sdr_fail(SDR_ERR_INVALID, "packing of %d bits per component (1, 2 or 4)", pk->bits);
    if (pk->flags & ~SDR_PACK_MSB_FIRST) return sdr_fail(SDR_ERR_INVALID, "unknown packing flags 0x%x", pk->flags);
    const int spb = 4 / pk->bits;
    if (n_samples < 0 || n_samples % spb) return sdr_fail(SDR_ERR_INVALID, "%lld samples: a packed slab holds a multiple of %d", (long long)n_samples, spb);
    return n_samples / spb;
}

enum PackedRoute { PACKED_SYNC, PACKED_BEGIN, PACKED_QUEUE };

static int upload_packed(sdr_engine* e, const sdr_iq_packing* pk, const void* packed, int64_t n, int64_t off, PackedRoute route) {
    if (!e) return sdr_fail(SDR_ERR_INVALID, "null engine");
    // (like any call but the tick's own: a resident tick server leaves, a slab parked for the next tick goes into the ring first --
    // before any argument is looked at, as in iq_copy: a call that is refused has still sent a resident server away)
    if (int rc = sdr_set_device(e)) return rc;
    if (!e->iq) return sdr_fail(SDR_ERR_STATE, "IQ ring not allocated");
    if (n < 0) return sdr_fail(SDR_ERR_RANGE, "negative sample count");
    const int64_t nbytes = packed_bytes_of(pk, n);
    if (nbytes < 0) return (int)nbytes;
    if (!packed && n > 0) return sdr_fail(SDR_ERR_INVALID, "host pointer is NULL");
    if (e->iq_fmt != SDR_FMT_CI8) return sdr_fail(SDR_ERR_UNSUPPORTED, "packed recordings are widened into a ci8 ring; this ring has format %d", e->iq_fmt);
    const int64_t cap = e->iq_capacity;
    if (n > cap) return sdr_fail(SDR_ERR_RANGE, "n_samples %lld exceeds ring capacity %lld", (long long)n, (long long)cap);
    if (off < 0) return sdr_fail(SDR_ERR_RANGE, "negative ring offset");
    if (n == 0) return SDR_OK;
    off %= cap;
    const size_t bytes = (size_t)nbytes;
    const int bits = pk->bits, msb = pk->flags & SDR_PACK_MSB_FIRST;
    const UnpackTable tab = unpack_table(pk->levels, bits);
    const bool granules = off % 8 == 0 && n % 8 == 0;
    ProfScope whole(e, "call_upload_packed");
    sdr_iq_mark_written(e, off, n);

    const void* src = nullptr;
    int half = -1;
    const bool slab = route == PACKED_BEGIN && bytes <= (1u << 20);
    if (slab) {
        // a receiver tick's slab: the kernel pulls it over the link out of page-locked memory, as the ingest kernel does --
        // the caller's own block (sdr_host_alloc, 16-byte aligned, whole granules) in place, anything else out of a staging half
        // ("ingest_by_copy_command": no kernel reads host memory -- the staging half goes into HBM by a copy command first)
        bool ours = false;
        if (granules && (uintptr_t)packed % 16 == 0 && !e->ingest_by_copy)
            for (const auto& blk : e->host_blocks)
                ours = ours || ((const char*)packed >= blk.first && (const char*)packed + bytes <= blk.first + blk.second);
        if (ours) {
            src = packed;
        } else {
            char* stage = nullptr;
            if (int rc = sdr_slab_half_acquire(e, bytes, &half, &stage)) return rc;
            memcpy(stage, packed, bytes);
            src = stage;
            if (e->ingest_by_copy) {
                if (int rc = sdr_devbuf_reserve(e, &e->unpack_stage, bytes)) return rc;
                SDR_HIP(hipMemcpyAsync(e->unpack_stage.ptr, stage, bytes, hipMemcpyHostToDevice, e->stream));
                src = e->unpack_stage.ptr;
            }
        }
    } else {
        // a kernel cannot read pageable memory: a copy command brings the packed bytes into HBM (the link transfer is the copy
        // engine's, beside whatever other streams compute), the kernel behind it on the same stream widens them
        if (int rc = sdr_devbuf_reserve(e, &e->unpack_stage, bytes)) return rc;
        SDR_HIP(hipMemcpyAsync(e->unpack_stage.ptr, packed, bytes, hipMemcpyHostToDevice, e->stream));
        src = e->unpack_stage.ptr;
    }
    {
        ProfScope ps(e, "unpack_kernel");
        if (granules && (uintptr_t)src % 8 == 0) {
            const size_t n16 = (size_t)n / 8, first = (size_t)off / 8, ring16 = (size_t)cap / 8;
            const unsigned blocks = (unsigned)((n16 + 255) / 256 < 2048 ? (n16 + 255) / 256 : 2048);
            if (bits == 1) hipLaunchKernelGGL(unpack_kernel<1>, dim3(blocks), dim3(256), 0, e->stream, src, (uint4*)e->iq, n16, first, ring16, tab, msb);
            else if (bits == 2) hipLaunchKernelGGL(unpack_kernel<2>, dim3(blocks), dim3(256), 0, e->stream, src, (uint4*)e->iq, n16, first, ring16, tab, msb);
            else hipLaunchKernelGGL(unpack_kernel<4>, dim3(blocks), dim3(256), 0, e->stream, src, (uint4*)e->iq, n16, first, ring16, tab, msb);
        } else {
            const unsigned blocks = (unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
            hipLaunchKernelGGL(unpack_plain_kernel, dim3(blocks), dim3(256), 0, e->stream, (const uint8_t*)src, (uint16_t*)e->iq, n, off, cap, tab,
                               bits, msb);
        }
    }
    SDR_HIP(hipGetLastError());
    if (slab && half >= 0) {
        SDR_HIP(hipEventRecord(e->slab_done[half], e->stream));
        e->slab_busy[half] = true;
    } else if (slab) {
        e->inplace_slab_in_flight = true;      // (sdr_bank_tick_mirrored_end waits for it where nothing else would)
    }
    // synchronous call; a `_begin` slab too long for the staging halves is copied before return by waiting for it, as
    // sdr_iq_upload_begin does
    if (route == PACKED_SYNC || (route == PACKED_BEGIN && !slab)) SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

extern "C" {

int64_t sdr_iq_packed_bytes(const sdr_iq_packing* pk, int64_t n_samples) { return packed_bytes_of(pk, n_samples); }

int sdr_iq_upload_packed(sdr_engine* e, const sdr_iq_packing* pk, const void* packed, int64_t n_samples, int64_t ring_offset) {
    return upload_packed(e, pk, packed, n_samples, ring_offset, PACKED_SYNC);
}

int sdr_iq_upload_packed_begin(sdr_engine* e, const sdr_iq_packing* pk, const void* packed, int64_t n_samples, int64_t ring_offset) {
    return upload_packed(e, pk, packed, n_samples, ring_offset, PACKED_BEGIN);
}

int sdr_iq_upload_packed_queue(sdr_engine* e, const sdr_iq_packing* pk, const void* packed, int64_t n_samples, int64_t ring_offset) {
    return upload_packed(e, pk, packed, n_samples, ring_offset, PACKED_QUEUE);
}

}  // extern "C"
