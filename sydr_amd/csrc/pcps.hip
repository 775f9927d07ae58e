// K2-K6: Parallel Code Phase Search on device (sydr/dsp/acquisition.py:9-115).
//
//   for every Doppler bin b:   F_b = FFT_N( x[n] * exp(-1j*(IF - bin_b)*((2n)*pi/fs)) )      (PRN independent,
//                                                                                             computed ONCE, not per PRN)
//   for every (PRN p, bin b):  map[p][b][:] += | IFFT_N( F_b * conj(FFT_N(upsampled code_p)) ) |
//   per PRN: first global argmax (row-major) + second peak in the winning row.
//
// N = samples per code = 4000 / 10000 / 25000 / 50000 are not powers of two, so
// the transform is a hand-written mixed-radix (2,3,4,5,8 + small primes)
// Stockham autosort FFT in fp64, batched over (PRN, bin); each pass streams the
// batch through HBM/L2 with 16-byte complex loads.  The Doppler mix and the
// int8->fp64 conversion are fused into the first forward pass, the code-spectrum
// multiply into the first inverse pass, and 1/N scale + magnitude + (non-)coherent
// accumulation into the last inverse pass.  fp64 throughout: the peak INDEX must
// match NumPy's bit for bit, and a 1e-7 relative error could reorder near-ties.
//
// This file: the code spectra, the forward transforms, the four routes of a search (pcps_plan.h chooses), the deep search's
// driver and the entry points (sdr_pcps_signal: the same search by chip rate and code period, circular or zero-padded over two
// periods -- pcps_impl; sdr_pcps_coherent: that search's transforms with the complex results kept, run_coherent).  The transforms are pcps_fft.h's, the peak kernels pcps_peak.h's, what a request means
// acq_request.h's; SerialSearch is serial_search.hip.  docs/notes/pcps_layout.md has the map.
#include "engine_internal.h"
#include <chrono>
#include "acq_deep.h"
#include "acq_request.h"
#include "coherent_request.h"
#include "detect_zone.h"
#include "pcps_coherent.h"
#include "pcps_fft.h"
#include "pcps_fast.h"
#include "pcps_fastn.h"
#include "pcps_peak.h"
#include "pcps_plan.h"

#include <cmath>
#include <cstring>
#include <vector>

#pragma clang fp contract(off)

namespace {

using namespace pcps;

// The two operand images of a PRN's code spectrum for the fused search at N = 2 M = 50 000 (pcps_fused.h): parity 0 is the
// spectrum itself, parity 1 carries the twiddle of the odd half of the radix-2 decimation-in-frequency step,
//     C1[k] = C[k] w^-k,  C1[k + M] = -C[k + M] w^-k,  w = exp(-2 pi i / N)   (tw[k] = w^k: multiplied conjugated).
__global__ __launch_bounds__(kThreads) void code_parity_kernel(const double2* __restrict__ C, const double2* __restrict__ tw, int N,
                                                               double2* __restrict__ out) {
    const int k = blockIdx.x * kThreads + threadIdx.x, prn = blockIdx.y;
    if (k >= N) return;
    const int M = N / 2;
    const double2 c = C[(size_t)prn * N + k];
    const double2 w = tw[k < M ? k : k - M];
    double2 o = make_double2(__builtin_fma(c.y, w.y, c.x * w.x), __builtin_fma(-c.x, w.y, c.y * w.x));    // c * conj(w)
    if (k >= M) o = make_double2(-o.x, -o.y);
    out[((size_t)prn * 2) * N + k] = c;
    out[((size_t)prn * 2 + 1) * N + k] = o;
}

// The replica of one code period, N samples at chip period tc, followed by T - N zeros (T == N: none; the zero-padded search
// of sdr_pcps_signal transforms two periods' length).
__global__ __launch_bounds__(kThreads) void upsample_batch_kernel(const int8_t* __restrict__ codes,
                                                                  const int32_t* __restrict__ code_len,
                                                                  int code_stride, const int32_t* __restrict__ slots,
                                                                  double ts, double tc, int N, int T,
                                                                  int8_t* __restrict__ out) {
    int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= T) return;
    int8_t chip = 0;
    if (k < N) {
        const int slot = slots[blockIdx.y];
        const int L = code_len[slot];
        double v = (ts * (double)k) / tc;  // gnsssignal.py:53
        int idx = (int)trunc(v);
        if (idx >= L) idx = L - 1;
        chip = codes[(size_t)slot * code_stride + idx];
    }
    out[(size_t)blockIdx.y * T + k] = chip;
}

// map += |csum| (acquisition.py:68)
__global__ __launch_bounds__(kThreads) void mag_acc_kernel(const double2* __restrict__ csum, double* __restrict__ map,
                                                           size_t count, int first_block) {
    size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    double mag = hypot(csum[i].x, csum[i].y);
    map[i] = first_block ? 0.0 + mag : map[i] + mag;
}

// The engine's switches the planner reads.
PcpsSwitches pcps_switches(const sdr_engine* e) {
    PcpsSwitches s;
    s.fused = e->pcps_fused, s.no_fast = e->pcps_no_fast, s.force_map = e->pcps_force_map, s.no_overlap = e->pcps_no_overlap;
    s.no_shared_spectra = e->pcps_no_shared_spectra, s.prn_chunk = e->pcps_prn_chunk, s.prof = e->prof;
    return s;
}

// What one call brings along that the plan does not hold.
struct PcpsCall {
    int64_t start = 0;
    double if_hz = 0.0;
    // the caller's slot numbers (nullptr: it handed in the code spectra), their copy in the page-locked block, their place
    // on the device (copied there only when the spectra have to be made)
    const int32_t *slots = nullptr, *slots_pinned = nullptr;
    int32_t* d_slots = nullptr;
    long long *dev_bin = nullptr, *dev_code = nullptr;      // device copies of the first peaks (read by the second sweep)
    // the page-locked results the peak kernels write (a few hundred bytes: one copy command and its stream latency less per
    // acquisition), and the done words behind them, raised to done_seq
    long long *res_bin = nullptr, *res_code = nullptr;
    double *res_ratio = nullptr, *res_value = nullptr;    // (res_value: the deep search's)
    unsigned* done = nullptr;
    unsigned done_seq = 0;
    const BluPlan* blu = nullptr;
    const long long* spec_off = nullptr;   // shared spectra: every bin's element offset inside its block of P class spectra
};

// The device table of shared-spectra offsets (kept while the shape stays).
int upload_spec_offsets(sdr_engine* e, const PcpsPlan& p, const long long** off_out) {
    const SharedSpectra& s = p.sh;
    *off_out = nullptr;
    if (!s.P) return SDR_OK;
    std::vector<int64_t> key = {(int64_t)p.N, (int64_t)p.nbins, (int64_t)s.P, (int64_t)s.q};
    if (key != e->pcps_spec_off_key) {
        std::vector<long long> off((size_t)p.nbins);
        for (int b = 0; b < p.nbins; ++b)
            off[(size_t)b] = (long long)(b % s.P) * (s.H + p.N) + s.H - (long long)(b / s.P) * s.q;
        e->pcps_spec_off_key.clear();
        if (int rc = sdr_devbuf_reserve(e, &e->pcps_spec_off, off.size() * sizeof(long long))) return rc;
        SDR_HIP(hipMemcpyAsync(e->pcps_spec_off.ptr, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, e->stream));
        SDR_HIP(hipStreamSynchronize(e->stream));      // (pageable source: complete before `off` goes)
        e->pcps_spec_off_key = key;
    }
    *off_out = (const long long*)e->pcps_spec_off.ptr;
    return SDR_OK;
}

// K7/a3: upsample every code and take conj(fft(code)) (channel_l1ca_kaplan.py:184-185), unless the caller handed in its own
// codeFFT arrays (function-level drop-in of PCPS()) -- or the spectra of exactly these staged codes at this rate are still in
// the buffer from the previous search (the reference recomputes them on every acquisition, kaplan:184-185; they only change
// when a slot is re-staged).
template <int FMT>
int code_spectra(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c) {
    const int N = p.N, n_prn = p.n_prn;
    std::vector<int64_t> key;
    if (c.slots) {
        // (the transform length, the samples per code inside it, both rates: a circular and a zero-padded search of the same
        // slots, or two chip rates of one code, never share spectra)
        int64_t fs_bits, chip_bits;
        memcpy(&fs_bits, &p.fs, sizeof(fs_bits));
        memcpy(&chip_bits, &p.chip_rate, sizeof(chip_bits));
        key = {(int64_t)N, (int64_t)p.cols, fs_bits, chip_bits, e->code_generation};
        for (int i = 0; i < n_prn; ++i) {
            key.push_back(c.slots[i]);
            key.push_back(e->code_stamp[c.slots[i]]);
        }
    }
    const bool spectra_cached = c.slots && key == e->pcps_spec_key && !e->pcps_no_spec_cache;
    if (!spectra_cached) {
        e->pcps_code2_ok = false;
        e->pcps_spec_key.clear();   // (valid again only once the new spectra are queued without error, below)
    }
    if (!c.slots || spectra_cached) return SDR_OK;
    int8_t* up = (int8_t*)e->pcps_b.ptr;  // scratch: n_prn*N bytes fits easily in a work buffer
    // (the slot numbers reach the device only now: a search whose spectra are still there needs no copy command in
    // front of its first kernel -- 2.7 us of copy and two boundaries on the stream)
    SDR_HIP(hipMemcpyAsync(c.d_slots, c.slots_pinned, (size_t)n_prn * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    {
        ProfScope ps(e, "pcps_upsample");
        hipLaunchKernelGGL(upsample_batch_kernel, dim3((N + kThreads - 1) / kThreads, n_prn), dim3(kThreads), 0,
                           e->stream, e->codes, e->code_len, e->code_stride, c.d_slots, 1.0 / p.fs, 1.0 / p.chip_rate, p.cols, N, up);
    }
    PassArgs a = {};
    a.tw = (const double2*)e->pcps_tw.ptr;
    a.N = N;
    a.code_samples = up;
    // ping-pong inside A (two halves are not needed: code batch is small) -> use A and F as scratch
    run_fft<false, LOAD_CODE_REAL, STORE_CONJ, FMT>(e, p.xf, a, n_prn, (double2*)e->pcps_a.ptr, (double2*)e->pcps_fwd.ptr,
                                                    (double2*)e->pcps_code.ptr, "pcps_code_fft", c.blu);
    SDR_HIP(hipGetLastError());
    e->pcps_spec_key = key;
    return SDR_OK;
}

// Forward transforms of the Doppler-mixed millisecond number `block` (coherent index ic), `batch` bins (or classes of
// shared spectra, written with their halos: F holds P rows of H + N) at once.  A block starts p.cols samples behind the one
// before it and is p.N samples long: the zero-padded search's blocks overlap by one code period.
template <int FMT>
void forward(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c, int batch, int64_t block, int ic, int iq_blocks) {
    PassArgs f = {};
    f.tw = (const double2*)e->pcps_tw.ptr;
    f.N = p.N;
    f.ring = e->iq;
    f.capacity = e->iq_capacity;
    f.first_sample = c.start + block * p.cols;
    f.carrier_offset = (int64_t)ic * p.N;
    f.fs = p.fs;
    f.if_hz = c.if_hz;
    f.bin_start = p.bin_start;
    f.bin_delta = p.bin_delta;
    f.iq_blocks = iq_blocks;
    f.halo = p.sh.H;
    run_fft<false, LOAD_IQ_MIX, STORE_PLAIN, FMT>(e, p.xf, f, batch, (double2*)e->pcps_a.ptr, (double2*)e->pcps_b.ptr,
                                                  (double2*)e->pcps_fwd.ptr, "pcps_fwd_fft", c.blu);
}

// The operands of an inverse sweep over the PRNs from p0 on, every bin.
PassArgs sweep_args(const sdr_engine* e, const PcpsPlan& p, int p0) {
    PassArgs g = {};
    g.tw = (const double2*)e->pcps_tw.ptr;
    g.N = p.N;
    g.in = (const double2*)e->pcps_fwd.ptr;
    g.code_spec = (const double2*)e->pcps_code.ptr + (size_t)p0 * p.N;
    g.nbins = p.nbins;
    g.scale = 1.0 / (double)p.N;
    g.map = (double*)e->pcps_map.ptr + (size_t)p0 * p.nbins * p.cols;
    g.cols = p.cols;
    g.csum = e->pcps_csum.ptr ? (double2*)e->pcps_csum.ptr + (size_t)p0 * p.nbins * p.N : nullptr;
    return g;
}

// N = 10 000, indices and ratio only, one coherent millisecond per block: the forward transforms of every block first, then
// ONE launch that keeps each (PRN, bin)'s transform in LDS and its non-coherent sum in registers and finds both peaks
// (pcps_fused10k.h) -- no map, no intermediate, no second sweep
template <int FMT>
int run_fused10k(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c) {
    // (the carrier restarts with every block; all blocks in one batch: [block][bin])
    const int per_block = p.sh.P ? p.sh.P : p.nbins;
    forward<FMT>(e, p, c, per_block * p.noncoh, 0, 0, per_block);
    const long long blk_stride = p.sh.P ? (long long)p.sh.P * (p.sh.H + p.N) : (long long)p.nbins * p.N;
    return sdr_pcps_fused10k_search(e, e->pcps_fwd.ptr, c.spec_off, blk_stride, e->pcps_code.ptr, e->pcps_tw.ptr, p.n_prn, p.nbins,
                                    p.noncoh, p.N, p.spc, e->pcps_part.ptr, c.res_bin, c.res_code, c.res_ratio, c.done, c.done_seq);
}

// Every (PRN, bin) transform of the search in ONE launch of persistent workgroups (no intermediate, no sweeps), then the first
// peaks, the second sweep and the ratio of the two in one more: the whole K6 (pcps_fused.h ifft_second_kernel).
template <int FMT>
int run_fused(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c) {
    const int N = p.N, n_prn = p.n_prn;
    forward<FMT>(e, p, c, p.sh.P ? p.sh.P : p.nbins, 0, 0, 0);
    const double2* C = (const double2*)e->pcps_code.ptr;
    const double2* tw = (const double2*)e->pcps_tw.ptr;
    if (p.terms == 2) {                    // N = 50 000: the spectra and their parity images
        if (!e->pcps_code2_ok) {           // (made with the spectra, kept as long as they are)
            ProfScope ps(e, "pcps_code_fft");
            hipLaunchKernelGGL(code_parity_kernel, dim3((N + kThreads - 1) / kThreads, n_prn), dim3(kThreads), 0, e->stream, C,
                               tw, N, (double2*)e->pcps_code2.ptr);
            e->pcps_code2_ok = true;
        }
        C = (const double2*)e->pcps_code2.ptr;
    }
    Best* parts = (Best*)e->pcps_part.ptr;
    if (int rc = sdr_pcps_fused_sweep(e, e->pcps_fwd.ptr, c.spec_off, C, tw, n_prn, p.nbins, N, parts)) return rc;
    Best* tops = parts + (size_t)n_prn * p.records_per_prn;
    return sdr_pcps_fused_second(e, e->pcps_fwd.ptr, c.spec_off, C, tw, n_prn, N, p.spc, parts, p.records_per_prn, tops,
                                 c.dev_bin, c.dev_code, tops + n_prn, c.res_bin, c.res_code, c.res_ratio, c.done, c.done_seq);
}

// Map-free inverse sweeps that leave per-wave records; then the maximum from the records and the winning row of every PRN
// alone (1/nbins of one inverse sweep) for the second peak.
template <int FMT>
int run_sweeps(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c) {
    const int n_prn = p.n_prn, nbins = p.nbins;
    double2* A = (double2*)e->pcps_a.ptr;
    double2* B = (double2*)e->pcps_b.ptr;
    Best* parts = (Best*)e->pcps_part.ptr;
    forward<FMT>(e, p, c, nbins, 0, 0, 0);
    // Register-resident kernels, several sweeps, nobody timing the stages: the sweeps alternate between two
    // streams and two intermediates, so that one sweep's partial last rounds of workgroups (and its launch
    // ramps) are filled by the other's -- ordered behind the forward transforms and in front of the peak
    // kernels by two events.
    if (p.overlap) {
        if (!e->pcps_aux) {
            SDR_HIP(hipStreamCreateWithFlags(&e->pcps_aux, hipStreamNonBlocking));
            SDR_HIP(hipEventCreateWithFlags(&e->pcps_ev[0], hipEventDisableTiming));
            SDR_HIP(hipEventCreateWithFlags(&e->pcps_ev[1], hipEventDisableTiming));
        }
        SDR_HIP(hipEventRecord(e->pcps_ev[0], e->stream));
        SDR_HIP(hipStreamWaitEvent(e->pcps_aux, e->pcps_ev[0], 0));
    }
    int sweep = 0;
    for (int p0 = 0; p0 < n_prn; p0 += p.prn_chunk, ++sweep) {
        const int pc = std::min(n_prn - p0, p.prn_chunk);
        PassArgs g = sweep_args(e, p, p0);
        g.partials = parts + (size_t)p0 * nbins * p.records_sweep;
        if (p.overlap)
            fast_run(e, p.xf, g, pc * nbins, (sweep & 1) ? B : A, (sweep & 1) ? e->pcps_aux : e->stream);
        else
            run_fft<true, LOAD_MUL_CODE, STORE_MAG_MAX, FMT>(e, p.xf, g, pc * nbins, A, B, nullptr, "pcps_inv_fft", c.blu);
    }
    if (p.overlap) {
        SDR_HIP(hipEventRecord(e->pcps_ev[1], e->pcps_aux));
        SDR_HIP(hipStreamWaitEvent(e->stream, e->pcps_ev[1], 0));
    }
    Best* tops = parts + (size_t)n_prn * p.records_per_prn;
    Best* seconds = tops + n_prn;      // [n_prn][records of the second sweep]
    long long *dev_bin = c.dev_bin, *dev_code = c.dev_code;
    {
        ProfScope ps(e, "pcps_peak");
        hipLaunchKernelGGL(argmax_records_kernel, dim3(n_prn), dim3(kThreads), 0, e->stream, parts, p.records_per_prn, p.N, tops,
                           dev_bin, dev_code);
    }
    PassArgs g = sweep_args(e, p, 0);
    g.sel_bin = dev_bin;
    g.tops = tops;
    g.spc = p.spc;
    g.partials = seconds;
    run_fft<true, LOAD_MUL_CODE_SEL, STORE_MAG_MAX, FMT>(e, p.xf, g, n_prn, A, B, nullptr, "pcps_inv_fft", c.blu);
    {
        ProfScope ps(e, "pcps_peak");
        hipLaunchKernelGGL(ratio_kernel, dim3(n_prn), dim3(64), 0, e->stream, seconds, p.records_second,
                           tops, dev_bin, dev_code, c.res_bin, c.res_code, c.res_ratio);
    }
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

// The map: |.| of every (PRN, bin) transform accumulated over the non-coherent blocks (the complex values over the coherent
// ones first), then its peaks.
template <int FMT>
int run_map(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c) {
    const int n_prn = p.n_prn, nbins = p.nbins, N = p.cols;      // (the map's columns)
    double2* A = (double2*)e->pcps_a.ptr;
    double2* B = (double2*)e->pcps_b.ptr;
    double* map = (double*)e->pcps_map.ptr;
    for (int inc = 0; inc < p.noncoh; ++inc) {
        for (int ic = 0; ic < p.coh; ++ic) {
            forward<FMT>(e, p, c, nbins, (int64_t)inc * p.coh + ic, ic, 0);
            for (int p0 = 0; p0 < n_prn; p0 += p.prn_chunk) {
                const int pc = std::min(n_prn - p0, p.prn_chunk);
                PassArgs g = sweep_args(e, p, p0);
                if (p.cols != p.N) {       // (zero-padded: coh == 1; the inverse pass reads no ring sample, one format serves)
                    g.first_block = inc == 0;
                    run_fft<true, LOAD_MUL_CODE, STORE_MAG_KEEP, SDR_FMT_CF64>(e, p.xf, g, pc * nbins, A, B, nullptr, "pcps_inv_fft", c.blu);
                } else if (p.coh == 1) {
                    g.first_block = inc == 0;
                    run_fft<true, LOAD_MUL_CODE, STORE_MAG_ACC, FMT>(e, p.xf, g, pc * nbins, A, B, nullptr, "pcps_inv_fft", c.blu);
                } else {
                    g.first_block = ic == 0;
                    run_fft<true, LOAD_MUL_CODE, STORE_CPLX_ACC, FMT>(e, p.xf, g, pc * nbins, A, B, nullptr, "pcps_inv_fft", c.blu);
                }
            }
        }
        if (p.coh > 1) {
            ProfScope ps(e, "pcps_mag_acc");
            size_t count = (size_t)n_prn * nbins * N;
            hipLaunchKernelGGL(mag_acc_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                               e->stream, (const double2*)e->pcps_csum.ptr, map, count, inc == 0 ? 1 : 0);
        }
    }
    // K6
    {
        ProfScope ps(e, "pcps_peak");
        Best* parts = (Best*)e->pcps_part.ptr;
        hipLaunchKernelGGL(argmax_part_kernel, dim3(kPeakParts, n_prn), dim3(kThreads), 0, e->stream, map,
                           (long long)nbins * N, parts);
        hipLaunchKernelGGL(peak_finish_kernel, dim3(n_prn), dim3(kThreads), 0, e->stream, map, nbins, N, p.spc, parts,
                           c.res_bin, c.res_code, c.res_ratio);
    }
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

// ---- the deep search (sdr_acq_deep): coherent blocks folded in front of ONE forward transform per (bin, block), the blocks'
// magnitudes added into their bit-edge group's map at the code-Doppler shift of (bin, block).  The transforms, the code spectra
// and the peak kernels are the map route's (run_map with coh = 1: the same instantiations); the fold and the shifted
// accumulation are acq_deep.hip's.  The shifted accumulation is a kernel of its own behind the inverse sweep's magnitude store
// (STORE_MAG_ACC into a scratch row per transform), not a store mode of the sweep's last pass: that costs one more read and
// write of pc * nbins * N doubles per block and sweep -- a sixth of what the sweep itself moves through HBM (its column kernel
// writes and its row kernel reads 16 N bytes per transform, the operands come on top) -- and leaves every existing kernel,
// the register-resident ones included, as it is; their stores go out in 64-byte runs of one map row, which a per-row offset
// would break at the wrap.
struct DeepCall {
    int64_t start = 0;
    double if_hz = 0.0;
    int coh = 1, noncoh = 1, groups = 1;
    const int32_t* q = nullptr;      // device: [noncoh][nbins] shifts, each in [0, N)
    double2* fold = nullptr;         // [nbins][N]
    double* mag = nullptr;           // [prn_chunk][nbins][N]
};

__global__ __launch_bounds__(64) void deep_peak_value_kernel(const double* __restrict__ map, long long per_prn, int N, int n_prn,
                                                             const long long* __restrict__ row, const long long* __restrict__ code,
                                                             double* __restrict__ value) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p < n_prn) value[p] = map[(size_t)p * per_prn + (size_t)row[p] * N + code[p]];
}

int run_deep(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c, const DeepCall& d) {
    const int n_prn = p.n_prn, nbins = p.nbins, N = p.N, G = d.groups;
    double2* A = (double2*)e->pcps_a.ptr;
    double2* B = (double2*)e->pcps_b.ptr;
    double* map = (double*)e->pcps_map.ptr;        // [n_prn][G][nbins][N]
    for (int i = 0; i < d.noncoh; ++i) {
        if (int rc = sdr_deep_fold(e, d.start + (int64_t)i * d.coh * N, N, d.coh, nbins, p.fs, d.if_hz, p.bin_start, p.bin_delta,
                                   d.fold))
            return rc;
        PassArgs f = {};
        f.tw = (const double2*)e->pcps_tw.ptr;
        f.N = N;
        f.in = d.fold;
        run_fft<false, LOAD_PLAIN, STORE_PLAIN, SDR_FMT_CF64>(e, p.xf, f, nbins, A, B, (double2*)e->pcps_fwd.ptr, "deep_fwd_fft", c.blu);
        for (int p0 = 0; p0 < n_prn; p0 += p.prn_chunk) {
            const int pc = std::min(n_prn - p0, p.prn_chunk);
            PassArgs g = sweep_args(e, p, p0);
            g.map = d.mag;
            g.first_block = 1;
            run_fft<true, LOAD_MUL_CODE, STORE_MAG_ACC, SDR_FMT_CF64>(e, p.xf, g, pc * nbins, A, B, nullptr, "deep_inv_fft", c.blu);
            if (int rc = sdr_deep_shift_acc(e, d.mag, map + (size_t)p0 * G * nbins * N, d.q + (size_t)i * nbins, pc, nbins, N, G,
                                            i % G, i < G ? 1 : 0))
                return rc;
        }
    }
    {
        // rows of a PRN: (group, bin), row r = group r / nbins, bin r % nbins; the ratio stays inside the winning row
        ProfScope ps(e, "deep_peak");
        Best* parts = (Best*)e->pcps_part.ptr;
        const long long per_prn = (long long)G * nbins * N;
        hipLaunchKernelGGL(argmax_part_kernel, dim3(kPeakParts, n_prn), dim3(kThreads), 0, e->stream, map, per_prn, parts);
        hipLaunchKernelGGL(peak_finish_kernel, dim3(n_prn), dim3(kThreads), 0, e->stream, map, G * nbins, N, p.spc, parts,
                           c.res_bin, c.res_code, c.res_ratio);
        hipLaunchKernelGGL(deep_peak_value_kernel, dim3((n_prn + 63) / 64), dim3(64), 0, e->stream, map, per_prn, N, n_prn,
                           c.res_bin, c.res_code, c.res_value);
    }
    SDR_HIP(hipGetLastError());
    return SDR_OK;
}

// ---- the coherent search (sdr_pcps_coherent): the zero-padded search's transforms with the complex results kept.  Forward:
// the padded route's, one launch per period, all M periods' spectra side by side ([M][nbins][T], PRN independent, made once
// however the units are cut).  Per chunk of (PRN, bin) units (coherent_request.h coherent_chunk): M inverse sweeps with
// STORE_CPLX_ACC as a plain store (first_block = 1) into the scratch [M][units][T] -- the instantiation of the map route's
// coherent blocks, the code-spectrum product numbered inside the chunk -- then pcps_coherent.hip's combine into the chunk's
// rows of R, the chunk's maxima and the kept column.  Behind the last chunk the map's peaks as run_deep takes them, and the
// pick.  A transform does not depend on the batch it runs in, so no value depends on the cut.
struct CohCall {
    double2* scr = nullptr;      // [M][units of the largest chunk][T]
    int cap = 0;                 // units a chunk may hold
    void *best = nullptr, *keep = nullptr;
    sdr_coh_result* results = nullptr;   // device
    double* power = nullptr;             // device
};

template <int FMT>
int run_coherent(sdr_engine* e, const PcpsPlan& p, const PcpsCall& c, const CohGeom& g, const CohCall& k) {
    const int T = p.N, N = p.cols, nbins = p.nbins, n_prn = p.n_prn, M = g.M;
    if (int rc = code_spectra<FMT>(e, p, c)) return rc;
    double2* A = (double2*)e->pcps_a.ptr;
    double2* B = (double2*)e->pcps_b.ptr;
    double2* F = (double2*)e->pcps_fwd.ptr;
    double* map = (double*)e->pcps_map.ptr;
    Best* parts = (Best*)e->pcps_part.ptr;
    for (int m = 0; m < M; ++m) {
        PassArgs f = {};
        f.tw = (const double2*)e->pcps_tw.ptr;
        f.N = T;
        f.ring = e->iq;
        f.capacity = e->iq_capacity;
        f.first_sample = c.start + (int64_t)m * N;
        f.fs = p.fs;
        f.if_hz = c.if_hz;
        f.bin_start = p.bin_start;
        f.bin_delta = p.bin_delta;
        run_fft<false, LOAD_IQ_MIX, STORE_PLAIN, FMT>(e, p.xf, f, nbins, A, B, F + (size_t)m * nbins * T, "coherent_fwd_fft", c.blu);
    }
    const int chunks = sdr::coherent_chunk_count(k.cap, n_prn, nbins);
    for (int i = 0; i < chunks; ++i) {
        const sdr::CohChunk ch = sdr::coherent_chunk(k.cap, n_prn, nbins, i);
        const int units = ch.units();
        for (int m = 0; m < M; ++m) {
            PassArgs q = {};
            q.tw = (const double2*)e->pcps_tw.ptr;
            q.N = T;
            q.in = F + ((size_t)m * nbins + ch.bin0) * T;
            q.code_spec = (const double2*)e->pcps_code.ptr + (size_t)ch.prn0 * T;
            q.nbins = ch.bins;
            q.scale = 1.0 / (double)T;
            q.cols = N;
            q.csum = k.scr + (size_t)m * units * T;
            q.first_block = 1;
            run_fft<true, LOAD_MUL_CODE, STORE_CPLX_ACC, SDR_FMT_CF64>(e, p.xf, q, units, A, B, nullptr, "coherent_inv_fft", c.blu);
        }
        if (int rc = sdr_coh_combine(e, g, ch, k.scr, map)) return rc;
        {
            ProfScope ps(e, "coherent_peak");
            hipLaunchKernelGGL(argmax_part_kernel, dim3(kPeakParts, ch.prns), dim3(kThreads), 0, e->stream,
                               map + ((size_t)ch.prn0 * nbins + ch.bin0) * N, (long long)ch.bins * N, parts);
            if (int rc = sdr_coh_keep(e, g, ch, k.scr, parts, k.best, k.keep)) return rc;
        }
    }
    {
        ProfScope ps(e, "coherent_peak");
        hipLaunchKernelGGL(argmax_part_kernel, dim3(kPeakParts, n_prn), dim3(kThreads), 0, e->stream, map, (long long)nbins * N, parts);
        hipLaunchKernelGGL(peak_finish_kernel, dim3(n_prn), dim3(kThreads), 0, e->stream, map, nbins, N, p.spc, parts, c.res_bin,
                           c.res_code, c.res_ratio);
    }
    SDR_HIP(hipGetLastError());
    return sdr_coh_pick(e, g, n_prn, k.keep, map, c.res_bin, c.res_code, c.res_ratio, k.results, k.power);
}

// The tables a plan's transforms read, made when the code length changes: the twiddles, and for a chirp-z length the chirp,
// the length-M twiddles and the spectra of both kernels (*blu_out: the chirp-z plan, filled where p.M is set).
int prepare_tables(sdr_engine* e, const PcpsPlan& p, BluPlan* blu_out) {
    const int N = p.N;
    int rc;
    if (e->pcps_tw_n != N) {
        if ((rc = sdr_devbuf_reserve(e, &e->pcps_tw, p.tbytes))) return rc;
        hipLaunchKernelGGL(twiddle_kernel, dim3((N + kThreads - 1) / kThreads), dim3(kThreads), 0, e->stream,
                           (double2*)e->pcps_tw.ptr, N);
        SDR_HIP(hipGetLastError());
        e->pcps_tw_n = N;
    }
    if (p.M) {
        const int M = p.M;
        for (DevBuf* b : {&e->pcps_blu, &e->pcps_blu_x, &e->pcps_blu_a, &e->pcps_blu_b})
            if ((rc = sdr_devbuf_reserve(e, b, b == &e->pcps_blu ? p.blu_bytes : p.blu_work_bytes))) return rc;
        double2* chirp = (double2*)e->pcps_blu.ptr;
        double2* spec_fwd = chirp + N;
        double2* twM = spec_fwd + 2 * M;
        *blu_out = {N, M, chirp, spec_fwd, spec_fwd + M, twM, (double2*)e->pcps_blu_x.ptr, (double2*)e->pcps_blu_a.ptr,
                    (double2*)e->pcps_blu_b.ptr, &p.xm};
        if (e->pcps_blu_n != N) {  // plan cached per code length: chirp, length-M twiddles, spectra of both kernels
            hipLaunchKernelGGL(twiddle_kernel, dim3((M + kThreads - 1) / kThreads), dim3(kThreads), 0, e->stream, twM, M);
            hipLaunchKernelGGL(blu_chirp_kernel, dim3((M + kThreads - 1) / kThreads), dim3(kThreads), 0, e->stream, chirp,
                               blu_out->x, blu_out->x + M, N, M);
            PassArgs a = {};
            a.N = M;
            a.tw = twM;
            a.in = blu_out->x;  // two transforms at once: [kernel_fwd, kernel_inv] -> [spec_fwd, spec_inv] (adjacent)
            run_fft<false, LOAD_PLAIN, STORE_PLAIN, SDR_FMT_CF64>(e, p.xm, a, 2, blu_out->a, blu_out->b, spec_fwd, "pcps_bluestein_plan");
            SDR_HIP(hipGetLastError());
            e->pcps_blu_n = N;
        }
    }
    return SDR_OK;
}

template <int FMT>
int pcps_search(sdr_engine* e, const PcpsPlan& p, PcpsCall& c) {
    if (int rc = code_spectra<FMT>(e, p, c)) return rc;
    if (int rc = upload_spec_offsets(e, p, &c.spec_off)) return rc;
    switch (p.route) {
        case ROUTE_FUSED10K: return run_fused10k<FMT>(e, p, c);
        case ROUTE_FUSED: return run_fused<FMT>(e, p, c);
        case ROUTE_SWEEPS: return run_sweeps<FMT>(e, p, c);
        default: return run_map<FMT>(e, p, c);
    }
}

}  // namespace

extern "C" {

int sdr_pcps_bins(double doppler_range, double doppler_step) {
    return sdr::acq_grid(doppler_range, doppler_step).nbins;      // len(np.arange(-R, R+1, S))
}

int sdr_two_peak_compare(sdr_engine* e, const double* corr_map, int n_bins, int n_code, int samples_per_chip,
                         int64_t* peak_bin, int64_t* peak_code, double* peak_ratio) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!corr_map || !peak_bin || !peak_code || !peak_ratio) return sdr_fail(SDR_ERR_INVALID, "NULL argument");
    if (n_bins < 1 || n_code < 2 || samples_per_chip < 0) return sdr_fail(SDR_ERR_INVALID, "bad map geometry");
    const size_t count = (size_t)n_bins * n_code;
    int rc = sdr_devbuf_reserve(e, &e->pcps_map, count * sizeof(double));
    if (!rc) rc = sdr_devbuf_reserve(e, &e->pcps_part, kPeakParts * sizeof(Best));
    if (!rc) rc = sdr_devbuf_reserve(e, &e->pcps_res, result_block(1, false, true, false, nullptr).bytes);
    if (rc) return rc;
    double* map = (double*)e->pcps_map.ptr;
    const ResultBlock res = result_block(1, false, true, false, e->pcps_res.ptr);
    SDR_HIP(hipMemcpyAsync(map, corr_map, count * sizeof(double), hipMemcpyHostToDevice, e->stream));
    {
        ProfScope ps(e, "pcps_peak");
        hipLaunchKernelGGL(argmax_part_kernel, dim3(kPeakParts, 1), dim3(kThreads), 0, e->stream, map,
                           (long long)count, (Best*)e->pcps_part.ptr);
        hipLaunchKernelGGL(peak_finish_kernel, dim3(1), dim3(kThreads), 0, e->stream, map, n_bins, n_code,
                           samples_per_chip, (const Best*)e->pcps_part.ptr, res.bin, res.code, res.ratio);
    }
    SDR_HIP(hipGetLastError());
    long long host[3];
    SDR_HIP(hipMemcpyAsync(host, res.bin, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    *peak_bin = host[0];
    *peak_code = host[1];
    memcpy(peak_ratio, &host[2], sizeof(double));
    return SDR_OK;
}

// by_signal: sdr_pcps_signal's request (acq_signal_check: `sig` gives the chip rate, the padding and the exclusion window,
// the slots the code length); else sdr_pcps's and sdr_pcps_spectra's.  Behind the check the two are one search: a transform
// length, the samples per code kept of it, a chip rate.
static int pcps_impl(sdr_engine* e, bool by_signal, const sdr_acq_signal* sig, const int32_t* code_slots, const double* code_spectra,
                     int n_code_in, int n_prn, int64_t start_sample, double fs, double if_hz, double doppler_range,
                     double doppler_step, int coh, int noncoh, int64_t* peak_bin, int64_t* peak_code, double* peak_ratio,
                     double* corr_map, int* n_bins_out, int* n_code_out) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!peak_bin || !peak_code || !peak_ratio) return sdr_fail(SDR_ERR_INVALID, "NULL peak outputs");
    sdr::AcqRequest rq = sdr_acq_request(e, code_slots, n_prn, start_sample, fs, doppler_range, doppler_step,
                                         coh < 1 || noncoh < 1 ? 0 : (int64_t)coh * noncoh);
    rq.n_code = n_code_in;
    sdr::AcqShape shape;
    sdr::AcqSignalShape sg;
    int rc;
    if (by_signal) {
        rc = sdr::acq_signal_check(rq, sig, coh, noncoh, &shape, &sg);
    } else {
        rc = sdr::acq_request_check(rq, sdr::kAcqLimitsPcps, &shape);
        sg.N = sg.T = shape.N, sg.chip_rate = 1.023e6;
    }
    // N: the transform length; cols: the samples per code = the map's columns
    const int nbins = shape.grid.nbins, N = sg.T, cols = sg.N;
    if (n_bins_out && nbins > 0) *n_bins_out = nbins;
    if (rc) return sdr_fail(rc, "%s", shape.text);
    if (n_code_out) *n_code_out = cols;
    const PcpsPlan p = plan_pcps(pcps_switches(e), N, shape.spc, fs, nbins, shape.grid.bin_start, shape.grid.bin_delta, coh, noncoh,
                                 n_prn, corr_map != nullptr, cols, sg.chip_rate);

    const void* code2_before = e->pcps_code2.ptr;
    const std::pair<DevBuf*, size_t> bufs[] = {{&e->pcps_fwd, p.fwd_bytes}, {&e->pcps_a, p.work_bytes}, {&e->pcps_b, p.work_bytes},
                                               {&e->pcps_code, p.code_bytes}, {&e->pcps_code2, p.code2_bytes}, {&e->pcps_map, p.map_bytes},
                                               {&e->pcps_csum, p.csum_bytes}, {&e->pcps_part, p.part_bytes}, {&e->pcps_res, p.res_bytes}};
    for (const auto& b : bufs)       // (0 bytes: a buffer this search does not use)
        if (b.second && (rc = sdr_devbuf_reserve(e, b.first, b.second))) return rc;
    if (e->pcps_code2.ptr != code2_before) e->pcps_code2_ok = false;
    BluPlan blu;
    if ((rc = prepare_tables(e, p, &blu))) return rc;
    // small transfers go through page-locked staging: one copy each way, no hidden synchronisation
    // page-locked: [results: bin, code, ratio per PRN][slot numbers][done words]
    if ((rc = sdr_pinned_reserve(e, &e->ctx0, p.pinned_bytes))) return rc;
    const ResultBlock pin = result_block(n_prn, false, true, true, e->ctx0.pinned);
    const ResultBlock dev = result_block(n_prn, false, true, false, e->pcps_res.ptr);
    PcpsCall c;
    c.start = start_sample;
    c.if_hz = if_hz;
    c.slots = code_slots;
    c.d_slots = dev.slots;
    c.dev_bin = dev.bin, c.dev_code = dev.code;
    c.res_bin = pin.bin, c.res_code = pin.code, c.res_ratio = pin.ratio;
    c.blu = p.M ? &blu : nullptr;
    if (code_spectra) {
        SDR_HIP(hipMemcpyAsync(e->pcps_code.ptr, code_spectra, p.code_bytes, hipMemcpyHostToDevice, e->stream));
    } else {
        memcpy(pin.slots, code_slots, (size_t)n_prn * sizeof(int32_t));
        c.slots_pinned = pin.slots;      // (copied to the device when spectra have to be made)
    }
    c.done = pin.done;
    memset(c.done, 0, (size_t)n_prn * sizeof(unsigned));
    c.done_seq = ++e->pcps_done_counter ? e->pcps_done_counter : ++e->pcps_done_counter;

    {
        // (one event pair around every kernel of the search: its in-stream time; while it records, the search stays on one stream)
        ProfScope whole(e, by_signal ? "call_pcps_signal" : "call_pcps");
        rc = sdr::with_fmt(e->iq_fmt, [&](auto fmt) { return pcps_search<decltype(fmt)::value>(e, p, c); });
    }
    if (rc) {
        // a search that stopped half way: what the code-spectra buffer holds is unknown, and a sweep may still be
        // running on the second stream -- join it before anybody re-uses the work buffers
        e->pcps_spec_key.clear();
        if (e->pcps_aux) (void)hipStreamSynchronize(e->pcps_aux);
        return rc;
    }

    if (corr_map)
        SDR_HIP(hipMemcpyAsync(corr_map, e->pcps_map.ptr, (size_t)n_prn * nbins * cols * sizeof(double),
                               hipMemcpyDeviceToHost, e->stream));
    bool seen = false;
    if (p.done_words) {       // (bounded: a launch that died never raises the words -- the stream is asked then)
        const auto t0 = std::chrono::steady_clock::now();
        int k = 0;
        for (long spins = 0;; ++spins) {
            while (k < n_prn && __atomic_load_n(&c.done[k], __ATOMIC_ACQUIRE) == c.done_seq) ++k;
            if (k == n_prn) {
                seen = true;
                break;
            }
            if ((spins & 4095) == 4095 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.05) break;
        }
    }
    if (!seen) SDR_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; i < n_prn; ++i) {
        peak_bin[i] = c.res_bin[i];
        peak_code[i] = c.res_code[i];
    }
    memcpy(peak_ratio, c.res_ratio, (size_t)n_prn * sizeof(double));
    return SDR_OK;
}

int sdr_pcps(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, double fs, double if_hz,
             double doppler_range, double doppler_step, int coh, int noncoh, int64_t* peak_bin,
             int64_t* peak_code, double* peak_ratio, double* corr_map, int* n_bins_out) {
    if (!code_slots) return sdr_fail(SDR_ERR_INVALID, "code_slots is NULL");
    return pcps_impl(e, false, nullptr, code_slots, nullptr, 0, n_prn, start_sample, fs, if_hz, doppler_range, doppler_step, coh,
                     noncoh, peak_bin, peak_code, peak_ratio, corr_map, n_bins_out, nullptr);
}

int sdr_pcps_signal(sdr_engine* e, const sdr_acq_signal* sig, const int32_t* code_slots, int n_prn, int64_t start_sample, double fs,
                    double if_hz, double doppler_range, double doppler_step, int coh, int noncoh, int64_t* peak_bin,
                    int64_t* peak_code, double* peak_ratio, double* corr_map, int* n_bins_out, int* n_code_out) {
    return pcps_impl(e, true, sig, code_slots, nullptr, 0, n_prn, start_sample, fs, if_hz, doppler_range, doppler_step, coh, noncoh,
                     peak_bin, peak_code, peak_ratio, corr_map, n_bins_out, n_code_out);
}

int sdr_pcps_spectra(sdr_engine* e, const double* code_spectra, int n_prn, int n_code, int64_t start_sample,
                     double fs, double if_hz, double doppler_range, double doppler_step, int coh, int noncoh,
                     int64_t* peak_bin, int64_t* peak_code, double* peak_ratio, double* corr_map,
                     int* n_bins_out) {
    if (!code_spectra || n_code < 2) return sdr_fail(SDR_ERR_INVALID, "code_spectra is NULL or too short");
    return pcps_impl(e, false, nullptr, nullptr, code_spectra, n_code, n_prn, start_sample, fs, if_hz, doppler_range, doppler_step,
                     coh, noncoh, peak_bin, peak_code, peak_ratio, corr_map, n_bins_out, nullptr);
}


// sdr_acq_deep (det == nullptr: nothing below differs from the search alone) and sdr_acq_deep_detect (det, peaks, noise): the
// detection passes run behind the search's own peak kernels, on the maps where they lie.
static int acq_deep_impl(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, const sdr_deep_cfg* cfg,
                         sdr_deep_result* results, double* corr_map, const sdr_detect_cfg* det, sdr_detect_peak* peaks,
                         sdr_detect_noise* noise) {
    if (int rc = sdr_set_device(e)) return rc;
    if (!code_slots || !cfg || !results) return sdr_fail(SDR_ERR_INVALID, "NULL argument");
    if (det) {
        if (!peaks || !noise) return sdr_fail(SDR_ERR_INVALID, "NULL peaks / noise");
        if (det->n_peaks < 1 || det->n_peaks > sdr::kDetectMaxPeaks)
            return sdr_fail(SDR_ERR_INVALID, "n_peaks = %d outside 1..%d", det->n_peaks, sdr::kDetectMaxPeaks);
        if (det->excl_code < 0 || det->excl_bins < 0 || det->reserved != 0)
            return sdr_fail(SDR_ERR_INVALID, "negative exclusion window or non-zero reserved field");
    }
    if (n_prn < 1) return sdr_fail(SDR_ERR_INVALID, "no PRN to search");
    const int C = cfg->coh, K = cfg->noncoh, G = cfg->groups;
    if (C < 1 || C > 20) return sdr_fail(SDR_ERR_INVALID, "coh = %d outside 1..20", C);
    if (K < 1) return sdr_fail(SDR_ERR_INVALID, "noncoh = %d < 1", K);
    if (G < 1 || G > 2 || K < G) return sdr_fail(SDR_ERR_INVALID, "groups = %d outside 1..2 or above noncoh = %d", G, K);
    if (!(cfg->fs > 0.0) || !std::isfinite(cfg->fs) || !std::isfinite(cfg->if_hz)) return sdr_fail(SDR_ERR_INVALID, "bad fs / if_hz");
    if (!(cfg->carrier_rf_hz >= 0.0) || !std::isfinite(cfg->carrier_rf_hz))
        return sdr_fail(SDR_ERR_INVALID, "carrier_rf_hz negative or not finite");
    const sdr::AcqRequest rq = sdr_acq_request(e, code_slots, n_prn, start_sample, cfg->fs, cfg->doppler_range, cfg->doppler_step,
                                               (int64_t)C * K);
    sdr::AcqShape shape;
    if (int rc = sdr::acq_request_check(rq, sdr::kAcqLimitsDeep, &shape)) return sdr_fail(rc, "%s", shape.text);
    const int nbins = shape.grid.nbins, N = shape.N;
    if (det && !sdr::detect_windows_fit(det->n_peaks, det->excl_code, N))
        return sdr_fail(SDR_ERR_INVALID, "%d peaks x (2 x %d + 1) excluded columns leave no noise cell of %d", det->n_peaks,
                        det->excl_code, N);
    if (det && sdr::detect_row_parts(N) > 65535) return sdr_fail(SDR_ERR_UNSUPPORTED, "grid too large");
    // the map route's plan of coh = 1 (transforms, PRN chunks, work buffers); the deep route's own buffers on top
    const PcpsPlan p = plan_pcps(pcps_switches(e), N, shape.spc, cfg->fs, nbins, shape.grid.bin_start, shape.grid.bin_delta, 1, K,
                                 n_prn, true);

    int rc;
    const size_t row_bytes = (size_t)nbins * N * sizeof(double);
    const size_t res_bytes = result_block(n_prn, true, true, false, nullptr).bytes;     // row, code, ratio, value per PRN; the slot numbers
    const std::pair<DevBuf*, size_t> bufs[] = {{&e->pcps_fwd, p.fwd_bytes}, {&e->pcps_a, p.work_bytes}, {&e->pcps_b, p.work_bytes},
                                               {&e->pcps_code, p.code_bytes}, {&e->pcps_map, (size_t)n_prn * G * row_bytes},
                                               {&e->pcps_part, p.part_bytes}, {&e->pcps_res, res_bytes},
                                               {&e->deep_fold, 2 * row_bytes}, {&e->deep_mag, (size_t)p.prn_chunk * row_bytes},
                                               {&e->deep_q, (size_t)K * nbins * sizeof(int32_t)}};
    for (const auto& b : bufs)
        if ((rc = sdr_devbuf_reserve(e, b.first, b.second))) return rc;
    if (det && (rc = sdr_devbuf_reserve(e, &e->deep_det, sdr_deep_detect_bytes(n_prn, G * nbins, N)))) return rc;
    BluPlan blu;
    if ((rc = prepare_tables(e, p, &blu))) return rc;
    if ((rc = sdr_pinned_reserve(e, &e->ctx0, (size_t)n_prn * sizeof(int32_t)))) return rc;
    memcpy(e->ctx0.pinned, code_slots, (size_t)n_prn * sizeof(int32_t));

    // q[b][i]: made here by sdr_acq_deep_shift's one expression, reduced with Python's modulo; the device rounds nothing
    std::vector<int32_t> q((size_t)K * nbins);
    for (int i = 0; i < K; ++i)
        for (int b = 0; b < nbins; ++b) {
            const int64_t r = sdr_acq_deep_shift(cfg, b, i) % N;
            q[(size_t)i * nbins + b] = (int32_t)(r < 0 ? r + N : r);
        }
    SDR_HIP(hipMemcpyAsync(e->deep_q.ptr, q.data(), q.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));      // (pageable source: complete before `q` goes)

    PcpsCall c;
    c.slots = code_slots;
    c.slots_pinned = (const int32_t*)e->ctx0.pinned;
    const ResultBlock dev = result_block(n_prn, true, true, false, e->pcps_res.ptr);
    c.d_slots = dev.slots;
    c.res_bin = dev.bin, c.res_code = dev.code, c.res_ratio = dev.ratio, c.res_value = dev.value;
    c.blu = p.M ? &blu : nullptr;
    DeepCall d;
    d.start = start_sample;
    d.if_hz = cfg->if_hz;
    d.coh = C, d.noncoh = K, d.groups = G;
    d.q = (const int32_t*)e->deep_q.ptr;
    d.fold = (double2*)e->deep_fold.ptr;
    d.mag = (double*)e->deep_mag.ptr;
    const DeepDetectWs ws = det ? sdr_deep_detect_ws(e->deep_det.ptr, n_prn) : DeepDetectWs{};
    {
        ProfScope whole(e, det ? "call_acq_deep_detect" : "call_acq_deep");
        rc = code_spectra<SDR_FMT_CF64>(e, p, c);
        if (!rc) rc = run_deep(e, p, c, d);
        if (!rc && det)
            rc = sdr_deep_detect(e, (const double*)e->pcps_map.ptr, n_prn, G * nbins, nbins, N, det, c.res_bin, c.res_code,
                                 c.res_value, ws);
    }
    if (rc) {
        e->pcps_spec_key.clear();      // (a search that stopped half way: what the code-spectra buffer holds is unknown)
        return rc;
    }
    std::vector<long long> host(4 * (size_t)n_prn);
    SDR_HIP(hipMemcpyAsync(host.data(), dev.bin, host.size() * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    std::vector<DeepDetectPeak> host_peaks(det ? (size_t)n_prn * sdr::kDetectMaxPeaks : 0);
    std::vector<sdr_detect_noise> host_noise(det ? (size_t)n_prn : 0);
    if (det) {
        SDR_HIP(hipMemcpyAsync(host_peaks.data(), ws.peaks, host_peaks.size() * sizeof(DeepDetectPeak), hipMemcpyDeviceToHost,
                               e->stream));
        SDR_HIP(hipMemcpyAsync(host_noise.data(), ws.noise, host_noise.size() * sizeof(sdr_detect_noise), hipMemcpyDeviceToHost,
                               e->stream));
    }
    if (corr_map)
        SDR_HIP(hipMemcpyAsync(corr_map, e->pcps_map.ptr, (size_t)n_prn * G * row_bytes, hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    for (int i = 0; det && i < n_prn; ++i) {
        noise[i] = host_noise[(size_t)i];
        const double sigma = std::sqrt(noise[i].variance);
        for (int k = 0; k < det->n_peaks; ++k) {
            const DeepDetectPeak& h = host_peaks[(size_t)i * sdr::kDetectMaxPeaks + k];
            sdr_detect_peak& o = peaks[(size_t)i * det->n_peaks + k];
            o.group = h.row < 0 ? -1 : h.row / nbins;
            o.reserved = 0;
            o.bin = h.row < 0 ? 0 : h.row % nbins;
            o.code = h.code;
            const int64_t end = (o.code + sdr_acq_deep_shift(cfg, (int)o.bin, K)) % N;
            o.code_end = h.row < 0 ? 0 : (end < 0 ? end + N : end);
            o.value = h.value;
            o.z = (o.value - noise[i].mean) / sigma;
        }
    }
    for (int i = 0; i < n_prn; ++i) {
        sdr_deep_result& r = results[i];
        const long long row = host[(size_t)i];
        r.peak_group = (int32_t)(row / nbins);
        r.reserved = 0;
        r.peak_bin = row % nbins;
        r.peak_code = host[(size_t)n_prn + i];
        memcpy(&r.peak_ratio, &host[2 * (size_t)n_prn + i], sizeof(double));
        memcpy(&r.peak_value, &host[3 * (size_t)n_prn + i], sizeof(double));
        const int64_t end = (r.peak_code + sdr_acq_deep_shift(cfg, (int)r.peak_bin, K)) % N;
        r.peak_code_end = end < 0 ? end + N : end;
    }
    return SDR_OK;
}

int sdr_acq_deep(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, const sdr_deep_cfg* cfg,
                 sdr_deep_result* results, double* corr_map) {
    return acq_deep_impl(e, code_slots, n_prn, start_sample, cfg, results, corr_map, nullptr, nullptr, nullptr);
}

int sdr_acq_deep_detect(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, const sdr_deep_cfg* cfg,
                        const sdr_detect_cfg* det, sdr_deep_result* results, sdr_detect_peak* peaks, sdr_detect_noise* noise,
                        double* corr_map) {
    if (!det) return sdr_fail(SDR_ERR_INVALID, "NULL detection settings");
    return acq_deep_impl(e, code_slots, n_prn, start_sample, cfg, results, corr_map, det, peaks, noise);
}

int sdr_pcps_coherent(sdr_engine* e, const sdr_coh_cfg* cfg, const int32_t* code_slots, const int32_t* sec_rows, int n_prn,
                      const int8_t* sec_codes, int n_sec, int64_t start_sample, double fs, double if_hz, double doppler_range,
                      double doppler_step, sdr_coh_result* results, double* corr_map, double* power, int* n_bins_out, int* n_code_out) {
    if (int rc = sdr_set_device(e)) return rc;
    sdr::CohRequest rq;
    rq.acq = sdr_acq_request(e, code_slots, n_prn, start_sample, fs, doppler_range, doppler_step, 1);
    rq.cfg = cfg, rq.sec_rows = sec_rows, rq.sec_codes = sec_codes, rq.n_sec = n_sec;
    rq.K = cfg ? sdr_acq_refine_bins(cfg->span_hz, cfg->step_hz) : 0;
    rq.results = results != nullptr;
    sdr::CohShape shape;
    int rc = sdr::coherent_request_check(rq, &shape);
    const int nbins = shape.acq.grid.nbins;
    if (n_bins_out && nbins > 0) *n_bins_out = nbins;
    if (rc) return sdr_fail(rc, "%s", shape.acq.text);
    const int N = shape.sig.N, T = shape.sig.T, M = cfg->n_periods, Ls = cfg->sec_len, K = rq.K;
    if (n_code_out) *n_code_out = N;
    // the zero-padded map route's plan (the transforms, the tables, the code spectra, the peaks); the buffers of this route on top
    PcpsPlan p = plan_pcps(pcps_switches(e), T, shape.acq.spc, fs, nbins, shape.acq.grid.bin_start, shape.acq.grid.bin_delta, 1, M,
                           n_prn, true, N, shape.sig.chip_rate);
    CohCall k;
    k.cap = sdr::coherent_chunk_units(e->coh_scratch_kb * 1024, M, T);
    int most = 0;      // units of the largest chunk
    for (int i = 0, n = sdr::coherent_chunk_count(k.cap, n_prn, nbins); i < n; ++i)
        most = std::max(most, sdr::coherent_chunk(k.cap, n_prn, nbins, i).units());
    const size_t in_flight = (size_t)std::max(most, std::max(nbins, n_prn));
    p.work_bytes = p.tbytes * in_flight;
    if (p.M) p.blu_work_bytes = (size_t)p.M * sizeof(double2) * std::max<size_t>(2, in_flight);
    auto round16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t b_sec = round16((size_t)n_sec * Ls), b_rows = round16((size_t)n_prn * sizeof(int32_t));
    const size_t b_best = (size_t)n_prn * sizeof(Best), b_keep = (size_t)n_prn * M * sizeof(double2);
    const size_t b_res = (size_t)n_prn * sizeof(sdr_coh_result), b_pow = (size_t)n_prn * Ls * K * sizeof(double);
    static_assert(sizeof(sdr_coh_result) % 16 == 0, "the power table behind the results stays aligned");
    const std::pair<DevBuf*, size_t> bufs[] = {{&e->pcps_fwd, std::max(p.fwd_bytes, p.tbytes * (size_t)M * nbins)},
                                               {&e->pcps_a, p.work_bytes}, {&e->pcps_b, p.work_bytes}, {&e->pcps_code, p.code_bytes},
                                               {&e->pcps_map, p.map_bytes}, {&e->pcps_part, p.part_bytes}, {&e->pcps_res, p.res_bytes},
                                               {&e->coh_scr, p.tbytes * (size_t)M * most},
                                               {&e->coh_ws, b_sec + b_rows + b_best + b_keep + b_res + b_pow}};
    for (const auto& b : bufs)
        if ((rc = sdr_devbuf_reserve(e, b.first, b.second))) return rc;
    BluPlan blu;
    if ((rc = prepare_tables(e, p, &blu))) return rc;
    if ((rc = sdr_pinned_reserve(e, &e->ctx0, (size_t)n_prn * sizeof(int32_t)))) return rc;
    memcpy(e->ctx0.pinned, code_slots, (size_t)n_prn * sizeof(int32_t));
    // the overlay rows and every PRN's row number, in the engine's own block (the source of the upload outlives the call)
    e->coh_host.resize(b_sec + b_rows);
    memcpy(e->coh_host.data(), sec_codes, (size_t)n_sec * Ls);
    memcpy(e->coh_host.data() + b_sec, sec_rows, (size_t)n_prn * sizeof(int32_t));
    char* ws = (char*)e->coh_ws.ptr;
    SDR_HIP(hipMemcpyAsync(ws, e->coh_host.data(), b_sec + b_rows, hipMemcpyHostToDevice, e->stream));

    CohGeom g;
    g.N = N, g.T = T, g.M = M, g.Ls = Ls, g.K = K, g.mode = cfg->mode, g.nbins = nbins;
    g.fs = fs, g.if_hz = if_hz, g.bin_start = p.bin_start, g.bin_delta = p.bin_delta, g.step_hz = cfg->step_hz;
    g.sec = (const int8_t*)ws, g.sec_rows = (const int32_t*)(ws + b_sec);
    k.scr = (double2*)e->coh_scr.ptr;
    k.best = ws + b_sec + b_rows;
    k.keep = ws + b_sec + b_rows + b_best;
    k.results = (sdr_coh_result*)(ws + b_sec + b_rows + b_best + b_keep);
    k.power = (double*)(ws + b_sec + b_rows + b_best + b_keep + b_res);
    PcpsCall c;
    c.start = start_sample;
    c.if_hz = if_hz;
    c.slots = code_slots;
    c.slots_pinned = (const int32_t*)e->ctx0.pinned;
    const ResultBlock dev = result_block(n_prn, false, true, false, e->pcps_res.ptr);
    c.d_slots = dev.slots;
    c.res_bin = dev.bin, c.res_code = dev.code, c.res_ratio = dev.ratio;
    c.blu = p.M ? &blu : nullptr;
    {
        ProfScope whole(e, "call_pcps_coherent");
        rc = sdr::with_fmt(e->iq_fmt, [&](auto fmt) { return run_coherent<decltype(fmt)::value>(e, p, c, g, k); });
    }
    if (rc) {
        e->pcps_spec_key.clear();      // (a search that stopped half way: what the code-spectra buffer holds is unknown)
        return rc;
    }
    SDR_HIP(hipMemcpyAsync(results, k.results, b_res, hipMemcpyDeviceToHost, e->stream));
    if (power) SDR_HIP(hipMemcpyAsync(power, k.power, b_pow, hipMemcpyDeviceToHost, e->stream));
    if (corr_map)
        SDR_HIP(hipMemcpyAsync(corr_map, e->pcps_map.ptr, (size_t)n_prn * nbins * N * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    SDR_HIP(hipStreamSynchronize(e->stream));
    return SDR_OK;
}

}  // extern "C"
