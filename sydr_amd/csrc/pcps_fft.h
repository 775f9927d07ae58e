// The transforms of the acquisition searches (K2-K5): a hand-written mixed-radix (2,3,4,5,8 + small primes) Stockham autosort
// FFT in fp64, batched over (PRN, bin) -- one kernel per radix pass, or the four-step pair with both sub-transforms in LDS where
// the planner splits N (pcps_plan.h), the register-resident kernels of pcps_fast.h / pcps_fastn.h for the inverse transforms
// at the usual rates, and the chirp-z transform for a length the planner cannot factor.  The Doppler mix and the int8->fp64
// conversion are fused into the first forward pass, the code-spectrum multiply into the first inverse pass, and 1/N scale +
// magnitude + (non-)coherent accumulation, or the running maximum of the map-free search, into the last inverse pass
// (PassArgs, the load / store modes).  run_fft is the one way in.  pcps_fast.h / pcps_fastn.h need PassArgs and Butterfly and
// include this header; the dispatch here needs their entry points and declares them; the translation unit that calls run_fft
// (pcps.hip, alone: the kernels are compiled once) includes all three.
#pragma once

#include "engine_internal.h"
#include "pcps_codelets.h"
#include "pcps_plan.h"
#include "sincos_reduced.h"

#include <cmath>
#include <type_traits>
#include <vector>

#pragma clang fp contract(off)

namespace {

using pcps::kThreads;
using pcps::kRowTile;
using pcps::Radices;
using pcps::FourStep;
using pcps::Xform;
using pcps::FAST_25K;

enum LoadMode { LOAD_PLAIN = 0, LOAD_IQ_MIX = 1, LOAD_MUL_CODE = 2, LOAD_CODE_REAL = 3, LOAD_MUL_CODE_SEL = 4 };
// STORE_MAG_MAX: nothing is stored -- the last stage keeps a running (maximum, first index) of |.|/N per wave and
// writes one 16-byte record per wave (the map-free search: the caller only wants indices and ratio).
// STORE_MAG_KEEP: STORE_MAG_ACC for the first `cols` outputs of every transform alone, at row pitch `cols` (the zero-padded
// search of sdr_pcps_signal: the lags at and beyond one code period of a two-period transform are neither turned into
// magnitudes nor written).
enum StoreMode { STORE_PLAIN = 0, STORE_CONJ = 1, STORE_MAG_ACC = 2, STORE_CPLX_ACC = 3, STORE_MAG_MAX = 4, STORE_MAG_KEEP = 5 };


struct PassArgs {
    const double2* in;    // [batch][N]
    double2* out;         // [batch][N]
    const double2* tw;    // W[m] = exp(-2*pi*i*m/N)
    int N, R, Ns, nbf;    // nbf = N / R butterflies per transform
    int tw_stride;        // N / (Ns * R)
    // LOAD_IQ_MIX
    const void* ring;
    int64_t capacity;
    int64_t first_sample;  // ring index of sample 0 of this 1 ms block
    int64_t carrier_offset;  // idx_coh * N (index into phasePoints)
    double fs, if_hz, bin_start, bin_delta;
    // LOAD_MUL_CODE: in = F[nbins][N]; code spectra [n_prn][N]
    const double2* code_spec;
    int nbins, n_prn;
    // LOAD_CODE_REAL
    const int8_t* code_samples;  // [batch][N]
    // STORE_*_ACC
    double* map;        // [batch][N] magnitudes
    double2* csum;      // [batch][N]
    double scale;
    int first_block;    // 1: overwrite, 0: accumulate
    // LOAD_MUL_CODE_SEL: transform p takes Doppler row sel_bin[p] (the winning row of PRN p)
    const long long* sel_bin;
    // STORE_MAG_MAX: per-wave records, [batch][tiles][waves]
    Best* partials;
    // STORE_MAG_MAX behind LOAD_MUL_CODE_SEL (second peak of the winning row): the first peaks and samples per chip
    const Best* tops;
    int spc;
    // STORE_MAG_MAX of the register-resident kernels: `in` starts at Doppler bin bin0 of the search (a sweep over the last
    // bins only: the fused sweep took the others) -- added to the bin of the records' flat index
    int bin0;
    // LOAD_IQ_MIX over several blocks at once: bins per block (0: the batch is one block's bins)
    int iq_blocks;
    // STORE_PLAIN with a halo (shared spectra): row t of the output is halo + N elements long, element k goes to halo + k and
    // the row's last `halo` elements are written in front of it as well -- out[t][i] = X_t[(i - halo) mod N]
    int halo;
    // STORE_MAG_KEEP: outputs kept per transform = the map's row pitch, 1 <= cols <= N
    int cols;
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
// multiply by -i (forward) or +i (inverse)
template <bool INV>
__device__ __forceinline__ double2 mul_mi(double2 a) {
    return INV ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x);
}

template <int R, bool INV>
struct Butterfly;

template <bool INV>
struct Butterfly<2, INV> {
    static __device__ __forceinline__ void run(double2* v) {
        double2 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    }
};

template <bool INV>
struct Butterfly<3, INV> {
    static __device__ __forceinline__ void run(double2* v) {
        const double c = -0.5, s = 0.86602540378443864676;  // cos, sin of 2*pi/3
        double2 t1 = cadd(v[1], v[2]);
        double2 t2 = csub(v[1], v[2]);
        double2 m = make_double2(v[0].x + c * t1.x, v[0].y + c * t1.y);
        double2 r = mul_mi<INV>(make_double2(s * t2.x, s * t2.y));
        v[0] = cadd(v[0], t1);
        v[1] = cadd(m, r);
        v[2] = csub(m, r);
    }
};

template <bool INV>
struct Butterfly<4, INV> {
    static __device__ __forceinline__ void run(double2* v) {
        double2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
        double2 t2 = cadd(v[1], v[3]), t3 = mul_mi<INV>(csub(v[1], v[3]));
        v[0] = cadd(t0, t2);
        v[1] = cadd(t1, t3);
        v[2] = csub(t0, t2);
        v[3] = csub(t1, t3);
    }
};

template <bool INV>
struct Butterfly<5, INV> {
    static __device__ __forceinline__ void run(double2* v) {
        const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;  // cos(2pi/5), cos(4pi/5)
        const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;   // sin(2pi/5), sin(4pi/5)
        double2 a1 = cadd(v[1], v[4]), b1 = csub(v[1], v[4]);
        double2 a2 = cadd(v[2], v[3]), b2 = csub(v[2], v[3]);
        double2 m1 = make_double2(v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y);
        double2 m2 = make_double2(v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y);
        double2 r1 = mul_mi<INV>(make_double2(s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y));
        double2 r2 = mul_mi<INV>(make_double2(s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y));
        v[0] = cadd(v[0], cadd(a1, a2));
        v[1] = cadd(m1, r1);
        v[4] = csub(m1, r1);
        v[2] = cadd(m2, r2);
        v[3] = csub(m2, r2);
    }
};

template <bool INV>
struct Butterfly<8, INV> {
    static __device__ __forceinline__ void run(double2* v) {
        const double h = 0.70710678118654752440;
        // radix-2 split into evens / odds, two radix-4 butterflies, then combine.
        double2 e[4] = {v[0], v[2], v[4], v[6]};
        double2 o[4] = {v[1], v[3], v[5], v[7]};
        Butterfly<4, INV>::run(e);
        Butterfly<4, INV>::run(o);
        // twiddles W8^k, k = 1..3: (h, -+h), (0, -+1), (-h, -+h)
        double2 w1 = INV ? make_double2(h * (o[1].x - o[1].y), h * (o[1].x + o[1].y))
                         : make_double2(h * (o[1].x + o[1].y), h * (o[1].y - o[1].x));
        double2 w2 = mul_mi<INV>(o[2]);
        double2 w3 = INV ? make_double2(-h * (o[3].x + o[3].y), h * (o[3].x - o[3].y))
                         : make_double2(h * (o[3].y - o[3].x), -h * (o[3].x + o[3].y));
        v[0] = cadd(e[0], o[0]);
        v[4] = csub(e[0], o[0]);
        v[1] = cadd(e[1], w1);
        v[5] = csub(e[1], w1);
        v[2] = cadd(e[2], w2);
        v[6] = csub(e[2], w2);
        v[3] = cadd(e[3], w3);
        v[7] = csub(e[3], w3);
    }
};

template <int LOAD, int FMT, bool INV>
__device__ __forceinline__ double2 load_elem(const PassArgs& a, int batch, int idx) {
    if (LOAD == LOAD_PLAIN) {
        return a.in[(size_t)batch * a.N + idx];
    } else if (LOAD == LOAD_IQ_MIX) {
        // acquisition.py:33,42-45,53: carrier = exp(-1j*freq*phasePoints), phasePoints[m] = ((m*2)*pi)/fs
        // (iq_blocks > 0: the batch holds that many Doppler bins of several consecutive blocks of N samples -- transform b is
        // bin b % iq_blocks of block b / iq_blocks: every non-coherent block of a search in one launch)
        const int blk = a.iq_blocks > 0 ? batch / a.iq_blocks : 0;
        batch -= blk * a.iq_blocks;
        int64_t pos = (a.first_sample + (int64_t)blk * a.N + idx) % a.capacity;
        double2 x = sdr::ring_read<FMT>(a.ring, pos);
        double bin = a.bin_start + (double)batch * a.bin_delta;
        double freq = a.if_hz - bin;
        int64_t m = a.carrier_offset + idx;
        double pp = (double)(m * 2) * M_PI;
        pp = pp / a.fs;
        double arg = freq * pp;
        double s, c;
        // (|arg| stays below ~2*pi*f*T: a few hundred radians -- the exact two-constant reduction and the minimax kernels
        // of the correlators, < 1 ulp, instead of libm's general sincos with its large-argument path)
        sdr::sincos_reduced(arg, &s, &c);
        return cmul(make_double2(c, -s), x);
    } else if (LOAD == LOAD_MUL_CODE) {
        int prn = batch / a.nbins, bin = batch - prn * a.nbins;
        double2 f = a.in[(size_t)bin * a.N + idx];
        double2 c = a.code_spec[(size_t)prn * a.N + idx];
        return cmul(f, c);
    } else if (LOAD == LOAD_MUL_CODE_SEL) {
        const int bin = (int)a.sel_bin[batch];
        double2 f = a.in[(size_t)bin * a.N + idx];
        double2 c = a.code_spec[(size_t)batch * a.N + idx];
        return cmul(f, c);
    } else {
        return make_double2((double)a.code_samples[(size_t)batch * a.N + idx], 0.0);
    }
}

template <int STORE>
__device__ __forceinline__ void store_elem(const PassArgs& a, int batch, int idx, double2 v) {
    const size_t o = (size_t)batch * a.N + idx;
    if (STORE == STORE_PLAIN) {
        if (a.halo) {
            const size_t row = (size_t)batch * (size_t)(a.halo + a.N);
            a.out[row + a.halo + idx] = v;
            if (idx >= a.N - a.halo) a.out[row + (idx - (a.N - a.halo))] = v;
        } else {
            a.out[o] = v;
        }
    } else if (STORE == STORE_CONJ) {
        a.out[o] = make_double2(v.x, -v.y);
    } else if (STORE == STORE_MAG_ACC) {
        double mag = hypot(v.x * a.scale, v.y * a.scale);
        a.map[o] = a.first_block ? 0.0 + mag : a.map[o] + mag;
    } else if (STORE == STORE_MAG_MAX) {
        // (only the four-step row kernel implements the running maximum; the launcher never selects it elsewhere)
    } else if (STORE == STORE_MAG_KEEP) {
        if (idx >= a.cols) return;
        const size_t k = (size_t)batch * a.cols + idx;
        double mag = hypot(v.x * a.scale, v.y * a.scale);
        a.map[k] = a.first_block ? 0.0 + mag : a.map[k] + mag;
    } else {
        double2 s = make_double2(v.x * a.scale, v.y * a.scale);
        a.csum[o] = a.first_block ? s : cadd(a.csum[o], s);
    }
}

// One Stockham pass of radix R: thread j owns butterfly j of transform blockIdx.y.
template <int R, bool INV, int LOAD, int STORE, int FMT>
__global__ __launch_bounds__(kThreads) void fft_pass_kernel(const PassArgs a) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= a.nbf) return;
    const int batch = blockIdx.y;
    const int k = j % a.Ns;
    double2 v[R];
#pragma unroll
    for (int t = 0; t < R; ++t) v[t] = load_elem<LOAD, FMT, INV>(a, batch, j + t * a.nbf);
    if (a.Ns > 1) {
#pragma unroll
        for (int t = 1; t < R; ++t) {
            double2 w = a.tw[(size_t)t * k * a.tw_stride];
            if (INV) w.y = -w.y;
            v[t] = cmul(v[t], w);
        }
    }
    Butterfly<R, INV>::run(v);
    const int o = (j - k) * R + k;
#pragma unroll
    for (int t = 0; t < R; ++t) store_elem<STORE>(a, batch, o + t * a.Ns, v[t]);
}

// Any other prime radix (7, 11, 13, ...): O(R^2) DFT with roots from the twiddle table.
// (up to pcps::kMaxGenericRadix: factor_radices)
template <bool INV, int LOAD, int STORE, int FMT>
__global__ __launch_bounds__(kThreads) void fft_pass_generic_kernel(const PassArgs a) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= a.nbf) return;
    const int batch = blockIdx.y;
    const int R = a.R;
    const int k = j % a.Ns;
    const int root_stride = a.N / R;
    const int o = (j - k) * R + k;
    for (int q = 0; q < R; ++q) {
        double2 acc = make_double2(0.0, 0.0);
        for (int t = 0; t < R; ++t) {
            double2 x = load_elem<LOAD, FMT, INV>(a, batch, j + t * a.nbf);
            if (a.Ns > 1 && t > 0) {
                double2 w = a.tw[(size_t)t * k * a.tw_stride];
                if (INV) w.y = -w.y;
                x = cmul(x, w);
            }
            double2 r = a.tw[(size_t)((t * q) % R) * root_stride];
            if (INV) r.y = -r.y;
            acc = cadd(acc, cmul(x, r));
        }
        store_elem<STORE>(a, batch, o + q * a.Ns, acc);
    }
}

__global__ __launch_bounds__(kThreads) void twiddle_kernel(double2* tw, int N) {
    int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= N) return;
    double s, c;
    sincospi(2.0 * (double)m / (double)N, &s, &c);
    tw[m] = make_double2(c, -s);
}

template <bool INV, int LOAD, int STORE, int FMT>
void launch_pass(sdr_engine* e, const PassArgs& a, int batch) {
    dim3 grid((a.nbf + kThreads - 1) / kThreads, batch);
    switch (a.R) {
        case 2: hipLaunchKernelGGL((fft_pass_kernel<2, INV, LOAD, STORE, FMT>), grid, dim3(kThreads), 0, e->stream, a); break;
        case 3: hipLaunchKernelGGL((fft_pass_kernel<3, INV, LOAD, STORE, FMT>), grid, dim3(kThreads), 0, e->stream, a); break;
        case 4: hipLaunchKernelGGL((fft_pass_kernel<4, INV, LOAD, STORE, FMT>), grid, dim3(kThreads), 0, e->stream, a); break;
        case 5: hipLaunchKernelGGL((fft_pass_kernel<5, INV, LOAD, STORE, FMT>), grid, dim3(kThreads), 0, e->stream, a); break;
        case 8: hipLaunchKernelGGL((fft_pass_kernel<8, INV, LOAD, STORE, FMT>), grid, dim3(kThreads), 0, e->stream, a); break;
        default: hipLaunchKernelGGL((fft_pass_generic_kernel<INV, LOAD, STORE, FMT>), grid, dim3(kThreads), 0, e->stream, a); break;
    }
}

/* ------------------------------------------------------------------------------------------------
 * Four-step transform: N = N1*N2, both sub-transforms done in LDS, two kernels and ONE round trip
 * through HBM per transform instead of one per radix pass (7 passes at N = 25000):
 *   A  columns:  Y[k1][n2] = sum_n1 x[N2*n1 + n2] W_N1^(n1 k1),  Z[k1][n2] = Y[k1][n2] * W_N^(n2 k1)
 *   B  rows:     X[k1 + N1*k2] = sum_n2 Z[k1][n2] W_N2^(n2 k2)
 * A workgroup owns a tile of T adjacent columns (A) or rows (B) so that every global access is a run
 * of T*16 contiguous bytes; the fused loads (Doppler mix / code spectrum product) sit in A and the
 * fused stores (conj / |.|/N accumulate / running maximum) in B.
 * ------------------------------------------------------------------------------------------------ */
// LDS row pitch (in complex values) of a tile of T columns.  No padding for the 4- and 8-column tiles in use: the
// butterflies walk the tile row by row (consecutive lanes = consecutive columns, then the next row), so an unpadded
// tile is read and written in contiguous 64- / 128-byte runs; a pad of one complex measured 7 % slower (47 % of the
// LDS cycles of the row kernel were bank conflicts), two 16 % slower.
constexpr int lds_pitch(int T) { return (T == 4 || T == 8) ? T : T + 1; }

// x / d for x*d < 2^32 with magic = 2^32/d + 1: three integer ops instead of a ~25-instruction division.
__device__ __forceinline__ int fast_div(int x, uint32_t magic) { return (int)__umulhi((uint32_t)x, magic); }
__host__ __device__ __forceinline__ uint32_t div_magic(int d) { return (uint32_t)(0x100000000ull / (uint32_t)d) + 1u; }

// One radix-R butterfly of a Stockham pass over data laid out [index][pitch] in LDS, column c.
template <int R, bool INV>
__device__ __forceinline__ void lds_butterfly(const double2* in, double2* out, int j, int c, int pitch, int nbf,
                                              int Ns, int tws, const double2* wsub, uint32_t ns_magic) {
    const int k = Ns == 1 ? 0 : j - fast_div(j, ns_magic) * Ns;
    double2 v[R];
#pragma unroll
    for (int t = 0; t < R; ++t) v[t] = in[(j + t * nbf) * pitch + c];
    if (Ns > 1) {
#pragma unroll
        for (int t = 1; t < R; ++t) {
            double2 w = wsub[t * k * tws];
            if (INV) w.y = -w.y;
            v[t] = cmul(v[t], w);
        }
    }
    Butterfly<R, INV>::run(v);
    const int o = (j - k) * R + k;
#pragma unroll
    for (int t = 0; t < R; ++t) out[(o + t * Ns) * pitch + c] = v[t];
}

template <bool INV>
__device__ __forceinline__ void lds_butterfly_generic(const double2* in, double2* out, int R, int j, int c, int pitch,
                                                      int nbf, int Ns, int tws, int Nsub, const double2* wsub,
                                                      uint32_t ns_magic) {
    const int k = Ns == 1 ? 0 : j - fast_div(j, ns_magic) * Ns;
    const int o = (j - k) * R + k;
    const int root = Nsub / R;
    for (int q = 0; q < R; ++q) {
        double2 acc = make_double2(0.0, 0.0);
        for (int t = 0; t < R; ++t) {
            double2 x = in[(j + t * nbf) * pitch + c];
            if (Ns > 1 && t > 0) {
                double2 w = wsub[t * k * tws];
                if (INV) w.y = -w.y;
                x = cmul(x, w);
            }
            double2 r = wsub[((t * q) % R) * root];
            if (INV) r.y = -r.y;
            acc = cadd(acc, cmul(x, r));
        }
        out[(o + q * Ns) * pitch + c] = acc;
    }
}

// In-LDS Stockham transform of `T` columns of length Nsub; returns the buffer holding the result.
template <bool INV, int T>
__device__ __forceinline__ double2* lds_fft(double2* a, double2* b, int Nsub, const Radices& rad, const double2* wsub) {
    constexpr int pitch = lds_pitch(T);
    int Ns = 1;
    double2* in = a;
    double2* out = b;
    for (int p = 0; p < rad.n; ++p) {
        const int R = rad.r[p];
        const int nbf = Nsub / R;
        const int tws = Nsub / (Ns * R);
        const uint32_t ns_magic = div_magic(Ns);
        for (int bf = threadIdx.x; bf < nbf * T; bf += kThreads) {
            const int j = bf / T, c = bf - j * T;
            switch (R) {
                case 2: lds_butterfly<2, INV>(in, out, j, c, pitch, nbf, Ns, tws, wsub, ns_magic); break;
                case 3: lds_butterfly<3, INV>(in, out, j, c, pitch, nbf, Ns, tws, wsub, ns_magic); break;
                case 4: lds_butterfly<4, INV>(in, out, j, c, pitch, nbf, Ns, tws, wsub, ns_magic); break;
                case 5: lds_butterfly<5, INV>(in, out, j, c, pitch, nbf, Ns, tws, wsub, ns_magic); break;
                case 8: lds_butterfly<8, INV>(in, out, j, c, pitch, nbf, Ns, tws, wsub, ns_magic); break;
                default: lds_butterfly_generic<INV>(in, out, R, j, c, pitch, nbf, Ns, tws, Nsub, wsub, ns_magic); break;
            }
        }
        __syncthreads();
        double2* tmp = in;
        in = out;
        out = tmp;
        Ns *= R;
    }
    return in;
}

// The same transform with the radix sequence known at compile time (every index constant folds: no
// runtime division, no radix switch, twiddle strides are immediates).
template <bool INV, int T, int NSUB, int NS, int R0, int... Rs>
__device__ __forceinline__ double2* lds_fft_static(double2* in, double2* out, const double2* wsub) {
    constexpr int pitch = lds_pitch(T);
    constexpr int nbf = NSUB / R0;
    constexpr int tws = NSUB / (NS * R0);
    for (int bf = threadIdx.x; bf < nbf * T; bf += kThreads) {
        const int j = bf / T, c = bf - j * T;
        lds_butterfly<R0, INV>(in, out, j, c, pitch, nbf, NS, tws, wsub, div_magic(NS));
    }
    __syncthreads();
    if constexpr (sizeof...(Rs) == 0)
        return out;
    else
        return lds_fft_static<INV, T, NSUB, NS * R0, Rs...>(out, in, wsub);
}

// Sub-transform lengths of the usual sampling rates (N = 4000: 50 x 80, 10000: 100 x 100, 25000: 125 x 200,
// 50000: 200 x 250) run the compile-time version -- 13 % off a whole acquisition at N = 25000; the sequences are
// those factor_radices() produces, so both versions do the same arithmetic in the same order.
template <bool INV, int T>
__device__ __forceinline__ double2* lds_fft_auto(double2* a, double2* b, int Nsub, const Radices& rad, const double2* wsub) {
    switch (Nsub) {
        case 50: return lds_fft_static<INV, T, 50, 1, 5, 5, 2>(a, b, wsub);
        case 80: return lds_fft_static<INV, T, 80, 1, 5, 8, 2>(a, b, wsub);
        case 100: return lds_fft_static<INV, T, 100, 1, 5, 5, 4>(a, b, wsub);
        case 125: return lds_fft_static<INV, T, 125, 1, 5, 5, 5>(a, b, wsub);
        case 200: return lds_fft_static<INV, T, 200, 1, 5, 5, 8>(a, b, wsub);
        case 250: return lds_fft_static<INV, T, 250, 1, 5, 5, 5, 2>(a, b, wsub);
        default: return lds_fft<INV, T>(a, b, Nsub, rad, wsub);
    }
}

// The raw operands of one element of the fused first stage, fetched without being combined: the global loads of
// several elements are issued back to back and waited for once (a loop of load -> use pays one memory round trip per
// iteration, ~1 us each under load, which is what these kernels' time was made of).
struct Fetched {
    double2 p, q;
};
template <int LOAD, int FMT, bool INV>
__device__ __forceinline__ Fetched fetch_elem(const PassArgs& a, int batch, int bin, int prn, int idx) {
    Fetched f;
    if constexpr (LOAD == LOAD_MUL_CODE || LOAD == LOAD_MUL_CODE_SEL) {
        f.p = a.in[(size_t)bin * a.N + idx];
        f.q = a.code_spec[(size_t)prn * a.N + idx];
    } else if constexpr (LOAD == LOAD_PLAIN) {
        f.p = a.in[(size_t)batch * a.N + idx];
        f.q = make_double2(0.0, 0.0);
    } else {
        f.p = load_elem<LOAD, FMT, INV>(a, batch, idx);
        f.q = make_double2(0.0, 0.0);
    }
    return f;
}
template <int LOAD>
__device__ __forceinline__ double2 combine_elem(const Fetched& f) {
    if constexpr (LOAD == LOAD_MUL_CODE || LOAD == LOAD_MUL_CODE_SEL) return cmul(f.p, f.q);
    else return f.p;
}

constexpr int kBatchLoads = 4;  // elements per lane whose loads are in flight together

// Kernel A: T adjacent columns n2 of one transform.  Dynamic LDS: 2 * N1*(T+1) + N1 double2.
template <bool INV, int LOAD, int FMT, int T>
__global__ __launch_bounds__(kThreads) void fft4_cols_kernel(const PassArgs a, int N1, int N2, const Radices rad,
                                                             double2* __restrict__ Z) {
    extern __shared__ double2 lds4[];
    constexpr int pitch = lds_pitch(T);
    double2* bufA = lds4;
    double2* bufB = bufA + N1 * pitch;
    double2* wsub = bufB + N1 * pitch;
    int batch = blockIdx.y;
    int n2_0 = blockIdx.x * T;
    int prn = batch, bin = batch;
    if constexpr (LOAD == LOAD_MUL_CODE) {
        // XCD-aware mapping (1-D grid).  Every (PRN, bin) transform multiplies the bin's spectrum by the PRN's code
        // spectrum: 29 MB of unique operands at 32 PRN x 41 bins x 25000, read 1312 times over.  Workgroups are dealt
        // to the 8 XCDs round-robin by linear id, each XCD with its own 4 MB L2 -- in (tile, batch) order every XCD
        // ends up streaming all of it (measured 629 MB per call, 8 x the code spectra + every spectrum tile per PRN).
        // Here XCD x = id % 8 owns a contiguous eighth of the (column tile, bin) pairs -- 2 MB of spectrum tiles and
        // the code tiles of ~3 column tiles, both L2-resident -- and runs all PRNs of a pair back to back.
        const int tiles = (N2 + T - 1) / T;
        const int n_prn = a.n_prn;
        const int pairs = tiles * a.nbins;
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        const int p_lo = (int)(((long long)pairs * xcd) >> 3), p_hi = (int)(((long long)pairs * (xcd + 1)) >> 3);
        const int pair = p_lo + slot / n_prn;
        if (pair >= p_hi) return;                       // (the grid is padded to the largest eighth)
        prn = slot - (slot / n_prn) * n_prn;
        const int tile = pair / a.nbins;
        bin = pair - tile * a.nbins;
        batch = prn * a.nbins + bin;
        n2_0 = tile * T;
    } else if constexpr (LOAD == LOAD_MUL_CODE_SEL) {
        bin = (int)a.sel_bin[batch];
    }
    const int total = N1 * T;
    const uint32_t t_magic = div_magic(T);
    // W_N1^m = W_N^(m*N2) for the sub-transform (read together with the first elements)
    for (int base = 0; base < total; base += kBatchLoads * kThreads) {
        Fetched f[kBatchLoads];
        int slot[kBatchLoads];
        double2 wv = make_double2(0.0, 0.0);
        // (each chunk of kBatchLoads*256 elements also brings 256 entries of the sub-transform's twiddle table:
        // T >= kBatchLoads chunks' worth cover all N1 of them)
        static_assert(T >= kBatchLoads, "the twiddle table rides along with the element chunks");
        const int m = base / kBatchLoads + threadIdx.x;
        const bool wm = m < N1;
        if (wm) wv = a.tw[(size_t)m * N2];
#pragma unroll
        for (int u = 0; u < kBatchLoads; ++u) {
            const int e = base + u * kThreads + threadIdx.x;
            const int n1 = fast_div(e, t_magic), c = e - n1 * T;
            const int n2 = n2_0 + c;
            const bool ok = e < total && n2 < N2;
            slot[u] = e < total ? n1 * pitch + c : -1;
            f[u].p = f[u].q = make_double2(0.0, 0.0);
            if (ok) f[u] = fetch_elem<LOAD, FMT, INV>(a, batch, bin, prn, N2 * n1 + n2);
        }
        if (wm) wsub[m] = wv;
#pragma unroll
        for (int u = 0; u < kBatchLoads; ++u)
            if (slot[u] >= 0) bufA[slot[u]] = combine_elem<LOAD>(f[u]);
    }
    __syncthreads();
    double2* res = lds_fft_auto<INV, T>(bufA, bufB, N1, rad, wsub);
    // Twiddle W_N^(n2*k1) = W_N^(n2_0*k1) * W_N^(c*k1): the first factor is one scattered table read per ROW
    // (kept in the now free wsub), the second comes from the first T*N1 entries of the table -- cache resident --
    // instead of one scattered read per element.
    for (int m = threadIdx.x; m < N1; m += kThreads) wsub[m] = a.tw[(size_t)n2_0 * m];  // n2_0*m < N
    __syncthreads();
    double2* __restrict__ zt = Z + (size_t)batch * N1 * N2 + n2_0;   // (k1, c) of the tile sits at zt[k1*N2 + c]: 32-bit offsets
    for (int base = 0; base < total; base += kBatchLoads * kThreads) {
        double2 w2[kBatchLoads];
        int k1s[kBatchLoads], cs[kBatchLoads];
#pragma unroll
        for (int u = 0; u < kBatchLoads; ++u) {
            const int e = base + u * kThreads + threadIdx.x;
            const int k1 = fast_div(e, t_magic), c = e - k1 * T;
            const bool ok = e < total && n2_0 + c < N2;
            k1s[u] = ok ? k1 : -1;
            cs[u] = c;
            w2[u] = make_double2(1.0, 0.0);
            if (ok) w2[u] = a.tw[c * k1];
        }
#pragma unroll
        for (int u = 0; u < kBatchLoads; ++u) {
            if (k1s[u] >= 0) {
                double2 w = cmul(wsub[k1s[u]], w2[u]);
                if (INV) w.y = -w.y;
                zt[k1s[u] * N2 + cs[u]] = cmul(res[k1s[u] * pitch + cs[u]], w);
            }
        }
    }
}

// Kernel B: T adjacent rows k1 of one transform.  Dynamic LDS: 2 * N2*(T+1) + N2 double2.
template <bool INV, int STORE, int T, bool LOADSEL = false>
__global__ __launch_bounds__(kThreads) void fft4_rows_kernel(const PassArgs a, int N1, int N2, const Radices rad,
                                                             const double2* __restrict__ Z) {
    extern __shared__ double2 lds4[];
    constexpr int pitch = lds_pitch(T);
    double2* bufA = lds4;
    double2* bufB = bufA + N2 * pitch;
    double2* wsub = bufB + N2 * pitch;
    const int batch = blockIdx.y;
    const int k1_0 = blockIdx.x * T;
    const uint32_t n2_magic = div_magic(N2);
    const int total = N2 * T;
    // the T rows of a tile are ONE contiguous run of Z (row k1 of transform `batch` starts at (batch*N1 + k1)*N2):
    // element e of the tile sits at tile + e, no per-element 64-bit index arithmetic
    const double2* __restrict__ tile = Z + ((size_t)batch * N1 + k1_0) * N2;
    const int exist = (N1 - k1_0 < T ? N1 - k1_0 : T) * N2;    // elements of the tile that belong to the transform
    for (int base = 0; base < total; base += kBatchLoads * kThreads) {
        double2 z[kBatchLoads];
        int slot[kBatchLoads];
        double2 wv = make_double2(0.0, 0.0);
        static_assert(T >= kBatchLoads, "the twiddle table rides along with the element chunks");
        const int m = base / kBatchLoads + threadIdx.x;
        const bool wm = m < N2;
        if (wm) wv = a.tw[(size_t)m * N1];     // W_N2^m = W_N^(m*N1)
#pragma unroll
        for (int u = 0; u < kBatchLoads; ++u) {
            const int e = base + u * kThreads + threadIdx.x;
            const int c = fast_div(e, n2_magic), n2 = e - c * N2;  // n2 fastest: each row of Z is read as one contiguous run
            slot[u] = e < total ? n2 * pitch + c : -1;
            z[u] = make_double2(0.0, 0.0);
            if (e < exist) z[u] = tile[e];
        }
        if (wm) wsub[m] = wv;
#pragma unroll
        for (int u = 0; u < kBatchLoads; ++u)
            if (slot[u] >= 0) bufA[slot[u]] = z[u];
    }
    __syncthreads();
    const double2* res = lds_fft_auto<INV, T>(bufA, bufB, N2, rad, wsub);
    if constexpr (STORE == STORE_MAG_MAX) {
        // map[p][b][k] = |v|/N is never written: each lane keeps the largest value it produced (first index on
        // ties, as np.argmax over the row-major map), the wave reduces with DPP moves and lane 63 writes 16 bytes.
        // Inside a lane the candidates are ordered by the squared magnitude (3 instructions instead of a ~40
        // instruction hypot per point); hypot -- the reference's np.abs -- is monotone in it up to its rounding, so
        // only candidates within 2^-48 (relative) of the lane's best are compared through hypot itself, and the
        // lane's winner gets its exact hypot once, before lanes are compared.  With SECOND (the pass over the
        // winning row alone) the same maximum runs over the columns TwoCorrelationPeakComparison allows.
        const int prn = LOADSEL ? batch : batch / a.nbins;
        const int bin = LOADSEL ? 0 : batch - prn * a.nbins;
        int a1 = 0, b0 = 0, b1 = 0;                    // allowed columns [0,a1) U [b0,b1) (acquisition.py:98-111)
        if constexpr (LOADSEL) {
            const long long ti = a.tops[batch].i;
            const int code = (int)(ti - (ti / a.N) * a.N);
            const int e0 = code - a.spc, e1 = code + a.spc;
            if (e0 < 1) {
                b0 = e1;
                b1 = a.N - 1;
            } else if (e1 >= a.N) {
                a1 = e0;
            } else {
                a1 = e0;
                b0 = e1;
                b1 = a.N - 1;
            }
        }
        // A lane walks its elements e = k2*T + c in increasing order, and the map index bin*N + (k1_0 + c) + N1*k2 grows
        // with e: the first occurrence of a lane's maximum is simply the earliest e, so only the winner's index is ever
        // formed.  The coarse ordering uses the UNSCALED squared magnitude (the 1/N of the inverse transform is a
        // positive constant: it moves the ordering by rounding only, far inside the 2^-48 band that goes through the
        // exact comparison of the scaled hypot, the reference's np.abs).
        double best_sq = -1.0, best_x = 0.0, best_y = 0.0;
        int best_e = -1;
        for (int e = threadIdx.x; e < N2 * T; e += kThreads) {
            const int k2 = e / T, c = e - k2 * T;
            bool live = k1_0 + c < N1;
            if (LOADSEL) {
                const int col = k1_0 + c + N1 * k2;
                live = live && (col < a1 || (col >= b0 && col < b1));
            }
            if (live) {
                const double2 v = res[k2 * pitch + c];
                const double sq = v.x * v.x + v.y * v.y;
                bool take = sq > best_sq;
                if (__builtin_expect(fabs(sq - best_sq) <= best_sq * 0x1p-48, 0)) {
                    const double m_new = hypot(v.x * a.scale, v.y * a.scale), m_old = hypot(best_x * a.scale, best_y * a.scale);
                    take = m_new > m_old;      // (equal: the earlier element, i.e. the smaller index, stays)
                }
                best_sq = take ? sq : best_sq;
                best_x = take ? v.x : best_x;
                best_y = take ? v.y : best_y;
                best_e = take ? e : best_e;
            }
        }
        int best_i = 0x7fffffff;
        double best_v = -1.0;
        if (best_e >= 0) {
            const int k2 = best_e / T, c = best_e - k2 * T;
            best_i = bin * a.N + k1_0 + c + N1 * k2;
            best_v = 0.0 + hypot(best_x * a.scale, best_y * a.scale);   // (0.0 + |.|: the map's own rounding)
        }
        wave_best(best_v, best_i);
        if ((threadIdx.x & 63) == 63) {
            Best r = {best_v, (long long)best_i};
            a.partials[((size_t)batch * gridDim.x + blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6)] = r;
        }
        return;
    }
    // Output k1 + N1*k2 of row k1: a row of the tile holds every N1-th lag.  STORE_MAG_KEEP ends the walk behind the last k2 that
    // still has a lag below `cols` in the tile's first row (the rows after it reach `cols` no later): the discarded lags of
    // the tile are not read from LDS, and store_elem drops what the last kept k2 holds beyond `cols`.  Lanes walk c fastest,
    // so a wave's stores to one k2 are T adjacent doubles of a map row at either pitch.
    int k2_end = N2;
    if constexpr (STORE == STORE_MAG_KEEP) {
        const int left = a.cols - k1_0;                       // (k1_0 < N1 <= cols is not required: left <= 0 keeps nothing)
        k2_end = left <= 0 ? 0 : (left - 1) / N1 + 1;
        if (k2_end > N2) k2_end = N2;
    }
    for (int e = threadIdx.x; e < k2_end * T; e += kThreads) {
        const int k2 = e / T, c = e - k2 * T;
        const int k1 = k1_0 + c;
        if (k1 < N1) store_elem<STORE>(a, batch, k1 + N1 * k2, res[k2 * pitch + c]);
    }
}

// the entry points of the register-resident kernels: pcps_fast.h (N = 125 x 200), pcps_fastn.h (N = 20 / 50 / 250 x 200)
namespace fast25k {
inline void run_cols(PassArgs& a, int batch, double2* Z, hipStream_t stream);
inline void run(sdr_engine* e, PassArgs a, int batch, double2* Z, hipStream_t stream);
}  // namespace fast25k
namespace fastn {
template <int N1, int STORE>
inline void run_rows(const PassArgs& a, int batch, const double2* Z, hipStream_t stream);
template <int STORE>
inline void run(int N, PassArgs a, int batch, double2* Z, hipStream_t stream);
}  // namespace fastn

template <bool INV, int LOAD0, int STORE_LAST, int FMT, int TA, int TB>
void run_four_step_t(sdr_engine* e, const FourStep& f, PassArgs a, int batch, double2* Z, double2* final_out) {
    a.out = final_out;
    const size_t shA = (size_t)(2 * f.N1 * lds_pitch(TA) + f.N1) * sizeof(double2);
    const size_t shB = (size_t)(2 * f.N2 * lds_pitch(TB) + f.N2) * sizeof(double2);
    // more than 64 KiB of dynamic LDS has to be requested explicitly (160 KiB per CU on MI355X)
    (void)hipFuncSetAttribute((const void*)fft4_cols_kernel<INV, LOAD0, FMT, TA>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shA);
    constexpr bool SEL = LOAD0 == LOAD_MUL_CODE_SEL;
    (void)hipFuncSetAttribute((const void*)fft4_rows_kernel<INV, STORE_LAST, TB, SEL>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shB);
    dim3 gridA((f.N2 + TA - 1) / TA, batch);
    if constexpr (LOAD0 == LOAD_MUL_CODE) {             // 1-D, XCD-aware: 8 x the largest eighth of the (tile, bin) pairs x PRNs
        const int pairs = (int)gridA.x * a.nbins;
        a.n_prn = batch / a.nbins;
        gridA = dim3(8u * (unsigned)((pairs + 7) / 8) * (unsigned)a.n_prn, 1);
    }
    hipLaunchKernelGGL((fft4_cols_kernel<INV, LOAD0, FMT, TA>), gridA, dim3(kThreads), shA, e->stream, a, f.N1, f.N2, f.rad1, Z);
    hipLaunchKernelGGL((fft4_rows_kernel<INV, STORE_LAST, TB, SEL>), dim3((f.N1 + TB - 1) / TB, batch), dim3(kThreads), shB,
                       e->stream, a, f.N1, f.N2, f.rad2, Z);
}

template <int STORE = STORE_MAG_MAX>
inline void fast_run(sdr_engine* e, const Xform& t, PassArgs a, int batch, double2* Z, hipStream_t stream) {
    if (t.fast == FAST_25K) {
        if constexpr (STORE == STORE_MAG_MAX) {
            fast25k::run(e, a, batch, Z, stream);
        } else {
            fast25k::run_cols(a, batch, Z, stream);
            fastn::run_rows<pcps::fast25k::N1, STORE>(a, batch, Z, stream);
        }
    } else {
        fastn::run<STORE>(t.four.N1 * t.four.N2, a, batch, Z, stream);
    }
}
template <bool INV, int LOAD0, int STORE_LAST, int FMT>
void run_four_step(sdr_engine* e, const Xform& t, PassArgs a, int batch, double2* Z, double2* final_out) {
    if constexpr (INV && LOAD0 == LOAD_MUL_CODE &&
                  (STORE_LAST == STORE_MAG_MAX || STORE_LAST == STORE_MAG_ACC || STORE_LAST == STORE_CPLX_ACC)) {
        if (t.fast) {         // the inverse transforms of a search at 4 / 10 / 25 / 50 MHz
            fast_run<STORE_LAST>(e, t, a, batch, Z, e->stream);
            return;
        }
    }
    if constexpr (!INV && LOAD0 == LOAD_IQ_MIX && STORE_LAST == STORE_PLAIN) {
        // a handful of forward transforms (shared spectra: four for a 250 Hz grid) are a chain of latencies, not work: narrower
        // column tiles put twice as many workgroups on its first half
        if (batch <= 8) {           // (measured: 0.2179 -> 0.2159 ms per 32-PRN call at 25 MHz, 0.4863 -> 0.4833 at 50 MHz)
            run_four_step_t<INV, LOAD0, STORE_LAST, FMT, 4, 4>(e, t.four, a, batch, Z, final_out);
            return;
        }
    }
    run_four_step_t<INV, LOAD0, STORE_LAST, FMT, SDR_PCPS_COL_TILE, kRowTile>(e, t.four, a, batch, Z, final_out);
}

/* ------------------------------------------------------------------------------------------------
 * Chirp-z (Bluestein) transform for a length N the planner cannot factor (a prime factor above 64):
 * what NumPy's pocketfft does for such sizes.  With c[m] = exp(+i*pi*m^2/N) (m^2 taken mod 2N in
 * integers, so the phase is exact to an ulp):
 *   forward  X[k] = conj(c[k]) * sum_n (x[n] conj(c[n])) * c[k-n]
 *   inverse  Y[n] =      c[n]  * sum_k (X[k]      c[k] ) * conj(c[n-k])          (unnormalised)
 * The sums are circular convolutions of length M >= 2N-1 (M = 2^a 3^b 5^c), done with the ordinary
 * transforms above.  The fused loads / stores of the PCPS stages sit in the pre / post kernels.
 * ------------------------------------------------------------------------------------------------ */
struct BluPlan {
    int N = 0, M = 0;
    const double2* chirp = nullptr;   // [N]
    const double2* spec_fwd = nullptr;  // FFT_M of the forward kernel, [M]
    const double2* spec_inv = nullptr;  // FFT_M of the inverse kernel, [M]
    const double2* twM = nullptr;     // twiddles of the length-M transform
    double2 *x = nullptr, *a = nullptr, *b = nullptr;  // [max batch][M] work buffers
    const Xform* xm = nullptr;        // the length-M transform
};

__global__ __launch_bounds__(kThreads) void blu_chirp_kernel(double2* chirp, double2* kern_fwd, double2* kern_inv, int N, int M) {
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    double2 c = make_double2(0.0, 0.0);
    const int d = m < N ? m : (M - m < N ? M - m : -1);  // kernel index: b[m] = c[|m|] for |m| < N (wrapped), else 0
    if (d >= 0) {
        const long long r = ((long long)d * d) % (2LL * N);
        double sn, cs;
        sincospi((double)r / (double)N, &sn, &cs);
        c = make_double2(cs, sn);
    }
    if (m < N) chirp[m] = c;
    kern_fwd[m] = c;
    kern_inv[m] = make_double2(c.x, -c.y);
}

template <int LOAD, int FMT, bool INV>
__global__ __launch_bounds__(kThreads) void blu_pre_kernel(const PassArgs a, const double2* __restrict__ chirp, int M,
                                                          double2* __restrict__ x) {
    const int m = blockIdx.x * kThreads + threadIdx.x;
    const int batch = blockIdx.y;
    if (m >= M) return;
    double2 v = make_double2(0.0, 0.0);
    if (m < a.N) {
        double2 c = chirp[m];
        if (!INV) c.y = -c.y;
        v = cmul(load_elem<LOAD, FMT, INV>(a, batch, m), c);
    }
    x[(size_t)batch * M + m] = v;
}

__global__ __launch_bounds__(kThreads) void blu_mul_kernel(double2* __restrict__ x, const double2* __restrict__ spec, int M) {
    const int m = blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    const size_t o = (size_t)blockIdx.y * M + m;
    x[o] = cmul(x[o], spec[m]);
}

template <int STORE, bool INV>
__global__ __launch_bounds__(kThreads) void blu_post_kernel(const PassArgs a, const double2* __restrict__ chirp, int M,
                                                           const double2* __restrict__ x) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    const int batch = blockIdx.y;
    if (k >= a.N) return;
    if (STORE == STORE_MAG_KEEP && k >= a.cols) return;
    double2 c = chirp[k];
    if (!INV) c.y = -c.y;
    const double inv_m = 1.0 / (double)M;
    double2 v = cmul(x[(size_t)batch * M + k], c);
    v.x *= inv_m;
    v.y *= inv_m;
    store_elem<STORE>(a, batch, k, v);
}

// Runs all passes of one batched transform.  `first` carries the fused load of
// pass 0, `last_store` the fused store of the final pass.  Ping-pongs bufA/bufB.
template <bool INV, int LOAD0, int STORE_LAST, int FMT>
void run_fft(sdr_engine* e, const Xform& t, PassArgs a, int batch, double2* bufA, double2* bufB, double2* final_out,
             const char* prof_name, const BluPlan* blu = nullptr);

template <bool INV, int LOAD0, int STORE_LAST, int FMT>
void run_bluestein(sdr_engine* e, const BluPlan& blu, PassArgs a, int batch, double2* final_out) {
    a.out = final_out;
    const int M = blu.M;
    const int n_out = STORE_LAST == STORE_MAG_KEEP ? a.cols : a.N;      // (outputs the post kernel keeps)
    const dim3 gm((M + kThreads - 1) / kThreads, batch), gn((n_out + kThreads - 1) / kThreads, batch);
    hipLaunchKernelGGL((blu_pre_kernel<LOAD0, FMT, INV>), gm, dim3(kThreads), 0, e->stream, a, blu.chirp, M, blu.x);
    PassArgs p = {};
    p.N = M;
    p.tw = blu.twM;
    p.in = blu.x;
    run_fft<false, LOAD_PLAIN, STORE_PLAIN, FMT>(e, *blu.xm, p, batch, blu.a, blu.b, blu.x, "pcps_bluestein_fft");
    hipLaunchKernelGGL(blu_mul_kernel, gm, dim3(kThreads), 0, e->stream, blu.x, INV ? blu.spec_inv : blu.spec_fwd, M);
    run_fft<true, LOAD_PLAIN, STORE_PLAIN, FMT>(e, *blu.xm, p, batch, blu.a, blu.b, blu.x, "pcps_bluestein_fft");
    hipLaunchKernelGGL((blu_post_kernel<STORE_LAST, INV>), gn, dim3(kThreads), 0, e->stream, a, blu.chirp, M, blu.x);
}

template <bool INV, int LOAD0, int STORE_LAST, int FMT>
void run_fft(sdr_engine* e, const Xform& t, PassArgs a, int batch, double2* bufA, double2* bufB, double2* final_out,
             const char* prof_name, const BluPlan* blu) {
    ProfScope ps(e, prof_name);
    if (blu) {
        run_bluestein<INV, LOAD0, STORE_LAST, FMT>(e, *blu, a, batch, final_out);
        return;
    }
    if (t.four.ok) {
        run_four_step<INV, LOAD0, STORE_LAST, FMT>(e, t, a, batch, bufA, final_out);
        return;
    }
    const std::vector<int>& radices = t.radices;
    const int np = (int)radices.size();
    int Ns = 1;
    const double2* src = a.in;
    for (int p = 0; p < np; ++p) {
        a.R = radices[p];
        a.Ns = Ns;
        a.nbf = a.N / a.R;
        a.tw_stride = a.N / (Ns * a.R);
        const bool first = p == 0, last = p == np - 1;
        a.in = first ? a.in : src;
        double2* dst = last ? final_out : ((p & 1) ? bufB : bufA);
        a.out = dst;
        if (first && last) launch_pass<INV, LOAD0, STORE_LAST, FMT>(e, a, batch);
        else if (first) launch_pass<INV, LOAD0, STORE_PLAIN, FMT>(e, a, batch);
        else if (last) launch_pass<INV, LOAD_PLAIN, STORE_LAST, FMT>(e, a, batch);
        else launch_pass<INV, LOAD_PLAIN, STORE_PLAIN, FMT>(e, a, batch);
        src = dst;
        Ns *= a.R;
    }
}

}  // namespace
