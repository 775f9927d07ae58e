// The in-LDS radix-2 fp64 transform of 64..4096 points that sdr_iq_probe's Welch kernel (probe.hip) and the excisor
// (mitigate.hip) share: its tables, the decimation-in-frequency forward pass and the decimation-in-time inverse that takes
// the forward pass's bit-reversed spectrum straight back to natural order.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace sdr {

constexpr int kFftLdsMin = 64, kFftLdsMax = 4096;

// host[0 .. nfft): exp(-2j*pi*k/nfft), k < nfft / 2, interleaved; host[nfft .. 2 nfft): the periodic Hann window.
// Returns the sum of the window's squares.
inline double fft_lds_fill_tables(int nfft, double* host) {
    for (int k = 0; k < nfft / 2; ++k) {
        const double a = 2.0 * M_PI * (double)k / (double)nfft;
        host[2 * k] = std::cos(a);
        host[2 * k + 1] = -std::sin(a);
    }
    double sumw2 = 0.0;
    for (int j = 0; j < nfft; ++j) {
        const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)j / (double)nfft);
        host[nfft + j] = w;
        sumw2 += w * w;
    }
    return sumw2;
}

#if defined(__HIPCC__)
// Decimation in frequency, in place, by the whole workgroup of THREADS lanes: X[k] ends at position bitrev(k).  The caller
// has a barrier behind its writes of x; the pass ends with one.
template <int THREADS>
__device__ __forceinline__ void fft_lds_forward(double2* x, int nfft, const double2* __restrict__ tw, int tid) {
    const int half = nfft >> 1;
#pragma unroll 1
    for (int h = half, step = 1; h >= 1; h >>= 1, step <<= 1) {
        for (int t = tid; t < half; t += THREADS) {
            const int k = t & (h - 1);
            const int i = ((t - k) << 1) + k;
            const double2 a = x[i], b = x[i + h];
            const double2 w = tw[k * step];
            const double dr = a.x - b.x, di = a.y - b.y;
            x[i] = make_double2(a.x + b.x, a.y + b.y);
            x[i + h] = make_double2(__builtin_fma(-di, w.y, dr * w.x), __builtin_fma(di, w.x, dr * w.y));
        }
        __syncthreads();
    }
}

// Its inverse without the 1 / nfft: decimation in time from the spectrum at bit-reversed positions to the sequence in
// natural order, the conjugate twiddles of the same table.  Same barriers.
template <int THREADS>
__device__ __forceinline__ void fft_lds_inverse(double2* x, int nfft, const double2* __restrict__ tw, int tid) {
    const int half = nfft >> 1;
#pragma unroll 1
    for (int h = 1, step = half; h <= half; h <<= 1, step >>= 1) {
        for (int t = tid; t < half; t += THREADS) {
            const int k = t & (h - 1);
            const int i = ((t - k) << 1) + k;
            const double2 a = x[i], b = x[i + h];
            const double2 w = tw[k * step];
            const double br = __builtin_fma(b.y, w.y, b.x * w.x), bi = __builtin_fma(-b.x, w.y, b.y * w.x);   // b * conj(w)
            x[i] = make_double2(a.x + br, a.y + bi);
            x[i + h] = make_double2(a.x - br, a.y - bi);
        }
        __syncthreads();
    }
}
#endif

}  // namespace sdr
