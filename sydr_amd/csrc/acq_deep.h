// The two kernels of the deep search (sdr_acq_deep, include/sydr_amd.h) that are not transforms: acq_deep.hip.  The route
// itself -- the transforms between them, the code spectra, the peaks -- is pcps.hip's run_deep.
#pragma once

#include "engine_internal.h"

// F[b][n] = sum_{c < coh} x[first + c*N + n] * exp(-1j * (if_hz - bin_b) * (((c*N + n) * 2) * pi / fs)),  b < nbins, n < N:
// one coherent block of coh code periods, mixed per Doppler bin and folded onto one period.  F = [nbins][N] double2.
int sdr_deep_fold(sdr_engine* e, int64_t first, int N, int coh, int nbins, double fs, double if_hz, double bin_start,
                  double bin_delta, void* F);
// map row (p, g, b) (+)= mag row (p, b) read q[b] samples on: map[((p*groups + g)*nbins + b)*N + n] (+)= mag[(p*nbins + b)*N +
// (n + q[b]) % N], 0 <= q[b] < N on the device; `store`: the group's first block (0.0 + mag, as the map routes of sdr_pcps).
int sdr_deep_shift_acc(sdr_engine* e, const double* mag, double* map, const int32_t* q, int n_prn, int nbins, int N, int groups,
                       int g, int store);

// sdr_acq_deep_detect's passes over the resident maps (acq_detect.hip): the further peaks and the noise cells' moments.
struct DeepDetectPeak {      // a peak as the kernels leave it: row = group * nbins + bin, -1 where no cell was left
    int32_t row, code;
    double value;
};
struct DeepDetectWs {        // the work space of one call, cut from one buffer of sdr_deep_detect_bytes()
    DeepDetectPeak* peaks;   // [n_prn][8]
    sdr_detect_noise* noise; // [n_prn]
    void* parts;             // the partial results of a pass
};
size_t sdr_deep_detect_bytes(int n_prn, int rows, int N);
DeepDetectWs sdr_deep_detect_ws(void* buf, int n_prn);
// map = [n_prn][rows][N] with rows = groups * nbins; (row0, code0, value0)[n_prn]: peak 0 as the peak kernels of the search
// left it in device memory.  Everything is queued on the engine's stream; nothing comes back to the host.
int sdr_deep_detect(sdr_engine* e, const double* map, int n_prn, int rows, int nbins, int N, const sdr_detect_cfg* det,
                    const long long* row0, const long long* code0, const double* value0, const DeepDetectWs& ws);
