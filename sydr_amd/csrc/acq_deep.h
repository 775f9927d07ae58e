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
