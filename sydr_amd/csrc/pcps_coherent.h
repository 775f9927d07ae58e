// The kernels of the coherent search (sdr_pcps_coherent, include/sydr_amd.h) that are not transforms: pcps_coherent.hip.  The
// route itself -- the transforms in front of them, the code spectra, the chunks, the peaks -- is pcps.hip's run_coherent.
#pragma once

#include "coherent_request.h"
#include "engine_internal.h"

// What the three kernels share of one call.
struct CohGeom {
    int N = 0, T = 0, M = 0, Ls = 0, K = 0, mode = 0, nbins = 0;
    double fs = 0.0, if_hz = 0.0, bin_start = 0.0, bin_delta = 0.0, step_hz = 0.0;
    const int8_t* sec = nullptr;         // device: [n_sec][Ls]
    const int32_t* sec_rows = nullptr;   // device: [n_prn]
};

// R of a chunk's units: map[((prn0 + pl) * nbins + bin0 + bl) * N + tau] = sqrt(max_{h,k} P), from the chunk's per-period
// correlations C = [M][units][T] (unit pl * bins + bl).
int sdr_coh_combine(sdr_engine* e, const CohGeom& g, const sdr::CohChunk& c, const void* C, double* map);
// Behind the combine of a chunk: where a PRN's largest R so far lies in this chunk (parts: argmax_part_kernel's records over the
// chunk's rows of each of its PRNs, indices from the chunk's first bin on), its M per-period correlations are kept --
// keep[p][m] -- and the running record best[p] (16 bytes: value, flat index in the PRN's map) is raised.  (value, then the
// lower index) is a total order, so what is kept at the end is the column of the map's first maximum, whatever the cut.
int sdr_coh_keep(sdr_engine* e, const CohGeom& g, const sdr::CohChunk& c, const void* C, const void* parts, void* best, void* keep);
// The pick at the peak cell of every PRN: P[h][k] from keep[p][.] with the bin peak_bin[p] gives -> results[p] (every field),
// power[p][Ls][K].  peak_bin / peak_code / peak_ratio: the peak kernels' results in device memory, map: R.
int sdr_coh_pick(sdr_engine* e, const CohGeom& g, int n_prn, const void* keep, const double* map, const long long* peak_bin,
                 const long long* peak_code, const double* peak_ratio, sdr_coh_result* results, double* power);
