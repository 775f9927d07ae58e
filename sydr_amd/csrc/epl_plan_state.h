// What an E/P/L plan holds: made, fetched and destroyed by epl_plan.hip, run by epl.hip.
#pragma once

#include <utility>
#include <vector>

#include "engine_internal.h"

struct sdr_epl_plan {
    sdr_epl_item* d_items = nullptr;
    double* d_out = nullptr;
    double* d_spacing = nullptr;
    char* d_setups = nullptr;   // straight-line kernels: one ChipSetup<n_taps> / ChipNSetup per item (correlator_chip.h, correlator_chip2.h)
    size_t setup_bytes = 0;     // sizeof(ChipSetup<n_taps>), 0: none
    size_t bytes_items = 0, bytes_out = 0, bytes_spacing = 0, bytes_setups = 0;   // what the four allocations hold (plan_give)
    int n_items = 0;
    int n_taps = 0;
    int lut_words = 0;
    int wide = 0;  // 16 / 8: every item has 16 (8) * code_step < 1, the boundary variant with that group width applies
    int group_stride = 0;  // C > 0: items[i] and items[i + C] use the same code slot for every i (epoch-major lists of C channels)
    bool borrowed = false;  // device buffers are the engine's workspaces (sdr_epl_batch): not freed with the plan
    bool doubled = false;  // the plan runs on the half-chip view: its device items / spacings carry 2*rem_code, 2*code_step, 2*spacing
    double fs = 0.0;
    int64_t code_generation = 0;  // of the engine's code tables the plan was validated against
    int64_t ring_capacity = 0;    // and of the ring
    // one event per stream a range of the plan was launched on, re-recorded behind every launch: fetch waits for
    // exactly these instead of the whole device
    std::vector<std::pair<hipStream_t, hipEvent_t>> ran_on;
    // a long list's setups are made on the engine's plan_stream after creation has returned: recorded behind them, waited
    // for on the device by every launch and fetch and by the host in destroy (nullptr: the setups were done when creation returned)
    hipEvent_t ready = nullptr;
    // work of the plan may be pending on the engine's own stream: a creation that ended on an error path or did all its work
    // there, a range run on stream id 0.  Destroy then waits for that stream as well.
    bool engine_stream_work = true;
};

// epl.hip: the half-chip view of the staged replicas is up to date (made on the engine's stream; `stream`: the one that will
// read it -- waited for, where that is another).
int sdr_epl_ensure_doubled_luts(sdr_engine* e, hipStream_t stream);
