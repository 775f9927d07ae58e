/*
 * sydr_amd.h -- C-ABI of the MI355X (gfx950) GNSS correlator engine.
 *
 * This is the drop-in boundary for the one hot path of aproposorg/sydr:
 * PCPS acquisition, the E/P/L tracking correlators and PRN replica
 * generation.  It supersedes the reference's legacy native layer
 * (sydr/c_functions/tracking.c, acquisition.c, loaded through ctypes by
 * sydr/old/tracking/tracking_epl_c.py:31 and
 * sydr/old/acquisition/acquisition_pcps_c.py:32) and is what the live NumPy
 * hot path (sydr/dsp/acquisition.py:9-115, sydr/dsp/tracking.py:92-116,
 * sydr/signal/gnsssignal.py:9-58) is replaced with.
 *
 * Conventions (kept from the reference's ctypes layer):
 *   - plain C linkage, plain pointers and sizes, caller allocates every output;
 *   - complex numbers are interleaved (re, im);
 *   - 2-D arrays are C-contiguous row-major;
 *   - the library keeps no caller pointer after a call returns.
 * Added over the reference (which returned void and had no error path):
 *   - every call returns 0 or a negative sdr_status, text via sdr_last_error();
 *   - one opaque engine per GPU; calls on one engine are serialised by the caller.
 *
 * All arithmetic that decides an INTEGER result (code-chip index, peak
 * indices) is IEEE fp64 in the reference's operation order.
 */
#ifndef SYDR_AMD_H
#define SYDR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: what this header declares -- and nothing else -- is in its dynamic
 * symbol table (sydr/c_functions/Makefile:1-12: one .so, only the bound symbols matter); tests/test_abi.py holds
 * `nm -D --defined-only` against these declarations. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SDR_ABI_VERSION 5   /* 5 (still): + sdr_pcps_coherent, sdr_coh_cfg / _result, option "coherent_scratch_kb" (additive); 5 (still): + sdr_pcps_signal, sdr_acq_signal (additive); 5 (still): + sdr_acq_deep_detect, sdr_detect_cfg / _peak / _noise (additive); 5 (still): + sdr_iq_cancel, sdr_cancel_stats (additive); 5 (still): + sdr_acq_deep, sdr_acq_deep_shift (additive); 5 (still): + sdr_ddc_cfg, sdr_ddc_create / _destroy / _reset / _push / _push_queue / _out_count (additive); 5 (still): + sdr_iq_probe (additive); 5 (still): + sdr_corr_profile, option "corr_profile_per_sample" (additive); 5 (still): + sdr_iq_packing, sdr_iq_packed_bytes, sdr_iq_upload_packed / _begin / _queue (additive); 5 (still): + sdr_acq_refine, sdr_acq_refine_bins (additive); 5: + sdr_bank_tick_mirrored_begin / _end, sdr_iq_upload_queue, sdr_host_alloc / _free, options "tick_server" + sdr_tick_server_stats, "bind_thread_to_device" (additive); 4: + sdr_build_id, sdr_epl_plan_create_dev, sdr_bank_tick_mirrored, sdr_iq_upload_begin, sdr_block_schedule, sdr_bank_step_begin / _end (additive) */

typedef struct sdr_engine sdr_engine;

enum sdr_status {
    SDR_OK = 0,
    SDR_ERR_INVALID = -1,     /* bad argument                                   */
    SDR_ERR_HIP = -2,         /* a HIP runtime call failed (text has the cause) */
    SDR_ERR_NOMEM = -3,       /* host or device allocation failed               */
    SDR_ERR_UNSUPPORTED = -4, /* size / format not supported by the kernels     */
    SDR_ERR_RANGE = -5,       /* request reaches outside the IQ ring / code LUT */
    SDR_ERR_STATE = -6        /* call made before the state it needs exists     */
};

/* IQ sample formats held in HBM.  ci8 is the reference's file format
 * (sydr/signal/rfsignal.py:36-37,127-130: interleaved int8 I,Q). */
enum sdr_iq_format {
    SDR_FMT_CI8 = 0,  /* int8  I, int8  Q  (2 B / sample) */
    SDR_FMT_CI16 = 1, /* int16 I, int16 Q  (4 B / sample) */
    SDR_FMT_CF32 = 2, /* float I, float Q  (8 B / sample) */
    SDR_FMT_CF64 = 3  /* double I, double Q (16 B / sample) = numpy complex128 */
};

#define SDR_MAX_TAPS 8
#define SDR_GPS_L1CA_CHIPS 1023

/* ---------------------------------------------------------------- library */
const char* sdr_last_error(void);
int sdr_abi_version(void);
/* First 16 hex digits of the SHA-256 over the library's sources as they were when it was built (the .hip / .h files of
 * sydr_amd/csrc in name order, then this header): what a profile or a counter file names as the build it was taken on. */
const char* sdr_build_id(void);
/* Number of visible GPUs (0 on a CPU-only host; never an error there). */
int sdr_device_count(int* n);

/* ----------------------------------------------------------------- engine */
int sdr_engine_create(int device_id, sdr_engine** out);
void sdr_engine_destroy(sdr_engine* e);
/* Wait for everything queued on the engine's stream, and for the setups of every E/P/L plan made so far. */
int sdr_engine_sync(sdr_engine* e);
/* HIP-event timing.  enable=1 brackets every stage of a call (named scopes: "epl_kernel", "pcps_fwd_fft", ...) with
 * hipEvents on the launch stream; enable=2 brackets each whole call instead ("call_pcps": one event pair around
 * everything sdr_pcps launches -- the per-stage pairs each cost the stream a few microseconds); sdr_prof_read drains
 * them (it syncs).  While either is on, sdr_pcps keeps to one stream. */
int sdr_prof_enable(sdr_engine* e, int enable);
/* Sum/count of launch durations of kernels whose name starts with `prefix`
 * ("" = all) since the last sdr_prof_reset. */
int sdr_prof_read(sdr_engine* e, const char* prefix, double* total_ms, int64_t* launches);
int sdr_prof_reset(sdr_engine* e);

/* Diagnostic switches (tests, A/B timing): "pcps_materialise_map" = 1 writes the whole correlation map even when the
 * caller asks for indices and ratio only; "pcps_general_kernels" = 1 keeps the general four-step kernels where the
 * register-resident 125 x 200 ones would run; "pcps_prn_chunk" = n searches n PRNs per inverse sweep; "pcps_one_stream" = 1
 * keeps the sweeps of a map-free search on one stream;
 * "pcps_fused" = 0 keeps a map-free search at 25 MHz on the two-kernel sweeps where one launch of persistent workgroups, one
 * (PRN, bin) transform per workgroup, would run (256 transforms or more); "pcps_no_spectra_cache" = 1
 * recomputes conj(fft(code)) in every search, as the reference does (channel_l1ca_kaplan.py:184-185), instead of keeping
 * the spectra of the staged codes; "ingest_by_copy_command" = 1 moves the slabs of sdr_iq_upload_begin / sdr_bank_tick
 * into the ring with a copy command instead of the ingest kernel (a packed slab of sdr_iq_upload_packed_begin: into HBM with
 * a copy command, its unpack kernel then reads no host memory); "track_one_launch_tick" = 1 runs a one-epoch step
 * (sdr_bank_tick*, sdr_bank_step with n_epochs = 1) as one workgroup per channel instead of on the cluster a block of
 * epochs would use (other order of additions); "track_two_launch_tick" = 1 runs that cluster's one-epoch step as two
 * launches cut at the exchange of the parts' sums instead of one (the part that draws its channel's last ticket
 * collects: same bits); "ingest_with_tick" = 0 gives the slab of sdr_iq_upload_begin a launch of its own again instead of
 * workgroups of the tick's launch; "pcps_no_shared_spectra" = 1 transforms the Doppler-mixed millisecond once per bin
 * even where bins a whole number of FFT bins apart could share a spectrum; "epl_no_chip_variant",
 * "epl_no_split_variant", "epl_no_half_chip_view" = 1 keep the E/P/L correlator from its chip-aligned core, from the
 * kernel with the tap switch positions compiled in, from the half-chip view of 32-52 samples per chip;
 * "epl_xcd_run" = R (0 .. 65536) lets each of the device's 8 XCDs take runs of R consecutive items of an E/P/L launch, so
 * that the channel-epochs of one millisecond of an epoch-major list read the ring through one L2 (0: the workgroups take the
 * items in linear order, dealt round-robin to the XCDs; -1: the library's default, 64); plans read it when they run; outputs are the same bits.  Integer
 * results do not depend on any of them, floating ones to rounding. */
int sdr_set_option(sdr_engine* e, const char* name, int value);

/* Measured HBM copy rate of THIS GPU: a hand-written 16-byte-per-lane grid-stride copy kernel moves n_bytes
 * from one buffer to another `reps` times; *gbps = (bytes read + bytes written) / time.  The second denominator
 * beside the 8 TB/s datasheet peak; no counterpart in the reference. */
int sdr_hbm_copy_rate(sdr_engine* e, int64_t n_bytes, int reps, double* gbps);

/* ---------------------------------------------------------------- IQ ring
 * Replaces the host shm ring (sydr/channel/channelManager.py:57-61,
 * sydr/utils/circularbuffer.py:21-137): capacity_samples slots in HBM,
 * addressed modulo capacity.  capacity must be a multiple of 8 samples. */
int sdr_iq_alloc(sdr_engine* e, int64_t capacity_samples, int fmt);
/* Copy n_samples host samples (in the ring's format) to ring_offset.. ,
 * wrapping at the end of the ring (CircularBuffer.shift, circularbuffer.py:54-82). */
int sdr_iq_upload(sdr_engine* e, const void* iq, int64_t n_samples, int64_t ring_offset);
/* Copy ring samples back to the host in the ring's format (tests / oracle).  Synchronises the engine's stream;
 * a ci8 ring holds its bytes sign-flipped, and the call flips them back on the host. */
int sdr_iq_download(sdr_engine* e, void* iq, int64_t n_samples, int64_t ring_offset);

/* Synthetic multi-satellite IQ written straight into the ring:
 *   x[n] = sum_s amp * c_s(chip_s(n)) * d_s(n) * exp(j*2*pi*(doppler_s*n/fs + phase_s)) + CN(0, sigma^2)
 * for ring sample numbers n = first_sample .. first_sample + n_samples - 1, each written to slot n mod capacity
 * (n_samples <= capacity; first_sample >= 0 may lie beyond the capacity).  One float32 value per component:
 * integer rings hold it rounded to even and clipped to +-127 / +-32767 (never -128 / -32768), float rings
 * hold the float32 value (a cf64 ring the same value widened).  chip_s(n) =
 * code_phase_s + n * 1.023e6*(1+doppler_s/1575.42e6)/fs (chips, modulo the code's length L: 1023 for a GPS
 * PRN, the staged length of a code slot; code_phase_s may be negative); with SDR_SYNTH_BOC11 the sign flips
 * in the second half of every chip.  d_s is a seeded +-1 sequence that changes every 20 code periods when
 * L == 1023 and every code period otherwise, keyed by the PRN number, or by slot + 1000 for a staged code
 * (so PRN p and slot p carry different data).  The noise is Box-Muller from 24-bit uniforms: its radius stops
 * at sqrt(2 ln 2^24) = 5.77 sigma.  Deterministic in (seed, n): a stream written in several calls is the
 * stream written in one.  The statement in NumPy: tests/synth_cases.py; docs/notes/synth.md. */
#define SDR_SYNTH_CODE_SLOT 1 /* `prn` is a staged code slot (any length), not a GPS PRN number      */
#define SDR_SYNTH_BOC11 2     /* multiply by the BOC(1,1) square sub-carrier (flip every half chip)  */
typedef struct sdr_synth_sat {
    int32_t prn;        /* GPS PRN 1..210, or a code slot with SDR_SYNTH_CODE_SLOT */
    int32_t flags;
    double doppler_hz;  /* carrier Doppler                             */
    double code_phase;  /* chips into the code at ring sample 0        */
    double carrier_phase; /* cycles at ring sample 0                   */
    double amplitude;   /* per-axis amplitude in LSB                   */
} sdr_synth_sat;
int sdr_iq_synth(sdr_engine* e, const sdr_synth_sat* sats, int n_sats, double fs,
                 double noise_sigma, uint64_t seed, int64_t first_sample, int64_t n_samples);

/* ------------------------------------------------------------ PRN replicas
 * Code slots are device-resident +-1 chip tables staged for the correlators.
 * sdr_code_gps_l1ca generates the C/A Gold code ON DEVICE (G1/G2 LFSRs, G2
 * delay table) and replaces GenerateGPSGoldCode (sydr/signal/gnsssignal.py:9-31
 * -> sydr/signal/ca.py:70-112; chip mapping bit 1 -> +1, bit 0 -> -1). */
int sdr_code_slots(sdr_engine* e, int n_slots, int max_chips);
/* Same, with the replicas staged over max_periods code periods so that one correlator epoch may span
 * several periods (e.g. 4 ms of C/A code) or taps may sit many chips out; chips*periods <= 32768. */
int sdr_code_slots_ex(sdr_engine* e, int n_slots, int max_chips, int max_periods);
int sdr_code_gps_l1ca(sdr_engine* e, int slot, int prn);
/* Stage an arbitrary +-1 code (e.g. a synthetic 4092-chip E1-like code). */
int sdr_code_custom(sdr_engine* e, int slot, const int8_t* chips, int n_chips);
/* Read a staged code back: out_chips[n_chips] in {-1,+1}. */
int sdr_code_read(sdr_engine* e, int slot, int8_t* out_chips, int max_chips, int* n_chips);
/* UpsampleCode (sydr/signal/gnsssignal.py:35-58): out[k] = code[trunc((ts*k)/tc)],
 * k < n_samples = round(fs/1000) for GPS L1 C/A; computed on device. */
int sdr_code_upsample(sdr_engine* e, int slot, double fs, int64_t n_samples, int8_t* out);

/* ------------------------------------------------ E/P/L tracking correlators
 * One item = one call of EPL (sydr/dsp/tracking.py:92-116) = one channel-epoch:
 *   replica_i = exp(1j*(-(carrier_hz*2.0*pi*(i/fs)) + rem_carrier)),  i = 0..n-1
 *   idx_i     = ceil(linspace(rem_code+spacing, code_step*n+rem_code+spacing, n, endpoint=False))
 *   I_tap, Q_tap = sum code[idx_i]*Re/Im(replica_i*x_i)
 * with code the padded table [c[L-1], c[0..L-1], c[0]] (channel_l1ca_kaplan.py:104-107),
 * extended periodically here so that any tap spacing can be served. */
typedef struct sdr_epl_item {
    int32_t code_slot;    /* staged PRN replica                                   */
    int32_t n_samples;    /* samples in this epoch (track_requiredSamples)        */
    int64_t start_sample; /* ring index of the first sample (currentSample)       */
    double carrier_hz;    /* carrierFrequency                                     */
    double rem_carrier;   /* remainingCarrier [rad]                               */
    double rem_code;      /* remainingCode [chips]                                */
    double code_step;     /* codeStep [chips/sample]                              */
} sdr_epl_item;

/* Synchronous convenience call: out[n_items][2*n_taps] = I,Q per tap, in tap order
 * (the reference's [IE,QE,IP,QP,IL,QL] for taps (-0.5,0,0.5)). */
int sdr_epl_batch(sdr_engine* e, const sdr_epl_item* items, int n_items, const double* spacing,
                  int n_taps, double fs, double* out);

/* Resident plans: items and outputs stay in HBM so a timed region holds only
 * kernel launches.  run is asynchronous on the engine stream.
 * Creating a plan checks every item against the ring and the staged replicas (host), uploads the list and, for lists the
 * straight-line kernels serve (ci8 ring; 24-25 samples per (half-)chip with taps +-0.5 chip or whole chips apart; 9.5-10 or
 * 11.5-12 samples per chip with taps +-0.5 chip), works out each epoch's setup -- tap constants, chip geometry, carrier
 * rotations -- in one launch with a thread per item: 400-560 bytes of device memory per item, so that the correlator
 * starts an epoch with scalar loads instead of ~450 vector instructions repeated in all 64 lanes.
 * For a list of 4096 items or more that launch is made on a stream of its own and creation returns once the list has been
 * checked (`items` is the caller's again, every error has been reported): run and fetch are ordered behind the setups on
 * the device, destroy waits for them, and so do sdr_engine_sync, sdr_iq_alloc and sdr_code_slots(_ex).
 * sdr_set_option(e, "epl_plan_wait", 1) makes creation wait for them itself (A/B timing, tests); same bits either way. */
typedef struct sdr_epl_plan sdr_epl_plan;
int sdr_epl_plan_create(sdr_engine* e, const sdr_epl_item* items, int n_items,
                        const double* spacing, int n_taps, double fs, sdr_epl_plan** out);
/* The same for a list that is already in DEVICE memory (a closed-loop launch's trajectory turned into items, a list another
 * kernel produced): copied device to device -- the plan owns its items either way -- and checked there, one thread per item;
 * nothing crosses the host but the verdict.  (The host form checks long lists the same way, behind their upload.) */
int sdr_epl_plan_create_dev(sdr_engine* e, const sdr_epl_item* items_dev, int n_items,
                            const double* spacing, int n_taps, double fs, sdr_epl_plan** out);
int sdr_epl_plan_run(sdr_engine* e, sdr_epl_plan* p);
/* Launch only items [first, first+count) of the plan (e.g. one second of a long stream). */
int sdr_epl_plan_run_range(sdr_engine* e, sdr_epl_plan* p, int64_t first, int64_t count);
int sdr_epl_plan_fetch(sdr_engine* e, sdr_epl_plan* p, double* out); /* syncs */
void sdr_epl_plan_destroy(sdr_engine* e, sdr_epl_plan* p);

/* --------------------------------------------------------- PCPS acquisition
 * PCPS (sydr/dsp/acquisition.py:9-74) + TwoCorrelationPeakComparison (:78-115)
 * for n_prn staged codes over the same ring slice:
 *   bins = arange(-doppler_range, doppler_range+1, doppler_step)
 *   map[prn][b][:] = sum_noncoh | sum_coh ifft( fft(x_ms * exp(-1j*(if_hz-bins[b])*k*2*pi/fs)) * conj(fft(code)) ) |
 * peak_bin/peak_code: first global maximum in row-major order;
 * peak_ratio: peak / second peak in the same row outside +-samplesPerChip,
 * never looking at the last code sample (reference behaviour).
 * corr_map may be NULL (indices and ratio only). n_bins_out (nullable) gets len(bins). */
int sdr_pcps(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, double fs,
             double if_hz, double doppler_range, double doppler_step, int coh, int noncoh,
             int64_t* peak_bin, int64_t* peak_code, double* peak_ratio, double* corr_map,
             int* n_bins_out);
/* Same search with caller-supplied code spectra: code_spectra[n_prn][n_code] interleaved
 * complex128 = the `codeFFT` argument of the reference's PCPS() (acquisition.py:9; built as
 * conj(fft(UpsampleCode(code))) at channel_l1ca_kaplan.py:184-185).  Function-level drop-in. */
int sdr_pcps_spectra(sdr_engine* e, const double* code_spectra, int n_prn, int n_code,
                     int64_t start_sample, double fs, double if_hz, double doppler_range,
                     double doppler_step, int coh, int noncoh, int64_t* peak_bin, int64_t* peak_code,
                     double* peak_ratio, double* corr_map, int* n_bins_out);
/* len(np.arange(-range, range+1, step)) for float range/step. */
int sdr_pcps_bins(double doppler_range, double doppler_step);
/* TwoCorrelationPeakComparison alone on a caller-supplied map[n_bins][n_code] (row-major
 * f64), as the legacy twoCorrelationPeakComparison symbol offered (acquisition.c:181-244);
 * the search itself runs on the device. */
int sdr_two_peak_compare(sdr_engine* e, const double* corr_map, int n_bins, int n_code,
                         int samples_per_chip, int64_t* peak_bin, int64_t* peak_code,
                         double* peak_ratio);

/* The same search for any staged code: chip rate, code period and a zero-padded (linear) correlation (no counterpart in the
 * reference, whose acquisition is GPS L1 C/A's; the NumPy statement is dsp.signalsearch.pcps_signal_statement).  All slots of
 * a call hold codes of one length L; s0 = start_sample.
 *   N = nearbyint(fs * L / chip_rate_hz) (half-even), T = N * (1 + pad); *n_code_out = N
 *   r_p[k] = c_p[min(trunc((ts*k)/tc), L-1)], ts = 1/fs, tc = 1/chip_rate_hz, k < N  (UpsampleCode with the chip rate a parameter)
 *   codeFFT_p = conj(fft(r_p followed by T - N zeros)),  bins = arange(-doppler_range, doppler_range+1, doppler_step)
 * pad = 0: sdr_pcps's map with this N and this replica (circular correlation over one code period).
 * pad = 1 (coh must be 1): for block j < noncoh and n < 2N
 *   y[n] = x[s0 + j*N + n] * exp(-1j*(if_hz - bins[b])*(n*2*pi/fs))      (blocks advance by N and read 2N samples)
 *   map[p][b][n] = sum_j | ifft( fft(y) * codeFFT_p )[n] |,  n < N only
 * -- the linear correlation of two periods of signal with one period of code: a data sign that flips at a code boundary
 * inside the window (a symbol as long as the code: E1-B/C, L5, L1C, B1C) no longer splits the peak over the Doppler bins.  The
 * window is (noncoh + 1) * N samples (coh * noncoh * N with pad = 0); it may cross the ring's end where sdr_pcps's may.
 * peak_bin / peak_code: the first maximum in row-major order; peak_ratio: sdr_two_peak_compare's on map[p] with
 * samples_per_chip = excl_samples, or nearbyint(fs / chip_rate_hz) when that is 0.  A sub-carrier needs no field: BOC(1,1) is
 * searched as its half-chip code at twice the chip rate (how the correlators track it), excl_samples covering the side
 * peaks.  Sums are added in a fixed order: two identical calls return identical bits; {1.023e6, 0, 0} on 1023-chip slots is
 * sdr_pcps, bit for bit.  corr_map (nullable): [n_prn][bins][N].
 * SDR_ERR_INVALID: NULL sig, chip rate not finite or not positive, pad outside 0..1, negative excl_samples, non-zero
 * reserved, pad = 1 with coh != 1, slots of different lengths, 2*excl_samples + 1 >= N, and every cause sdr_pcps names;
 * SDR_ERR_UNSUPPORTED: T outside 2 .. 2^24; SDR_ERR_RANGE: a window longer than the ring.  A refused call changes nothing.
 * Profiler scope "call_pcps_signal" around the call's kernels; the inner scopes are sdr_pcps's. */
typedef struct sdr_acq_signal {
    double  chip_rate_hz;   /* > 0, finite: chips per second of the staged codes                       */
    int32_t pad;            /* 0: circular over one code period (sdr_pcps's model)
                               1: linear correlation, code zero-padded to two periods                  */
    int32_t excl_samples;   /* second-peak exclusion half-width; 0 = nearbyint(fs / chip_rate_hz)      */
    int32_t reserved[2];    /* 0 */
} sdr_acq_signal;
int sdr_pcps_signal(sdr_engine* e, const sdr_acq_signal* sig, const int32_t* code_slots, int n_prn,
                    int64_t start_sample, double fs, double if_hz, double doppler_range, double doppler_step,
                    int coh, int noncoh, int64_t* peak_bin, int64_t* peak_code, double* peak_ratio,
                    double* corr_map /* nullable [n_prn][bins][N] */, int* n_bins_out, int* n_code_out);

/* SerialSearch acquisition (sydr/dsp/acquisition.py:119-155; plugin sydr/channel/channel_l1ca_kaplan_ss.py):
 *   map[prn][b][k] = sum over `noncoh` successive code periods of
 *                    |sum_n x[n]*exp(+1j*bins[b]*n*2*pi/fs) * code[(trunc((ts*n)/tc) - k) mod L]|^2
 * with ts = 1/fs, tc = 1/1.023e6, n < N = the samples of a code period, for the L circular chip shifts k, and
 * TwoCorrelationPeakComparison_SS (:159-193) on each map (second peak = maximum outside the 3x3 block around
 * the first, with Python's slice semantics).  The slots' codes have one length L <= 4096 that holds every chip a
 * period's samples land on, L >= trunc((ts*(N-1))/tc) + 1 (1023 at 4 MHz, 1022 at 1.0 MHz): a shorter code is
 * refused with SDR_ERR_INVALID, as the reference raises IndexError; a longer code's further chips enter through
 * the circular shift alone.  corr_map (nullable) is [n_prn][bins][L]. */
int sdr_serial_search(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, double fs,
                      double doppler_range, double doppler_step, int noncoh, int64_t* peak_bin,
                      int64_t* peak_code, double* peak_ratio, double* corr_map, int* n_bins_out);
int sdr_two_peak_compare_ss(sdr_engine* e, const double* corr_map, int n_rows, int n_cols,
                            int64_t* peak_bin, int64_t* peak_code, double* peak_ratio);

/* ------------------------------------------- the correlation function on a dense tap grid
 * What a multi-correlator receiver shows of the peak it tracks (multipath and signal-quality monitoring, discriminator
 * S-curves, the correlation plot beside the acquisition map): the taps of EPL above on the grid
 *   s_j = first_chips + j * step_chips,   0 <= j < n_taps <= SDR_CORR_MAX_TAPS
 * (fp64 exactly as written, one multiply and one add: first + step * np.arange(T)), for every item, in ONE pass over the
 * samples.  out[i][j] = (I, Q) of what EPL returns for item i with the single spacing s_j:
 *   - the same carrier replica;
 *   - the same ceil(linspace(rem_code + s_j, code_step*n + rem_code + s_j, n, endpoint=False)) index in the reference's
 *     operation order;
 *   - padded index p standing for chip c[(p - 1) mod L] (Python's modulo) for ANY p: the call indexes the chip table
 *     modulo the code length itself, so taps many chips out and epochs of several code periods need no
 *     sdr_code_slots_ex periods.
 * Any finite first_chips / step_chips (zero, negative, not dyadic); all four ring formats; a window may cross the ring's
 * end.  Synchronous on the engine's stream like sdr_epl_batch; sums are added in a fixed order (two identical calls return
 * identical bits).  A window that holds NaN / Inf samples (a float ring) gives non-finite outputs for that item.
 * Once the carrier is wiped off, a tap's sum is a sum over CHIPS of the chip's sign times a difference of prefix sums of
 * the wiped samples (~1000 terms per tap at any rate, not one per sample); below ~8 samples per chip -- or with
 * sdr_set_option(e, "corr_profile_per_sample", 1) at any rate (tests, A/B timing) -- the taps are summed sample by
 * sample instead: same definition, results equal to rounding.
 * SDR_ERR_INVALID: NULL pointers, n_items < 1, n_taps outside 1..1024, non-finite first_chips / step_chips, fs <= 0, a
 * slot that is not staged, n_samples < 1, code_step <= 0 or non-finite NCO parameters; SDR_ERR_RANGE: a window longer
 * than the ring, a negative start_sample (the rules of sdr_epl_batch); SDR_ERR_UNSUPPORTED: a chip index that would leave
 * +-2^30; SDR_ERR_STATE: no ring or no code slots.
 * sdr_prof_enable scopes: "corr_items_upload", "corr_walk_kernel" / "corr_per_sample_kernel", "call_corr_profile". */
#define SDR_CORR_MAX_TAPS 1024
int sdr_corr_profile(sdr_engine* e, const sdr_epl_item* items, int n_items, double first_chips, double step_chips,
                     int n_taps, double fs, double* out /* [n_items][n_taps][2] = I, Q */);

/* ------------------------------------------- a delay-Doppler map around a known code phase and carrier
 * The search of a small neighbourhood of a state the receiver already has -- a few chips and a few hundred hertz around
 * a code phase and a carrier: reacquisition after a short loss, a warm start from a prediction, the check that a channel
 * sits on the main peak (not on a cross-correlation peak or a side lobe), and the data product of reflectometry.
 * An item is an sdr_epl_item read as a PREDICTION: start_sample = s0, n_samples = W (the whole window), carrier_hz = f0,
 * rem_carrier / rem_code / code_step = the NCO state at s0 -- what sdr_track_state holds for a channel's next epoch, with
 * a longer n.  With B = n_blocks, S = n_segments, Q = B*S, T = n_taps, K = 2*floor(span_hz/step_hz) + 1:
 *   Stage 1: segment q < Q covers window samples [a_q, b_q), a_q = (q*W)/Q, b_q = ((q+1)*W)/Q (64-bit integer
 *   divisions).  z[q][j] = what EPL above returns for the single spacing s_j = first_chips + j*step_chips (fp64, one
 *   multiply, one add) on ring samples s0+a_q .. s0+b_q-1 (modulo the capacity) with carrier_hz = f0,
 *   rem_carrier_q = (rem_carrier + (-(f0*2.0*pi*a_q/fs))) mod 2*pi (Python's modulo: in [0, 2*pi)),
 *   rem_code_q = rem_code + (double)a_q * code_step (the product, then the sum) and the item's code_step; a padded
 *   index p stands for chip c[(p - 1) mod L] for ANY p, as in sdr_corr_profile.  tau_q = (a_q + b_q - 1) / 2.0 / fs.
 *   Stage 2: d_k = (k - (K-1)/2) * step_hz.  For block b < B:
 *   Z[b][k][j] = sum_{s<S} z[b*S+s][j] * exp(-2j*pi*d_k*tau_{b*S+s}) (s ascending),
 *   map[k][j] = sum_{b<B} |Z[b][k][j]|^2 (b ascending): coherent inside a block, non-coherent across blocks -- choose B so
 *   that a block is shorter than what a data bit or the frequency error allows.
 *   Result: (peak_bin, peak_tap) = the first maximum of map in row-major (k, j) order; peak_hz = f0 + d_peak_bin,
 *   peak_chips = s_peak_tap, peak_value = the map there.  The true code phase at s0 is rem_code + peak_chips, the true
 *   carrier peak_hz.  second_value = the maximum of the entries whose tap lies a chip or more from the peak's
 *   (|s_j - s_peak_tap| >= 1.0, any k), noise_mean their mean; both 0.0 when no entry qualifies.
 * map (nullable) receives [n_items][K][n_taps], segment_sums (nullable) z as [n_items][Q][n_taps][2]; Z and the map are
 * made on the device, the host link carries only what is asked for.  Sums are added in a fixed order, no atomics: two
 * identical calls return identical bits.  Synchronous on the engine's stream like sdr_corr_profile; all four ring formats;
 * a window may cross the ring's end; items of one call may have different W.  A window that holds NaN / Inf samples (a
 * float ring) gives that item a non-finite map, peak_value = second_value = noise_mean = NaN, peak_bin = (K-1)/2,
 * peak_tap = 0, peak_hz = f0, peak_chips = first_chips; no other item is affected.
 * At 8 samples per chip or more a tap is summed as one term per chip run over prefix sums of the wiped samples, below
 * that -- or with sdr_set_option(e, "ddm_per_sample", 1) -- as a term per sample: same definition, equal to rounding.
 * sdr_ddm_bins: K of the grid (host helper like sdr_acq_refine_bins; 0 for a bad grid).
 * SDR_ERR_INVALID: NULL items / cfg / results, n_items outside 1..65535, n_taps outside 1..SDR_CORR_MAX_TAPS, non-finite first_chips /
 * step_chips, a bad fs, step_hz <= 0, span_hz < 0 or either non-finite, n_blocks < 1, n_segments outside 1..64,
 * n_segments == 1 with K > 1 (one segment per block carries no frequency information: every row of the map would be
 * equal to rounding), a slot that is not staged, n_samples < 1, code_step <= 0 or non-finite NCO parameters;
 * SDR_ERR_UNSUPPORTED: K > 4096, Q > 4096, Q > W for some item (an empty segment), a chip index that would leave +-2^30,
 * a code too long for the LDS; SDR_ERR_RANGE: a window longer than the ring, a negative start_sample; SDR_ERR_STATE: no
 * ring or no code slots.  A refused call writes nothing.
 * sdr_prof_enable scopes: "ddm_items_upload", "ddm_segments_kernel", "ddm_map_kernel", "ddm_peak_kernel", "call_ddm". */
typedef struct sdr_ddm_cfg {
    double fs, first_chips, step_chips, span_hz, step_hz;
    int32_t n_taps, n_blocks, n_segments, reserved;
} sdr_ddm_cfg;
typedef struct sdr_ddm_result {
    int32_t peak_bin, peak_tap;
    double peak_hz, peak_chips, peak_value, second_value, noise_mean;
} sdr_ddm_result;
int sdr_ddm_bins(double span_hz, double step_hz);
int sdr_ddm(sdr_engine* e, const sdr_epl_item* items, int n_items, const sdr_ddm_cfg* cfg, sdr_ddm_result* results,
            double* map /* nullable [n_items][K][n_taps] */,
            double* segment_sums /* nullable [n_items][n_blocks*n_segments][n_taps][2] */);

/* ------------------------------------------- successive interference cancellation on the ring
 * The Gold codes isolate one C/A signal from another by only ~24 dB: a satellite tracked at 50 dB-Hz leaves cross-correlation
 * peaks in every other PRN's search map as high as the peak of a signal 24 dB weaker.  The remedy: rebuild each strongly
 * tracked signal from what its loop already knows -- the NCO inputs of every epoch (an sdr_epl_item) and a complex amplitude
 * per epoch --, subtract it from the samples and search in the residue (sdr_pcps / sdr_acq_deep).
 * items[n_ch][n_epochs], amps[n_ch][n_epochs][2] = (a_re, a_im), 1 <= n_ch <= SDR_CANCEL_MAX_CHANNELS; the window is ring
 * samples window_start .. window_start + W - 1 (W = window_samples; it may cross the ring's end).  For an item with
 * n = n_samples, L chips c staged in its slot and A = a_re + j*a_im, sample i = 0..n-1 of the item gets the prompt tap of EPL
 * above (sydr/dsp/tracking.py:92-116: lines 102-104 the replica, 111-112 the chip index), in the reference's operation order:
 *   t_i     = np.arange(0.0, n) / fs
 *   theta_i = -(carrier_hz * 2.0 * np.pi * t_i) + rem_carrier
 *   idx_i   = ceil(linspace(rem_code + 0.0, code_step*n + rem_code + 0.0, n, endpoint=False))
 *   chip_i  = c[(idx_i - 1) mod L]                                              (Python's modulo, any idx)
 *   r_re    = chip_i * (a_re*cos(theta_i) + a_im*sin(theta_i))
 *   r_im    = chip_i * (a_im*cos(theta_i) - a_re*sin(theta_i))                  (A * chip * conj(replica))
 * every product and sum in fp64 exactly as written (the library is built without contraction).  An item sits at window
 * offset off = (start_sample - window_start) mod capacity and lies wholly inside the window (off + n <= W); within a channel
 * the offsets ascend and do not overlap, gaps are allowed, items with n_samples == 0 are padding and are skipped.  A window
 * sample m with ring value x widened to fp64 becomes
 *   y = x;  for ch = 0 .. n_ch-1 in this order:  if an item of ch covers m:  y_re -= r_re;  y_im -= r_im
 * and is stored in the ring's format: cf64 as it is, cf32 rounded to nearest, ci8 / ci16 by sdr_ddc_push's rule (rint,
 * clipped to +-127 / +-32767).  A sample no item covers is copied as it is.  A NaN or Inf input sample stays non-finite and
 * affects no other sample.  The least-squares amplitude of an epoch is its prompt over n_samples (it carries the data
 * bit's sign and the carrier phase): the prompt of the same item on the cancelled samples is then zero to rounding.
 * dst == NULL, or dst == e with dst_offset == window_start (modulo the capacity): the window is replaced in place.  Any
 * other dst -- another engine on the same device with a ring of the same format, or a window of e's own ring that shares no
 * sample with the source window --: the cancelled window goes to dst's ring at dst_offset, wrapping there too, and the
 * source window stays as it is (a live receiver's trackers keep reading the original ring, its searches run on the second
 * engine).  The call waits for dst's stream, runs on e's stream and returns when it is done, like sdr_corr_profile.  Every
 * output sample is written by exactly one thread, which has read its own input first; no atomics touch the samples: two
 * identical calls return identical bits, in place is safe.
 * stats (nullable): samples_written = W, samples_changed = samples at least one item covers, clipped_components = components
 * of an integer ring whose rounded value lay beyond a rail -- exact, equal to the NumPy statement's
 * (sydr_amd/signal/cancel.py: cancel_statement).
 * SDR_ERR_INVALID: NULL items / amps, n_ch outside 1..64, n_epochs < 1, window_samples < 1, fs <= 0, non-finite amplitudes
 * or NCO parameters, code_step <= 0, n_samples < 0, a slot that is not staged, items of a channel that overlap or do not
 * ascend, dst == e with a different window that overlaps the source window, a dst on another device or with a ring of another
 * format; SDR_ERR_RANGE: a window longer than either ring, a negative window_start / dst_offset / start_sample, an item not
 * wholly inside the window; SDR_ERR_UNSUPPORTED: a chip index that would leave +-2^30; SDR_ERR_STATE: no ring (either
 * engine) or no code slots.  A refused call writes nothing.
 * sdr_prof_enable scopes: "cancel_items_upload", "cancel_kernel", "call_iq_cancel". */
#define SDR_CANCEL_MAX_CHANNELS 64
typedef struct sdr_cancel_stats {
    int64_t samples_written, samples_changed, clipped_components;
} sdr_cancel_stats;
int sdr_iq_cancel(sdr_engine* e, const sdr_epl_item* items /* [n_ch][n_epochs] */, const double* amps /* [n_ch][n_epochs][2] */,
                  int n_ch, int n_epochs, double fs, int64_t window_start, int64_t window_samples,
                  sdr_engine* dst /* nullable */, int64_t dst_offset, sdr_cancel_stats* stats /* nullable */);

/* ------------------------------- fine carrier frequency and bit edge behind an acquisition
 * The step between acquisition and tracking of the textbook receiver (code wipe-off over ~10 ms, a fine frequency
 * search), which the reference left out: sdr_pcps hands tracking the best bin of its grid, up to half a grid step off
 * (125 Hz with the shipped 250 Hz), and a Costas loop alone (the Borre plugin) never pulls that in.
 * For each item -- code_slot, start_sample = s0, a ring index at which a code period begins (what the plugins'
 * enterTracking leaves in currentSample), carrier_hz = f0, the coarse carrier (IF included), code_hz -- with
 * M = n_periods, S = n_segments:
 *   N = nearbyint(fs * L / code_hz) samples per code period (L = the chips staged in the slot), code_step = code_hz / fs.
 *   Stage 1: segment (m, s), m < M, s < S, covers window samples [a, b), a = m*N + (s*N)/S, b = m*N + ((s+1)*N)/S
 *   (integer divisions).  z[m][s] = the prompt tap (spacing 0.0) of EPL above on ring samples s0+a .. s0+b-1 (modulo the
 *   capacity) with carrier_hz = f0, rem_carrier = (-(f0*2.0*pi*a/fs)) mod 2*pi, rem_code = ((s*N)/S) * code_step, that
 *   code_step.  tau[m][s] = (a + b - 1) / 2 / fs.
 *   Stage 2: K = 2*floor(span_hz/step_hz) + 1 frequencies d_k = (k - (K-1)/2) * step_hz;
 *   Z[m][k] = sum_s z[m][s] * exp(-2j*pi*d_k*tau[m][s]).  Hypothesis h = 0: no sign change inside the window;
 *   h = 1..M-1: periods m >= h enter with the opposite sign.  P[h][k] = | sum_m sign_h(m) * Z[m][k] |^2.
 *   Result: (h*, k*) = first maximum of P in row-major (h, k) order; fine_hz = f0 + d_k*, fine_idx = k*, bit_edge = h*
 *   (reported, not acted upon), power = P[h*][k*], power_no_edge = max_k P[0][k].
 * One call serves all items (one per searched PRN); both stages run on the device on the engine's stream, sums in a
 * fixed order (two identical calls return identical bits).  power (nullable) receives P as [n_items][n_periods][K],
 * segment_sums (nullable) z as [n_items][n_periods][n_segments][2].
 * A window that holds NaN / Inf samples (a float ring) is reported, not guessed: power = power_no_edge = NaN,
 * fine_hz = f0, fine_idx = (K-1)/2, bit_edge = 0.
 * SDR_ERR_INVALID: NULL items / results, n_items < 1, n_periods outside 1..20 (one data bit: at most one edge),
 * n_segments outside 1..64, a bad grid, a slot that is not staged; SDR_ERR_UNSUPPORTED: n_segments > N, K > 4096, a code
 * period of more than ~16 000 chips or 2^30 samples; SDR_ERR_RANGE: a window longer than the ring, a negative start_sample. */
typedef struct sdr_refine_item {
    int32_t code_slot, reserved;
    int64_t start_sample;
    double carrier_hz, code_hz;
} sdr_refine_item;
typedef struct sdr_refine_result {
    double fine_hz, power, power_no_edge;
    int32_t fine_idx, bit_edge;
} sdr_refine_result;
/* K of the grid above (host helper like sdr_pcps_bins; 0 for a bad grid). */
int sdr_acq_refine_bins(double span_hz, double step_hz);
int sdr_acq_refine(sdr_engine* e, const sdr_refine_item* items, int n_items, double fs, int n_periods, int n_segments,
                   double span_hz, double step_hz, sdr_refine_result* results,
                   double* power /* nullable [n_items][n_periods][K] */,
                   double* segment_sums /* nullable [n_items][n_periods][n_segments][2] */);

/* ------------------------------- secondary-code phase and fine carrier frequency behind an acquisition
 * The step behind sdr_pcps_signal's zero-padded search for signals whose sign may change at every code period (E1-B/C, L5,
 * E5a/b, B1C): where the secondary (overlay) code stands, and with it the carrier to a fine grid's step.  For each item --
 * code_slot (the staged PRIMARY code), sec_row (its row of sec_codes), start_sample = s0, a ring index at which a primary
 * code period begins, carrier_hz = f0, code_hz -- with M = n_periods, S = n_segments, Ls = sec_len, c = the item's row:
 *   Stage 1 is sdr_acq_refine's stage 1, word for word: N = nearbyint(fs * L / code_hz); segment (m, s) covers window samples
 *   [m*N + (s*N)/S, m*N + ((s+1)*N)/S) = [a, b); z[m][s] = EPL's prompt with the rem_carrier, rem_code and code_step written
 *   there; tau[m][s] = (a + b - 1) / 2 / fs.
 *   Frequencies: K = 2*floor(span_hz/step_hz) + 1 (sdr_acq_refine_bins), d_k = (k - (K-1)/2) * step_hz,
 *   Z[m][k] = sum_s z[m][s] * exp(-2j*pi*d_k*tau[m][s]).
 *   Hypotheses: h, 0 <= h < Ls, means that period 0 of the window carries secondary chip c[h]: w_h(m) = c[(h + m) mod Ls].
 *   mode SDR_SEC_PILOT: X[h][k] = sum_m w_h(m) Z[m][k], P[h][k] = |X[h][k]|^2.
 *   mode SDR_SEC_DATA (a data symbol as long as the secondary period: L5-I, E5a-I): periods are grouped by
 *   g = (h + m) div Ls, P[h][k] = sum_g | sum_{m in g} w_h(m) Z[m][k] |^2, partial groups at the window's ends included.
 *   Result: (h*, k*) = first maximum of P in row-major (h, k) order; sec_phase = h*, fine_idx = k*, fine_hz = f0 + d_k*,
 *   power = P[h*][k*], power_other = max of P[h][k] over h != h*, all k; prompt = X[h*][k*] (SDR_SEC_DATA: 0.0, 0.0).
 * n_periods need not be a multiple of sec_len and may be below it (a partial-code search).  One call serves all items; all
 * stages run on the device on the engine's stream; every sum has a fixed order and no atomics (two identical calls return
 * identical bits, whatever else the engine has done).  power (nullable) receives P as [n_items][sec_len][K], segment_sums
 * (nullable) z as [n_items][n_periods][n_segments][2].
 * A window that holds NaN / Inf samples (a float ring) is reported as sdr_acq_refine reports it: power = power_other = NaN,
 * fine_hz = f0, fine_idx = (K-1)/2, sec_phase = 0, prompt 0.
 * Limits: n_periods 2..128, sec_len 2..128, n_segments 1..64 with n_periods * n_segments <= 2048, K <= 4096, n_sec 1..n_items
 * with every sec_row inside it, mode 0 or 1.
 * SDR_ERR_INVALID: NULL items / sec_codes / results, counts outside these ranges, a secondary chip that is neither +1 nor -1,
 * a bad sec_row, a slot that is not staged, a bad grid, a non-finite carrier or a non-positive code_hz; SDR_ERR_UNSUPPORTED:
 * n_periods * n_segments > 2048, n_segments > N, K > 4096, a code period of more than ~16 000 chips or 2^30 samples;
 * SDR_ERR_RANGE: a window longer than the ring, a negative start_sample; SDR_ERR_STATE: no ring or no code slots.  A refused
 * call changes nothing.
 * sdr_prof_enable scopes: "call_secondary" around "secondary_segments", "secondary_search", "secondary_pick". */
typedef struct sdr_sec_item {
    int32_t code_slot;      /* the staged PRIMARY code                                   */
    int32_t sec_row;        /* which row of sec_codes this item's signal carries         */
    int64_t start_sample;   /* a ring index at which a primary code period begins        */
    double  carrier_hz, code_hz;
} sdr_sec_item;
typedef struct sdr_sec_result {
    double  fine_hz, power, power_other;  /* power_other: max of P[h][k] over h != sec_phase, all k */
    double  prompt_re, prompt_im;         /* mode 0: the coherent sum X[h*][k*]; mode 1: 0.0, 0.0    */
    int32_t fine_idx, sec_phase;
} sdr_sec_result;
#define SDR_SEC_PILOT 0
#define SDR_SEC_DATA  1
int sdr_acq_secondary(sdr_engine* e, const sdr_sec_item* items, int n_items,
                      const int8_t* sec_codes /* [n_sec][sec_len], each +1 or -1 */, int n_sec, int sec_len,
                      double fs, int n_periods, int n_segments, double span_hz, double step_hz, int mode,
                      sdr_sec_result* results,
                      double* power /* nullable [n_items][sec_len][K] */,
                      double* segment_sums /* nullable [n_items][n_periods][n_segments][2] */);

/* ------------------------------- coherent search under secondary-code hypotheses
 * The acquisition of a signal that carries a secondary (overlay) code, coherent across its code periods: where
 * sdr_pcps_signal's zero-padded search adds the M periods of a window as magnitudes, this one adds the complex per-period
 * correlations under every hypothesis of the overlay phase and every frequency of a fine grid, and returns code sample,
 * Doppler bin, overlay phase and fine carrier in one call (opt-in by calling it; the NumPy statement is
 * dsp.signalsearch.pcps_coherent_statement).  With M = n_periods, Ls = sec_len, c = the PRN's row sec_rows[p] of sec_codes,
 * s0 = start_sample:
 *   L, N, r_p, bins: exactly sdr_pcps_signal's.  T = 2N.  codeFFT_p = conj(fft(r_p followed by N zeros)).
 *   Blocks: for m < M and n < 2N, y_m[n] = x[s0 + m*N + n] * exp(-1j*(if_hz - bins[b])*(n*2*pi/fs)).  This is block j = m of
 *   sdr_pcps_signal's pad = 1.  The carrier restarts per block, as there.
 *   Per-period correlation: C_m[b][tau] = ifft(fft(y_m) * codeFFT_p)[tau] for tau < N.  The complex value is kept.  It is the
 *   linear correlation of the period that begins at window sample m*N + tau.
 *   Rotation: g(m,b,k) = exp(-2j*pi*(if_hz - bins[b] + d_k)*(m*N)/fs).  This continues the carrier across blocks and moves it
 *   by the fine offset.  K = sdr_acq_refine_bins(span_hz, step_hz), d_k = (k - (K-1)/2) * step_hz.
 *   Hypotheses: w_h(m) = c[(h + m) mod Ls], as in sdr_acq_secondary.
 *   Pilot mode (SDR_SEC_PILOT): X[b][h][k][tau] = sum_m w_h(m) g(m,b,k) C_m[b][tau], with m ascending.  P = |X|^2.
 *   Data mode (SDR_SEC_DATA): periods are grouped by g = (h + m) div Ls.
 *   P = sum_g |sum_{m in g} w_h(m) g(m,b,k) C_m[b][tau]|^2.  Partial groups at both ends are included.
 *   Reduced map: R[p][b][tau] = sqrt(max_{h,k} P[b][h][k][tau]).  It is a magnitude, like every other map here, so the ini
 *   files' ratio threshold means what it means elsewhere.  corr_map receives it.
 *   Peak: peak_bin, peak_code and peak_ratio are sdr_two_peak_compare's on R[p], with samples_per_chip = excl_samples (or its
 *   default).  The window quirks of the reference are kept, as in sdr_pcps_signal.
 *   Pick at the peak cell: (h*, k*) is the first maximum of P[b*][.][.][tau*] in row-major (h, k) order.  power_other and
 *   prompt are as in sdr_acq_secondary.  power receives that [Ls][K] table.
 *   Window: (M + 1) * N samples.  It may cross the ring's end where sdr_pcps's may.  All four ring formats are supported.
 *   Order: every sum has a fixed order and nothing is added atomically.  Maxima are taken with p > best, so NaN never wins,
 *   as in refine / secondary (a cell whose every P is NaN has R = 0).  Two identical calls return identical bits, whatever the
 *   engine did before.
 * Limits: n_periods 2..128 and sec_len 2..128, neither needing to divide the other.  K <= 64 and sec_len * K <= 4096.
 * n_sec 1..n_prn, with every sec_rows[p] inside it.  T within sdr_pcps_signal's 2..2^24.
 * Statuses: sdr_pcps_signal's and sdr_acq_secondary's causes, each with the status it has there (K > 64 and
 * sec_len * K > 4096: SDR_ERR_UNSUPPORTED, as K > 4096 there).  A refused call changes nothing.
 * The per-period correlations of a chunk of (PRN, bin) units lie in a scratch of [M][units][T] complex doubles; the units are
 * cut into chunks under a byte budget (sdr_set_option "coherent_scratch_kb", 0 = the default of 2 GiB; never less than one
 * unit).  No result depends on the cut.
 * sdr_prof_enable scopes: "call_pcps_coherent" around "coherent_fwd_fft", "coherent_inv_fft", "coherent_combine",
 * "coherent_peak", "coherent_pick". */
typedef struct sdr_coh_cfg {
    double  chip_rate_hz;        /* as sdr_acq_signal                                                    */
    double  span_hz, step_hz;    /* fine grid: K = sdr_acq_refine_bins(span_hz, step_hz), d_k = (k-(K-1)/2)*step_hz */
    int32_t n_periods;           /* M: code periods added coherently (pilot) / per symbol group (data)   */
    int32_t sec_len;             /* Ls                                                                   */
    int32_t mode;                /* SDR_SEC_PILOT / SDR_SEC_DATA, sdr_acq_secondary's meaning            */
    int32_t excl_samples;        /* as sdr_acq_signal; 0 = nearbyint(fs / chip_rate_hz)                  */
    int32_t reserved[2];         /* 0 */
} sdr_coh_cfg;
typedef struct sdr_coh_result {
    double  carrier_hz;          /* if_hz - bins[peak_bin] + d_{fine_idx}                                */
    double  peak, peak_ratio;    /* R at the peak cell; sdr_two_peak_compare's ratio on R[p]             */
    double  power, power_other;  /* P[h*][k*] at the peak cell; max of P[h][k], h != h*, at that cell    */
    double  prompt_re, prompt_im;/* pilot: X[h*][k*] at the peak cell; data: 0.0, 0.0                    */
    int64_t peak_code;           /* tau*: window sample at which a code period begins                    */
    int32_t peak_bin, fine_idx, sec_phase, reserved;
} sdr_coh_result;
int sdr_pcps_coherent(sdr_engine* e, const sdr_coh_cfg* cfg, const int32_t* code_slots, const int32_t* sec_rows, int n_prn,
                      const int8_t* sec_codes /* [n_sec][sec_len], +1 / -1 */, int n_sec,
                      int64_t start_sample, double fs, double if_hz, double doppler_range, double doppler_step,
                      sdr_coh_result* results /* [n_prn] */, double* corr_map /* nullable [n_prn][bins][N] */,
                      double* power /* nullable [n_prn][sec_len][K] */, int* n_bins_out, int* n_code_out);

/* ------------------------------- deep acquisition: folded coherent blocks, code-Doppler shift, bit-edge groups
 * The search for weak signals (opt-in like sdr_acq_refine; sdr_pcps is unchanged).  N, the Doppler grid d_b = bins[b]
 * (np.arange(-doppler_range, doppler_range + 1, doppler_step)), the code spectra codeFFT_p = conj(fft(UpsampleCode(code_p)))
 * and the mixing sign (the carrier removed for bin b is if_hz - d_b: a peak_bin means what sdr_pcps's means) are sdr_pcps's.
 * With C = coh coherent periods per block (1..20), K = noncoh blocks (>= 1), G = groups bit-edge groups (1 or 2, K >= G) and
 * carrier_rf_hz, the carrier the code Doppler is scaled by (> 0, or 0 for no compensation), the window is C*K*N ring samples
 * from start_sample = s0 (it may cross the ring's end where sdr_pcps's may).  For block i < K, bin b, sample n < N:
 *   phi[k]     = k * 2 * pi / fs, k < C*N              (np.array(range(C*N)) * 2 * np.pi / fs: the carrier restarts with every
 *                                                       block, as the reference's does)
 *   F[b][i][n] = sum_{c<C} x[s0 + (i*C + c)*N + n] * exp(-1j * (if_hz - d_b) * phi[c*N + n])
 *   R[p][b][i] = ifft( fft(F[b][i]) * codeFFT_p )
 *   q[b][i]    = nearbyint( d_b * float(i*C*N) / carrier_rf_hz )   (fp64 in this order, half-even; 0 when carrier_rf_hz == 0)
 *   M[p][g][b][n] = sum over i = g (mod G), ascending i, of | R[p][b][i][ (n + q[b][i]) mod N ] |        (Python's modulo)
 * The C mixed periods of a block are added in front of ONE forward transform (the transform is linear): C times fewer
 * transforms than sdr_pcps(coh = C).  Blocks that hold a data-bit edge lose energy; with G = 2 and C*N half a bit or less, the
 * blocks of one of the two groups hold none.  q moves every block's map back by the code's drift at the bin's Doppler, so
 * the peak of a long window stays on one sample.  With G = 1 and carrier_rf_hz = 0, M is PCPS(coh = C, noncoh = K)'s map up
 * to the order of additions.
 * Per PRN: (peak_group, peak_bin, peak_code) = the first maximum of M[p] in row-major (g, b, n) order, peak_value = M[p]
 * there, peak_ratio = TwoCorrelationPeakComparison on M[p][peak_group] (the second peak from the winning row, with the
 * reference's exclusion window, as in sdr_pcps), peak_code_end = (peak_code + nearbyint(d_peak * float(K*C*N) /
 * carrier_rf_hz)) mod N: the code start referred to the window's END, which is what a caller that places currentSample
 * behind the window needs (postAcquisitionUpdate); equal to peak_code when carrier_rf_hz == 0.
 * The shifts are made on the host by sdr_acq_deep_shift's expression and uploaded as integers; sums are added in a fixed
 * order (two identical calls return identical bits); the call is synchronous on the engine's stream.  The maps of all PRNs
 * stay resident for the call: n_prn * G * bins * N * 8 bytes (32 PRNs, two groups, 201 bins at 25 MHz: 2.6 GB); a call
 * whose buffers cannot be reserved fails with SDR_ERR_NOMEM like any other.  corr_map (nullable) receives M.
 * SDR_ERR_INVALID: NULL code_slots / cfg / results, n_prn < 1, coh outside 1..20, noncoh < 1, groups outside 1..2,
 * noncoh < groups, a bad grid or fs, negative or non-finite carrier_rf_hz, a slot that is not staged; SDR_ERR_RANGE: a
 * window longer than the ring, a negative start_sample; SDR_ERR_STATE: no ring or no code slots.
 * sdr_prof_enable scopes: "deep_fold", "deep_fwd_fft", "deep_inv_fft", "deep_shift_acc", "deep_peak", "call_acq_deep" (the
 * code spectra, made when they are not cached, keep sdr_pcps's "pcps_upsample" / "pcps_code_fft"). */
typedef struct sdr_deep_cfg {
    double fs, if_hz, doppler_range, doppler_step, carrier_rf_hz;
    int32_t coh, noncoh, groups, reserved;
} sdr_deep_cfg;
typedef struct sdr_deep_result {
    int64_t peak_bin, peak_code, peak_code_end;
    int32_t peak_group, reserved;
    double peak_ratio, peak_value;
} sdr_deep_result;
int sdr_acq_deep(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, const sdr_deep_cfg* cfg,
                 sdr_deep_result* results, double* corr_map /* nullable [n_prn][groups][bins][N] */);
/* q[b][i] above for b = bin, i = block (host helper like sdr_pcps_bins; block = noncoh gives the shift of peak_code_end;
 * 0 for a NULL cfg, a negative bin or block, or carrier_rf_hz == 0). */
int64_t sdr_acq_deep_shift(const sdr_deep_cfg* cfg, int bin, int64_t block);

/* ------------------------------- detection statistics of a deep search: K separated peaks and the noise floor (opt-in)
 * sdr_acq_deep's search, and then, on the maps while they are resident on the device, per PRN (M[G][B][N] its map as
 * above, dist(n, m) the circular distance mod N):
 *   peak k, k = 0 .. n_peaks-1: the first maximum, in row-major (g, b, n) order, of M over the cells outside every zone Z_j,
 *     j < k;  Z_j = {(g, b, n): |b - b_j| <= excl_bins and dist(n, n_j) <= excl_code} for EVERY g (the groups are the same
 *     signal on interleaved blocks).  Peak 0 is sdr_acq_deep's peak.  group, bin, code, value = M there, code_end =
 *     peak_code_end's expression with the peak's own bin; group = -1 and value = 0.0 where no cell is left.
 *   noise cells Omega: every (g, b, n) with dist(n, n_j) > excl_code for every reported peak j, in all bins and all groups
 *     (a signal's ridge runs along the Doppler axis: whole code columns are left out).  n_cells = |Omega| (exact),
 *     mean = (sum over Omega of M) / n_cells, variance = (sum over Omega of (M - mean)^2) / n_cells with `mean` the double
 *     returned (two passes, population variance).
 *   z_k = (value_k - mean) / sqrt(variance), fp64 in this order, made on the host side of the library from the numbers it
 *     returns.  The call reports sigma units; it says nothing about the distribution behind them.
 * The sums are fixed-order fp64 sums of non-negative terms: mean and variance lie within (n_cells + 4) * 2^-53, relative, of
 * the exactly rounded sums of the same cells; indices, counts and peak values are exact.  The parts the sums are made of are
 * runs of 2048 columns of one map row -- a constant, not derived from n_prn or the device: a PRN's figures depend on its own
 * map alone and two identical calls return identical bits.  `results` and `corr_map` are bit for bit sdr_acq_deep's.  With
 * groups = 1 and carrier_rf_hz = 0 this is a plain PCPS map with statistics.
 * SDR_ERR_INVALID: sdr_acq_deep's causes, NULL det / peaks / noise, n_peaks outside 1..8, a negative window, a non-zero
 * `reserved`, n_peaks * (2*excl_code + 1) >= N (Omega could be empty).  A refused call changes nothing.
 * sdr_prof_enable scopes: sdr_acq_deep's, and "deep_detect_peaks", "deep_detect_noise", "call_acq_deep_detect" (in place of
 * "call_acq_deep"). */
typedef struct sdr_detect_cfg {
    int32_t n_peaks /* 1..8 */, excl_code /* samples, >= 0 */, excl_bins /* >= 0 */, reserved;
} sdr_detect_cfg;
typedef struct sdr_detect_peak {
    int64_t bin, code, code_end;
    int32_t group, reserved;
    double value, z;
} sdr_detect_peak;
typedef struct sdr_detect_noise {
    int64_t n_cells;
    double mean, variance;
} sdr_detect_noise;
int sdr_acq_deep_detect(sdr_engine* e, const int32_t* code_slots, int n_prn, int64_t start_sample, const sdr_deep_cfg* cfg,
                        const sdr_detect_cfg* det, sdr_deep_result* results /* as sdr_acq_deep */,
                        sdr_detect_peak* peaks /* [n_prn][n_peaks] */, sdr_detect_noise* noise /* [n_prn] */,
                        double* corr_map /* nullable, as sdr_acq_deep */);

/* ------------------------------------------------- closed-loop tracking
 * On-device loop closure: one persistent workgroup per
 * channel runs n_epochs of correlate -> discriminators -> loop filters -> NCO
 * update without leaving the GPU.  loop_kind selects the reference plugin whose
 * arithmetic is followed: 0 = Borre (channel_l1ca_borre.py:333-451),
 * 1 = Kaplan (channel_l1ca_kaplan.py:342-619). */
typedef struct sdr_track_state {
    int32_t code_slot;
    int32_t n_samples;        /* track_requiredSamples of the NEXT epoch            */
    int64_t current_sample;   /* currentSample (ring index)                         */
    double carrier_hz;        /* carrierFrequency                                   */
    double code_hz;           /* codeFrequency                                      */
    double rem_carrier;       /* remainingCarrier / NCO_remainingCarrier            */
    double rem_code;          /* remainingCode / NCO_remainingCode                  */
    double code_step;         /* codeStep                                           */
    double dll_mem;           /* Borre: NCO_codeError; Kaplan: dllDiscrim           */
    double pll_mem;           /* Borre: NCO_carrierError; Kaplan: fll_vel_memory    */
    double i_prompt_prev;     /* Kaplan iPromptPrev                                 */
    double q_prompt_prev;     /* Kaplan qPromptPrev                                 */
    double fll_lock;          /* Kaplan fllLockIndicator                            */
    double pll_lock;          /* Kaplan pllLockIndicator                            */
    double cn0;               /* Kaplan cn0 (= dllLockIndicator)                    */
    double cn0_ratio_acc;     /* Kaplan cn0_PdPnRatio                               */
    double fll_bw;            /* Kaplan fllBandwidth                                */
    double pll_bw;            /* Kaplan pllBandwidth                                */
    int32_t code_counter;     /* codeCounter                                        */
    int32_t accum_counter;    /* Kaplan correlatorsAccumCounter                     */
    int32_t lock_state;       /* Kaplan LoopLockState (1 PULL_IN, 2 WIDE, 3 NARROW) */
    int32_t track_flags;      /* TrackingFlags bit set                              */
    int32_t time_in_state;    /* Kaplan timeSinceLastState                          */
    int32_t spacing_sel;      /* Kaplan: 0 = wide taps, 1 = narrow taps             */
    /* navigation-bit accumulation on device: decodeBit of
     * channel_l1ca_kaplan.py:728-754 / channel_l1ca_borre.py:470-491 + Prompt2Bit (dsp/decoding.py:16-27) */
    double nav_prompt_sum;    /* navPromptSum                                       */
    int32_t nav_sum_counter;  /* navPromptSumCounter                                */
    int32_t nav_bits_emitted; /* bits produced so far (navBitsCounter without the reference's flushes) */
} sdr_track_state;

typedef struct sdr_loop_cfg {
    int32_t loop_kind;        /* 0 Borre, 1 Kaplan                                  */
    int32_t n_taps;           /* 3 (E/P/L, the reference) or 5 (VE/E/P/L/VL); the discriminators use the centre
                               * tap as prompt and its two neighbours as early / late                           */
    double fs;
    double spacing_wide[SDR_MAX_TAPS];
    double spacing_narrow[SDR_MAX_TAPS];
    double dll_tau1, dll_tau2, dll_pdi;
    double pll_tau1, pll_tau2, pll_pdi;       /* Borre                              */
    double dll_threshold;                     /* Kaplan                             */
    double fll_bw_pullin, fll_bw_wide, fll_bw_narrow, fll_thr_wide, fll_thr_narrow;
    double pll_bw_wide, pll_bw_narrow, pll_thr_wide, pll_thr_narrow;
    /* generalisation beyond the reference's GPS L1 C/A epoch (BASELINE configs 4-5; no reference counterpart):
     * chips per correlator epoch (code length x code periods; 0 = 1023, the reference's GPS_L1CA_CODE_SIZE_BITS at
     * channel_l1ca_kaplan.py:529-532) and epochs per navigation symbol (0 = 20 = LNAV_MS_PER_BIT). */
    double epoch_chips;
    int32_t epochs_per_bit;
    int32_t reserved;
    /* epoch duration the Kaplan discriminators / filters / C/N0 estimator are scaled with; 0 = 1e-3 s, the constant
     * the reference hard-codes (channel_l1ca_kaplan.py:417,425,443,494).  4e-3 for the 4 ms epochs of configs 4-5. */
    double epoch_seconds;
} sdr_loop_cfg;

/* Per-epoch record written when traj != NULL (what the reference's tracking
 * packet carries, channel_l1ca_kaplan.py:653-676, plus the NCO inputs used). */
typedef struct sdr_track_epoch {
    int64_t start_sample;
    int32_t n_samples;
    int32_t lock_state;
    double carrier_hz_in, rem_carrier_in, rem_code_in, code_step_in; /* inputs of the epoch */
    double corr[2 * SDR_MAX_TAPS];
    double dll, pll, fll;
    double carrier_err, code_err;
    double carrier_hz, code_hz;           /* after the update */
    double cn0, pll_lock, fll_lock;
    int32_t track_flags;
    int32_t nav_bit;                      /* -1: none this epoch; 0/1: bit closed by this epoch (20 prompts) */
} sdr_track_epoch;

/* A channel is tracked by a cluster of 1, 2, 4 or 8 cooperating workgroups (one per compute unit; the
 * partial sums of an epoch are added in a fixed order, so a given cluster size always gives the same
 * bits).  parts = 0 (default) lets the library fill the GPU: min(8, CUs / n_ch) rounded down to a power
 * of two.  The reference has no counterpart: its channels are one Python process each
 * (sydr/channel/channel.py:90-151). */
int sdr_track_cluster(sdr_engine* e, int parts);
int sdr_track_closed_loop(sdr_engine* e, int n_ch, sdr_track_state* st, const sdr_loop_cfg* cfg,
                          int n_epochs, sdr_track_epoch* traj /* [n_ch][n_epochs], nullable */);
/* Same run; additionally the navigation bits decided during it leave the device as one byte each
 * (only 1 bit per 20 ms per channel has to cross PCIe): nav_bits[n_ch][max_bits] (0/1), bit k of
 * channel c at nav_bits[c*max_bits + k]; n_bits[c] = number written for channel c. */
int sdr_track_closed_loop_bits(sdr_engine* e, int n_ch, sdr_track_state* st, const sdr_loop_cfg* cfg,
                               int n_epochs, sdr_track_epoch* traj, int8_t* nav_bits, int max_bits,
                               int32_t* n_bits);

/* Same run with a per-channel outcome instead of one status for the call: epochs_done[c] = epochs channel c
 * completed (< n_epochs when its NCO left the staged replica / the ring: that channel stops, st[c] holds its last
 * valid state, the others are unaffected -- the reference likewise lets a channel that lost lock run on alone,
 * sydr/channel/channel.py:121-160).  cfgs: one sdr_loop_cfg per channel when cfg_per_channel != 0, else cfgs[0]
 * serves all (channelManager.addChannel takes a configuration per call, channelManager.py:70-93). */
int sdr_track_closed_loop_ex(sdr_engine* e, int n_ch, sdr_track_state* st, const sdr_loop_cfg* cfgs,
                             int cfg_per_channel, int n_epochs, sdr_track_epoch* traj, int8_t* nav_bits,
                             int max_bits, int32_t* n_bits, int32_t* epochs_done);

/* ------------------------------------------------- device-resident channel bank
 * The tracking state of every channel of one GPU lives in HBM (sdr_track_state + sdr_loop_cfg per channel) and
 * is advanced there; the host keeps views.  This replaces the reference's one-process-per-channel fan-out with
 * its per-millisecond Event barrier (sydr/channel/channelManager.py:70-127,149-188, sydr/channel/channel.py:121-160):
 * one sdr_bank_step = "every listed channel runs n_epochs tracking epochs", one sdr_bank_tick = one iteration of the
 * receiver's outer loop (receiver.py:120-131: addNewRFData of one slab, then run) in a single call.
 * Channels are independent; a call on one stream never touches channels that are not listed. */
typedef struct sdr_bank sdr_bank;
int sdr_bank_create(sdr_engine* e, int max_channels, sdr_bank** out);
void sdr_bank_destroy(sdr_engine* e, sdr_bank* b);
/* Host -> HBM: (re)initialise channel ch (after acquisition: postAcquisitionUpdate, channel_l1ca_kaplan.py:217-235). */
int sdr_bank_put(sdr_engine* e, sdr_bank* b, int ch, const sdr_track_state* st, const sdr_loop_cfg* cfg);
/* HBM -> host. */
int sdr_bank_get(sdr_engine* e, sdr_bank* b, int ch, sdr_track_state* st);
/* Advance the listed channels by n_epochs each.  records[n_ch][n_epochs] (nullable) receives the per-epoch
 * packets' contents, states_out[n_ch] (nullable) the states after the run, epochs_done[n_ch] (nullable) the epochs
 * each channel completed, nav_bits/n_bits as in sdr_track_closed_loop_bits.  stream_id: 0 = the engine's stream,
 * else a stream from sdr_stream_create (one stream per channel batch).  Synchronous on that stream. */
int sdr_bank_step(sdr_engine* e, sdr_bank* b, const int32_t* channels, int n_ch, int n_epochs,
                  sdr_track_epoch* records, sdr_track_state* states_out, int32_t* epochs_done,
                  int8_t* nav_bits, int max_bits, int32_t* n_bits, int stream_id);
/* sdr_bank_step (on the engine's stream, records and states always produced) in two halves: _begin queues the launch and
 * the copies of its results into page-locked memory and returns at once; _end waits and hands them out.  One step may be
 * in flight per bank; work queued on the engine's stream in between (a tick, an upload) runs after it.  Lets a receiver
 * that tracks ahead (sydr_amd/channel/readahead.py) have its next block computed while it still hands out the current
 * one's packets.  SDR_ERR_STATE: _begin with a step in flight, _end without one. */
int sdr_bank_step_begin(sdr_engine* e, sdr_bank* b, const int32_t* channels, int n_ch, int n_epochs);
int sdr_bank_step_end(sdr_engine* e, sdr_bank* b, sdr_track_epoch* records /* [n_ch][n_epochs] */, sdr_track_state* states_out,
                      int32_t* epochs_done);
/* One receiver tick: copy n_samples new host samples into the ring at ring_offset (CircularBuffer.shift), then
 * one epoch for the listed channels (n_ch may be 0: ingest only).  One stream synchronisation in all. */
int sdr_bank_tick(sdr_engine* e, sdr_bank* b, const void* iq, int64_t n_samples, int64_t ring_offset,
                  const int32_t* channels, int n_ch, sdr_track_epoch* records, sdr_track_state* states_out,
                  int32_t* epochs_done);

/* The same tick with the reference's per-tick bookkeeping done here instead of in the caller's language: which
 * channels are ready (channel.py:137-146 -- the ring holds their next epoch completely: getNbUnreadSamples >=
 * track_requiredSamples), one epoch for those, and the caller's MIRRORS of the bank brought up to date in place --
 * what ChannelManager.run() needs to make its TRACKING_UPDATE and CHANNEL_UPDATE packets (channelManager.py:149-188,
 * channel.py:205-228) is in `records` / `updates` when the call returns.  Every array has max_channels rows and is
 * owned by the caller; rows of channels that do not run are not touched. */
typedef struct sdr_tick_update {      /* one CHANNEL_UPDATE (channel.py:205-228) */
    int32_t channel;
    int32_t track_flags;              /* the device's TrackingFlags bits | host_flags[channel]            */
    int64_t unread;                   /* unprocessed_samples: getNbUnreadSamples(currentSample) afterwards */
    int64_t epochs_since_tow;         /* code_since_tow                                                    */
} sdr_tick_update;
typedef struct sdr_tick_mirror {
    int32_t max_channels;             /* rows of every array = the bank's max_channels                     */
    int32_t reserved;
    sdr_track_state* states;          /* in/out: state of every channel as last put / advanced             */
    sdr_track_epoch* last;            /* out: the newest epoch record per channel                          */
    int64_t* epochs_since_tow;        /* in/out (nullable): += 1 per epoch run (codeSinceTOW)              */
    const uint8_t* tracking;          /* in: channel is in ChannelState.TRACKING                           */
    uint8_t* lost;                    /* in/out: the device parked the channel (its NCO left the replica / the ring) */
    const int64_t* host_flags;        /* in (nullable): TrackingFlags bits the host owns (the decoder's)   */
    int32_t* ran;                     /* out: channels that completed an epoch in this tick, ascending     */
    sdr_track_epoch* records;         /* out: their records, same order                                    */
    sdr_tick_update* updates;         /* out: one row per channel with tracking != 0, ascending            */
    int32_t n_ran, n_updates;         /* out                                                               */
    int32_t n_nav_bits;               /* out: records of this tick with nav_bit >= 0                       */
    int32_t n_lost;                   /* out: channels parked by this tick                                 */
    int64_t max_unread;               /* out: largest `unread` among the channels still running            */
} sdr_tick_mirror;
/* iq may be NULL / n_samples 0 when the slab was handed over with sdr_iq_upload_begin already; write_index = the
 * ring's write index AFTER this tick's slab (CircularBuffer.idxWrite). */
int sdr_bank_tick_mirrored(sdr_engine* e, sdr_bank* b, const void* iq, int64_t n_samples, int64_t ring_offset,
                           int64_t write_index, sdr_tick_mirror* m);
/* The same tick in two halves, so that ONE host thread drives the banks of several devices the way the reference's
 * manager drives its channel processes -- start every one, then wait for each (channelManager.py:164-171: eventRun.set()
 * for all, then eventDone.wait() for all).  _begin decides who is ready and queues their epoch on the engine's stream
 * (nothing is waited for; the bank's own page-locked block takes the results, so other calls on the engine may come in
 * between, but none that touches THIS bank: they return SDR_ERR_STATE); _end waits, absorbs the results into the mirrors
 * and writes the tick's rows.  sdr_bank_tick_mirrored == _begin + _end.  Same `m` in both halves. */
int sdr_bank_tick_mirrored_begin(sdr_engine* e, sdr_bank* b, const void* iq, int64_t n_samples, int64_t ring_offset,
                                 int64_t write_index, sdr_tick_mirror* m);
int sdr_bank_tick_mirrored_end(sdr_engine* e, sdr_bank* b, sdr_tick_mirror* m);
/* sdr_set_option(e, "tick_server", 1): the steady tick (sdr_bank_tick_mirrored*, the slab handed over by
 * sdr_iq_upload_begin) is answered by RESIDENT kernels instead of launches and a stream synchronisation -- what the
 * reference's manager gets from channel processes that wait on an Event between ticks (channel.py:121-160).  The cluster form
 * of the tracking kernel stays on the device; eight more workgroups, the doormen, watch a 64-byte request line in page-locked
 * memory (the whole request in one access over the link), pull an eighth of the slab each into the ring and release the
 * channels; every channel ANSWERS THE HOST ITSELF -- state, record and the request's number written straight into page-locked
 * memory by one of its waves -- and the host spins on those words; who is ready is decided on the device by the arithmetic of
 * channel.py:137-146 and must agree with the caller's mirror (SDR_ERR_STATE otherwise).  Same clusters and order of additions
 * as the plain tick: same bits.  Served: banks whose tracking channels run one tap count and number at most a quarter of the
 * compute units (64), after eight such ticks in a row with no other call on the engine in between (a server takes ~25 ms to
 * start); anything else takes the plain path.  Any other call on the engine (a search, a put, an upload by another route,
 * sdr_engine_destroy) tells the server to leave first and waits for it; the next steady tick starts a new one.  Nothing on the
 * device waits without a bound: the server leaves by itself after 0.2 s without a request; the host waits at most 0.25 s for
 * an answer, then reports SDR_ERR_HIP and goes back to plain ticks.
 * out4: {a server is resident now, requests answered, servers started, the engine went back to plain ticks for good}.
 *
 * sdr_set_option(e, "bind_thread_to_device", 1): the CALLING thread is restricted to the CPUs next to the engine's GPU (the
 * local_cpulist of its PCI function; never outside the thread's present mask), 0 gives it its old mask back; SDR_ERR_UNSUPPORTED
 * where sysfs does not say.  A served tick is a handful of round trips through page-locked words: from the other socket of a
 * two-socket host each crosses the sockets' interconnect too (21 us per tick against 27, examples/receiver_loop.c).  Opt-in: a
 * library does not move its caller's threads unasked. */
int sdr_tick_server_stats(sdr_engine* e, int64_t* out4);
/* Where the answered requests' time went ON THE DEVICE, microseconds summed over them (the first doorman's wall-clock stamps):
 * {slab pulled into the ring, channels released, every channel has answered -- as the doorman sees it, which keeps quiet
 * while the channels work: up to a microsecond late --, the request closed}. */
int sdr_tick_server_phases(sdr_engine* e, double* out4);
/* ... and channel 0's own tick (lane 0 of its first part): {release seen, samples visible, correlated, sums exchanged, loops
 * updated, answer written}. */
int sdr_tick_server_tracker_phases(sdr_engine* e, double* out6);
/* sdr_iq_upload without the wait: the samples are copied out of `iq` before the call returns (the caller may reuse
 * its buffer), their transfer into the ring is queued on the engine's stream and ordered before everything queued
 * there afterwards (slabs above 1 MiB are uploaded synchronously).  sdr_engine_sync completes it for readers on
 * other streams.  Lets addNewRFData start the transfer while the caller is still on its way to run().  Any number of
 * slabs may be outstanding: the engine stages them in two page-locked halves and waits, before it overwrites a half, for
 * the transfer that read it (an event per half) -- a caller that queues a third slab while the first has not reached the
 * ring blocks in this call until it has; nothing is lost or reordered.  A tick in which no channel was ready
 * (sdr_bank_tick_mirrored with n_ran == 0 and n_samples == 0) launches nothing and waits for nothing: the slab is then
 * still in flight when the call returns.  Between receiver ticks the slab only waits in its staging half: the next
 * sdr_bank_tick_mirrored's ONE launch begins with workgroups that pull it into the ring while the trackers behind them set
 * up (or the resident tick server's doormen pull it); every other call on the engine puts it into the ring first, in order.
 * ONE exception to "copied before the call returns": a slab that lies in page-locked memory from sdr_host_alloc, on a 16-byte
 * boundary and a whole number of 16-byte granules long, is read IN PLACE by whoever pulls it into the ring (no staging copy:
 * ~2 us of a 50 KB slab) -- the caller leaves it unchanged until the next sdr_bank_tick* of the engine, or sdr_engine_sync,
 * has returned. */
int sdr_iq_upload_begin(sdr_engine* e, const void* iq, int64_t n_samples, int64_t ring_offset);
/* A chunk of a recording (any size) queued for the ring WITHOUT being copied first: one asynchronous copy command on the
 * engine's stream, ordered like everything else queued there; the caller keeps `iq` valid and unchanged until
 * sdr_engine_sync (or a later synchronous call on the engine) returns.  From page-locked memory (sdr_host_alloc) the call
 * returns at once and the transfer runs beside whatever other streams compute -- how a file reader feeds the ring a second
 * of samples at a time while the previous second is correlated (rfsignal.py:58-132 reads the file chunk by chunk; bench.py
 * `host_fed`); from pageable memory the runtime stages the chunk through its own buffers and the call returns when the last
 * piece has been handed over.  n_samples up to the ring's capacity, wrapping at its end. */
int sdr_iq_upload_queue(sdr_engine* e, const void* iq, int64_t n_samples, int64_t ring_offset);
/* Page-locked host memory for recordings that are fed with sdr_iq_upload_queue (hipHostMalloc / hipHostFree on the engine's
 * device).  The block is the caller's until sdr_host_free; the engine keeps no pointer to it. */
int sdr_host_alloc(sdr_engine* e, size_t bytes, void** out);
int sdr_host_free(sdr_engine* e, void* block);

/* ------------------------------------------------- packed recordings: 1, 2 or 4 bits per component
 * What most front ends deliver and most recordings hold: several I,Q samples to a byte.  They cross the host link packed and
 * are widened on the device INTO the ci8 ring (what enters is converted where it enters, as the ring's sign flip is): after a
 * packed upload the ring holds, byte for byte, what unpacking on the host followed by the unpacked namesake of the call would
 * have left, and nothing downstream of the ring changes.
 * A packing is `bits` in {1, 2, 4} per component, a field order and a table of 1 << bits int8 levels:
 *   fields per byte F = 8 / bits; samples per byte SPB = 4 / bits (4, 2, 1);
 *   sample k of a slab has component c (0 = I, 1 = Q) in field j = 2k + c: byte j / F, position p = j % F;
 *   the field sits at bit bits * p of its byte (least significant field first), or at bits * (F - 1 - p) with SDR_PACK_MSB_FIRST;
 *   code = (byte >> shift) & ((1 << bits) - 1), value = levels[code] -- any int8, -128 included.
 * n_samples of a packed slab is a multiple of SPB; the slab occupies n_samples * 2 * bits / 8 bytes from any byte address.
 * The packing travels with every call: the engine keeps none.  Each call is its unpacked namesake with one more step and keeps
 * that namesake's contract: sdr_iq_upload_packed is synchronous; _begin has copied the slab before it returns (up to 1 MiB of
 * packed bytes through the page-locked staging halves, longer ones by waiting; a block of sdr_host_alloc on a 16-byte boundary
 * whose destination is whole 16-byte ring granules is read in place under the rule stated for sdr_iq_upload_begin) and is
 * ordered before what is queued afterwards; _queue leaves the block with the caller until sdr_engine_sync: a copy command
 * brings the packed bytes into a staging buffer in HBM (the engine's, grown on demand, released with the ring) and the unpack
 * kernel follows it on the engine's stream.  Any ring_offset >= 0, taken modulo the capacity, wrapping at the ring's end;
 * n_samples up to the capacity.  Readers on other streams are ordered behind the unpack, not only behind the copy.
 * A packed slab is never parked for the tick's own launch or the resident tick server's doormen (those pull raw granules): a
 * slab parked earlier goes into the ring first, a resident server is told to leave, and the unpack is a launch of its own in
 * front of the tick's.  Folding the unpack into the tick's launch is not done here.
 * SDR_ERR_INVALID: NULL arguments, bits not 1 / 2 / 4, unknown flag bits, n_samples not a multiple of SPB;
 * SDR_ERR_UNSUPPORTED: the ring is not SDR_FMT_CI8; SDR_ERR_RANGE / SDR_ERR_STATE as sdr_iq_upload gives them.
 * sdr_prof_enable scopes: "unpack_kernel", "call_upload_packed". */
#define SDR_PACK_MSB_FIRST 1
typedef struct sdr_iq_packing {
    int32_t bits, flags;
    int8_t levels[16];    /* the first 1 << bits are used */
} sdr_iq_packing;
/* Bytes n_samples occupy packed (host helper like sdr_pcps_bins; < 0: invalid packing or sample count). */
int64_t sdr_iq_packed_bytes(const sdr_iq_packing* pk, int64_t n_samples);
int sdr_iq_upload_packed(sdr_engine* e, const sdr_iq_packing* pk, const void* packed, int64_t n_samples, int64_t ring_offset);
int sdr_iq_upload_packed_begin(sdr_engine* e, const sdr_iq_packing* pk, const void* packed, int64_t n_samples, int64_t ring_offset);
int sdr_iq_upload_packed_queue(sdr_engine* e, const sdr_iq_packing* pk, const void* packed, int64_t n_samples, int64_t ring_offset);

/* ------------------------------------------------- down-conversion and decimation into the ring
 * A digital down-converter (mixer, FIR low-pass, decimator) between the host's slab and the ring, for real or complex
 * recordings at an intermediate frequency and for wide-band recordings (50 MHz where the channels need 10 MHz): converted where
 * the samples enter the ring, nothing downstream of the ring changes.  The NumPy form of what follows is
 * sydr_amd/signal/downconvert.py `statement`; it is the only yardstick.
 * A converter has an input format, a decimation D in 1..64, T in 1..512 taps h[0..T-1] (doubles), a frequency word and a gain:
 *   fcw = round(shift_hz / fs_in * 2^64) mod 2^64      (unsigned, 2^-64 turns per INPUT sample; exact rational arithmetic)
 * Inputs are counted j = 0, 1, ... from creation or reset, across pushes; x_j is the sample as a complex number (imaginary part
 * 0 for real formats), x_j = 0 for j < 0:
 *   p_j = (j * fcw) mod 2^64                           (uint64 wrap)
 *   t_j = (p_j >> 11) * 2^-53                          (exact in a double, in [0, 1))
 *   z_j = x_j * (cos 2 pi t_j - i sin 2 pi t_j)
 *   v_m = gain * sum_{k < T} h_k * z_{m D - k}         m = 0, 1, ...   (fp64; k ascending, product then sum)
 * A push of n_in inputs whose first has index N writes exactly the outputs m with N <= m D < N + n_in, in order, at ring samples
 * (ring_offset + i) mod capacity, and nothing else.  A cf64 ring stores v, a cf32 ring v rounded to nearest float, an integer
 * ring clip(rint(v)) (ties to even; clip +-127 for ci8, +-32767 for ci16).  T = 1, h = {1}, D = 1, fcw = 0, gain = 1 leaves a
 * real recording as (r, 0) exactly.  The converter keeps the last T - 1 RAW inputs as its history and the phasor is a function
 * of j alone: what the ring holds does not depend on how the stream was cut into pushes, bit for bit, float rings included.
 * The group delay (T - 1) / 2 input samples of a symmetric filter is the caller's to account for.
 * sdr_ddc_push keeps sdr_iq_upload's host-buffer contract (synchronous; `in` is the caller's again on return),
 * sdr_ddc_push_queue that of sdr_iq_upload_queue (one copy command into a staging buffer of the engine in HBM, the kernels
 * behind it on the engine's stream, no wait: `in` stays valid and unchanged until sdr_engine_sync or a later synchronous call
 * returns).  *n_out (nullable) = the outputs written = what sdr_ddc_out_count said before the call (host arithmetic on the
 * converter's count of inputs).  Like every call but the tick's own, a push sends a resident tick server away and puts a parked
 * slab into the ring first.
 * SDR_ERR_INVALID: NULL arguments, D outside 1..64, T outside 1..512, a non-finite tap or gain, an unknown format, non-zero
 * flags, n_in < 0, a converter of another engine; SDR_ERR_STATE: no ring; SDR_ERR_RANGE: more outputs than the ring holds,
 * ring_offset outside 0 .. capacity - 1.  n_in = 0 succeeds and writes nothing.  A refused push changes neither the ring nor
 * the converter.  sdr_prof_enable scopes: "ddc_kernel", "ddc_history_kernel", "call_ddc_push". */
enum sdr_ddc_input {
    SDR_DDC_IN_R8 = 0,   /* real int8                 */
    SDR_DDC_IN_R16 = 1,  /* real int16                */
    SDR_DDC_IN_CI8 = 2,  /* int8  I, int8  Q          */
    SDR_DDC_IN_CI16 = 3  /* int16 I, int16 Q          */
};
typedef struct sdr_ddc_cfg {
    int32_t in_fmt, decimation, n_taps, flags;   /* flags: 0 */
    uint64_t fcw;
    double gain;
    const double* taps;                          /* [n_taps]; copied by sdr_ddc_create */
} sdr_ddc_cfg;
typedef struct sdr_ddc sdr_ddc;
int sdr_ddc_create(sdr_engine* e, const sdr_ddc_cfg* cfg, sdr_ddc** out);
void sdr_ddc_destroy(sdr_engine* e, sdr_ddc* d);
/* History zero, j = 0 (ordered behind the pushes queued so far). */
int sdr_ddc_reset(sdr_engine* e, sdr_ddc* d);
int sdr_ddc_push(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t ring_offset, int64_t* n_out);
int sdr_ddc_push_queue(sdr_engine* e, sdr_ddc* d, const void* in, int64_t n_in, int64_t ring_offset, int64_t* n_out);
int64_t sdr_ddc_out_count(const sdr_ddc* d, int64_t n_in);

/* ------------------------------------------------- rational-rate resampling in the converter (interpolate by L, decimate by M)
 * sdr_ddc_create_rational makes a converter that moves a recording between rates whose ratio is L / M: a 16.368 MHz recording
 * enters the ring at 12 MHz with L / M = 250 / 341.  cfg->decimation is M, cfg->n_taps is T, the length of the prototype filter
 * h[0..T-1] at the UP-SAMPLED rate (L times the input's); everything else of cfg is as above.  The mixer is unchanged: p_j, t_j and
 * z_j are functions of the INPUT index j alone.  For output m = 0, 1, ...:
 *   u = m * M      q = u div L      p = u mod L      K_p = ceil((T - p) / L)   (0 when p >= T)
 *   v_m = gain * sum_{k < K_p} h[p + k L] * z_{q - k}   (fp64; k ascending, product then sum, no contraction; z_j = 0 for j < 0)
 * -- zero-stuffing by L, the filter, every M-th sample kept, of which only the non-zero products are formed, in a fixed order;
 * K_p = 0 gives gain * 0.0.  A push of n_in inputs whose first has index N writes exactly the outputs m with
 * N L <= m M < (N + n_in) L (that is N <= q_m < N + n_in): sdr_ddc_out_count = ceil((N + n_in) L / M) - ceil(N L / M), in host
 * arithmetic.  The history is the last ceil(T / L) - 1 RAW inputs; the ring does not depend on how the stream was cut into pushes,
 * bit for bit.  The group delay of a symmetric prototype is (T - 1) / (2 L) input samples = (T - 1) / (2 M) output samples.
 * Limits: L in 1..1024, M in 1..1024 with M <= 64 L, T in 1..32768 with ceil(T / L) <= 512 (SDR_ERR_INVALID otherwise, on top of
 * sdr_ddc_create's causes).  interpolation == 1 IS sdr_ddc_create(e, cfg, out): the same limits, kernels, launches and bytes.
 * Every other sdr_ddc_* call takes the handle as it takes sdr_ddc_create's -- reset, push, push_queue, out_count, destroy, and
 * sdr_ddc_mitigate / _delay / _mitigation_stats below, the mitigator sitting on the stream v_m.  A push that would take
 * (N + n_in) * L to 2^62 is refused with SDR_ERR_RANGE (sdr_ddc_out_count returns it too); a refused call changes nothing.
 * sdr_prof_enable scopes of a converter with L > 1: "resample_kernel", "ddc_history_kernel" (the integer converter's, saving
 * ceil(T / L) - 1 inputs), "call_ddc_push". */
int sdr_ddc_create_rational(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, sdr_ddc** out);

/* ------------------------------------------------- input layouts: packed, float32 and interleaved recordings through the converter
 * sdr_ddc_create_layout makes a converter whose inputs are described by an INPUT LAYOUT in place of an sdr_ddc_input: how the
 * recording's bytes hold the samples.  The kernels decode the layout where they load their inputs; the push stages the bytes as
 * they are (one copy command of sdr_ddc_layout_bytes bytes: a packed recording stays packed over the link and in HBM).  The NumPy
 * form is sydr_amd/signal/downconvert.py `decode`.
 * Fields.  A recording is a sequence of fields f = 0, 1, ..., one component each, of one kind: INT8, INT16 (native byte order),
 * FLOAT32 (native) or PACKED, a code of `bits` bits, bits one of 1, 2, 4.  With F = 8 / bits, field f of a packed recording lies
 * in byte f div F at position p = f mod F: its code is the `bits` bits from bit bits * p up (least significant field first) or,
 * with MSB_FIRST, from bit bits * (F - 1 - p) up; the component is levels[code], an int8 (sdr_iq_packing's rule, field for
 * field).  Every component is widened to fp64, which is exact for all four kinds.
 * Frames.  A frame is `stride` consecutive fields; input j of the stream is frame j:
 *   real:                 x_j = field(j * stride + lane) + 0i
 *   COMPLEX:              a = field(j * stride + lane), b = field(j * stride + lane + 1), x_j = a + ib
 *   COMPLEX | SWAP_IQ:    x_j = b + ia
 * From x_j on everything is the converter's statement above (p_j, t_j, z_j, v_m, the resampler's form, the mitigator, the
 * ring's formats).  Frames of a packed layout need not be whole bytes: a 1-bit real stream with stride 3 is valid.
 * Limits (SDR_ERR_INVALID otherwise): stride in 1..64; lane >= 0 and lane + (COMPLEX ? 2 : 1) <= stride; bits 1, 2 or 4 exactly
 * when the kind is PACKED and 0 otherwise; SWAP_IQ only with COMPLEX; MSB_FIRST only with PACKED; no other flag bit, reserved 0.
 * Pushes.  n_in counts frames and `in` points at the first byte of the push's first frame.  A push reads
 * B = n_in * stride * (bytes per field) bytes, of a packed layout B = n_in * stride * bits / 8, which must be a whole number:
 * otherwise the push is refused with SDR_ERR_INVALID and neither the ring nor the converter changes -- every push begins on a
 * byte boundary.  sdr_ddc_out_count, the kept inputs (the last Tp - 1, held DECODED: this stream's components alone, int8, int16 or
 * float32, one or two per input, zeros after creation or reset) and the promise that the ring does not depend on the cut, bit
 * for bit, are the converter's as before.
 * Float inputs are the caller's to keep finite: a NaN or Inf input may change only the outputs whose filter window contains it
 * (with a mitigator: the outputs of the segments that contain it), to unspecified values; every other output is what it would
 * be with that input replaced by 0.
 * Bit for bit, in every ring format: the layouts {INT8 real, stride 1, lane 0}, {INT16 real, 1, 0}, {INT8 COMPLEX, 2, 0} and
 * {INT16 COMPLEX, 2, 0} give the ring of SDR_DDC_IN_R8, _R16, _CI8 and _CI16; a packed layout gives the ring the matching INT8
 * layout gives on the unpacked bytes; a float32 recording that holds integers within int16 gives the ring of the INT16 layout.
 * cfg is as for sdr_ddc_create_rational (cfg->in_fmt is not read), interpolation == 1 the integer converter.  Every other
 * sdr_ddc_* call takes the handle as it takes any converter's.  Scopes: those of the converter ("ddc_kernel" / "resample_kernel",
 * "ddc_history_kernel", "call_ddc_push").  A converter of sdr_ddc_create / _rational makes the launches it always made. */
enum sdr_ddc_field { SDR_DDC_FIELD_INT8 = 0, SDR_DDC_FIELD_INT16 = 1, SDR_DDC_FIELD_FLOAT32 = 2, SDR_DDC_FIELD_PACKED = 3 };
#define SDR_DDC_LAYOUT_COMPLEX   1
#define SDR_DDC_LAYOUT_SWAP_IQ   2
#define SDR_DDC_LAYOUT_MSB_FIRST 4
typedef struct sdr_ddc_layout {
    int32_t field, bits, stride, lane, flags, reserved;
    int8_t  levels[16];          /* PACKED: the first 1 << bits are read */
} sdr_ddc_layout;
/* cfg as for sdr_ddc_create_rational (cfg->in_fmt is not read); interpolation == 1: the integer converter */
int sdr_ddc_create_layout(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, const sdr_ddc_layout* layout, sdr_ddc** out);
/* bytes a push of n_in frames reads (host arithmetic, like sdr_iq_packed_bytes); SDR_ERR_INVALID for a bad layout, n_in < 0 or a
 * packed push that is not whole bytes */
int64_t sdr_ddc_layout_bytes(const sdr_ddc_layout* layout, int64_t n_in);

/* ------------------------------------------------- antenna arrays: the elements of a multi-element recording combined in the converter
 * sdr_ddc_create_array makes a converter over a recording that interleaves the K elements of an antenna array, K in 2..8: the
 * kernels decode the K elements of a frame where they load it and hand the mixer ONE input, x = w^H s -- with weights that put a
 * null on a broadband jammer (power inversion, MVDR) the defence the blanker and the excisor cannot give.  Nothing downstream of
 * the ring changes and the recording crosses the link and lies in HBM as it is, packed if it is packed.  The NumPy form of what
 * follows is sydr_amd/signal/array.py `statement`; it is the only yardstick.
 * An array is an input layout (above) plus K elements, element a at lane lanes[a] of the frame: distinct lanes, each with
 * lanes[a] >= 0 and lanes[a] + (COMPLEX ? 2 : 1) <= stride, in any order, adjacent or not; layout->lane is not read.  Element a
 * of frame j is decoded exactly as the layout decodes a stream at that lane: s_a = sr_a + i si_a (si = 0 of a real layout,
 * SWAP_IQ honoured).  With weights w_a = wr_a + i wi_a = weights[a][0] + i weights[a][1], finite doubles, the converter's input
 * j is x_j = sum_a conj(w_a) s_a, formed in fp64 in this order and no other, every product and every sum rounded, no contraction:
 *   re = 0; im = 0
 *   for a = 0 .. K-1:   re = re + wr_a sr_a;  re = re + wi_a si_a;  im = im + wr_a si_a;  im = im - wi_a sr_a
 * From x_j on everything is the converter's statement above (p_j, t_j, z_j, v_m, the resampler's form, the mitigator, the
 * ring's formats).  Weights belong to input indices: sdr_ddc_array_weights takes effect with the first input of the next push
 * (it is ordered on the engine's stream behind the pushes queued so far), earlier inputs keep the x_j they had -- the history
 * holds the last Tp - 1 COMBINED inputs as cf64 -- so with the weight changes at the same input indices the ring does not depend
 * on how the stream was cut into pushes, bit for bit.  Bit for bit too, in every ring format: the weights e_a (1 at a, 0
 * elsewhere) give the ring of sdr_ddc_create_layout with lane = lanes[a]; a packed array gives the ring of the INT8 array on the
 * unpacked bytes.  The C-ABI takes weights and does not solve for them (sydr_amd/signal/array.py has the two usual rules).
 * Covariance (flags = SDR_DDC_ARRAY_MEASURE; one more pass over the staged bytes of every push).  Over the inputs j pushed
 * since creation, reset or the last clearing read:
 *   R[a][b] = sum_j s_a conj(s_b):   re = sum (sr_a sr_b + si_a si_b),   im = sum (si_a sr_b - sr_a si_b),   n = their number
 * For INT8, INT16 and PACKED fields the sums are exact 64-bit integers, each converted to double once at the read: the same
 * numbers on every run and those of the statement, equal, not close.  For FLOAT32 fields the device adds in fp64 in a fixed
 * order of its own (the same pushes give the same bits); a component differs from the statement's by at most
 * 2 n 2^-52 sum_j (|sr_a sr_b| + |si_a si_b|) and correspondingly for the imaginary part.  sdr_ddc_array_covariance waits for
 * the engine's stream and writes R as [K][K][2] doubles (row a, column b, re then im; the lower triangle the conjugate of the
 * upper) and *n; clear != 0 zeroes both behind the read.
 * sdr_ddc_reset zeroes the history and the covariance and keeps the weights.  Every other sdr_ddc_* call takes the handle as it
 * takes any converter's: reset, push, push_queue, out_count, destroy, mitigate, delay, mitigation_stats, and
 * sdr_ddc_layout_bytes (of the layout) says the bytes of a push.
 * SDR_ERR_INVALID: NULL arguments, n_elements outside 2..8, a repeated or out-of-frame lane, a non-finite weight, an unknown
 * flag, a layout outside its limits, every cause of sdr_ddc_create_layout's cfg, and a converter without an array passed to
 * sdr_ddc_array_weights or sdr_ddc_array_covariance; SDR_ERR_STATE: sdr_ddc_array_covariance on a converter made without
 * SDR_DDC_ARRAY_MEASURE.  A refused call changes nothing.  Scopes: those of the converter ("ddc_kernel" / "resample_kernel",
 * "ddc_history_kernel", "call_ddc_push") and "ddc_array_cov_kernel" for the covariance pass.  A converter of sdr_ddc_create,
 * sdr_ddc_create_rational or sdr_ddc_create_layout makes exactly the launches, and writes exactly the bytes, it always made. */
#define SDR_DDC_ARRAY_MEASURE 1
typedef struct sdr_ddc_array {
    int32_t n_elements, flags;   /* K in 2..8; flags: 0 or SDR_DDC_ARRAY_MEASURE */
    int32_t lanes[8];            /* the first K are read */
    double weights[8][2];        /* w_a = weights[a][0] + i weights[a][1]; the first K are read */
} sdr_ddc_array;
/* cfg, interpolation and layout as for sdr_ddc_create_layout (layout->lane is not read) */
int sdr_ddc_create_array(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, const sdr_ddc_layout* layout, const sdr_ddc_array* array,
                         sdr_ddc** out);
/* w = [K][2]; from the next push on; ordered on the stream */
int sdr_ddc_array_weights(sdr_engine* e, sdr_ddc* d, const double* w);
/* R = [K][K][2]; waits for the stream */
int sdr_ddc_array_covariance(sdr_engine* e, sdr_ddc* d, double* R, int64_t* n, int clear);

/* ------------------------------------------------- space-time adaptive weights (STAP): a short FIR per element of an array converter
 * sdr_ddc_create_stap makes an array converter (above) with K x T weights in place of K, T in 1..8: a T-tap FIR per element in
 * front of the mixer.  The time taps give nulls that depend on frequency -- two elements remove several partial-band or
 * narrow-band jammers from different directions, which K - 1 spatial nulls cannot -- and absorb the elements' differing channel
 * responses.  Nothing downstream of the ring changes.  The NumPy form of what follows is sydr_amd/signal/stap.py `Statement`; it
 * is the only yardstick.
 * A space-time array is an array (layout, K lanes: array->n_elements, lanes, flags; array->weights is not read) plus T = n_taps
 * taps.  Weights are w[t][a] = w[2 (t K + a)] + i w[2 (t K + a) + 1], t = 0..T-1, a = 0..K-1, finite doubles, laid out [T][K][2].
 * s_a[i] is element a of frame i, decoded exactly as the array converter decodes it, and 0 for every i before the first input
 * since creation or sdr_ddc_reset.  The converter's input j is x_j = sum_t sum_a conj(w[t][a]) s_a[j - t], formed in fp64 with one
 * running pair that starts at +0.0, t ascending and inside each t a ascending, the array converter's four operations per (t, a),
 * every product and every sum rounded, no contraction:
 *   re = 0; im = 0
 *   for t = 0 .. T-1:  for a = 0 .. K-1:  (sr, si) = s_a[j - t]
 *       re = re + wr sr;  re = re + wi si;  im = im + wr si;  im = im - wi sr
 * From x_j on everything is the converter's statement (p_j, t_j, z_j, v_m, the resampler's form, the mitigator, the ring's
 * formats).  Weights belong to input indices: sdr_ddc_stap_weights takes effect with the first input of the next push, for all T
 * taps of that input (it is ordered on the engine's stream behind the pushes queued so far, which keep the weights they were
 * queued with); earlier x_j, those in the FIR's history included, keep their values -- the history holds the last Tp - 1 COMBINED
 * inputs as cf64 -- and the raw elements of the last T - 1 frames are carried across pushes beside it.  With the weight changes at
 * the same input indices the ring does not depend on how the stream was cut into pushes, bit for bit.  T = 1 gives the ring of
 * sdr_ddc_create_array with the same weights; the weight e_a at tap t0 alone gives the ring of sdr_ddc_create_layout with
 * lane = lanes[a] on the stream with t0 zero frames prepended.  The C-ABI takes weights and does not solve for them
 * (sydr_amd/signal/stap.py has power inversion and MVDR on the space-time covariance).
 * Lag covariance (array->flags = SDR_DDC_ARRAY_MEASURE; one more pass of T lags over the staged bytes of every push).  For
 * tau = 0..T-1, over the inputs j pushed since creation, reset or the last clearing read, n their number:
 *   C[tau][a][b] = sum_j s_a[j] conj(s_b[j - tau]):   re = sum (sr_a sr_b' + si_a si_b'),   im = sum (si_a sr_b' - sr_a si_b')
 * (sr_b', si_b') = s_b[j - tau] being the real earlier input when one has been pushed since creation or reset -- before a
 * clearing read too -- and zero otherwise.  For INT8, INT16 and PACKED fields the sums are exact 64-bit integers, each converted
 * to double once at the read: those of the statement, equal, not close.  For FLOAT32 fields the device adds in fp64 in a fixed
 * order of its own (the same pushes give the same bits); a component differs from the statement's by at most
 * 2 n 2^-52 sum_j (|sr_a sr_b'| + |si_a si_b'|) and correspondingly for the imaginary part.  sdr_ddc_stap_covariance waits for
 * the engine's stream and writes C as [T][K][K][2] doubles and *n; clear != 0 zeroes both behind the read.
 * sdr_ddc_reset zeroes both histories and the covariance and keeps the weights.  sdr_ddc_delay keeps reporting the mitigator's
 * own delay: a caller whose weights pass the reference element at tap t0 adds t0 input samples itself.  Every other sdr_ddc_*
 * call takes the handle as it takes any converter's, sdr_ddc_mitigate included.
 * SDR_ERR_INVALID: every cause of sdr_ddc_create_array (array->weights aside), n_taps outside 1..8, w NULL, a non-finite weight,
 * sdr_ddc_stap_weights or sdr_ddc_stap_covariance on a converter not made by sdr_ddc_create_stap, and sdr_ddc_array_weights or
 * sdr_ddc_array_covariance on one that was; SDR_ERR_STATE: sdr_ddc_stap_covariance on a converter made without
 * SDR_DDC_ARRAY_MEASURE.  A refused call changes nothing.  Scopes: those of the converter and "ddc_stap_cov_kernel" for the lag
 * pass.  A converter of the four older constructors makes exactly the launches, and writes exactly the bytes, it always made. */
/* cfg, interpolation, layout and array as for sdr_ddc_create_array (array->weights is not read); w = [n_taps][K][2] */
int sdr_ddc_create_stap(sdr_engine* e, const sdr_ddc_cfg* cfg, int interpolation, const sdr_ddc_layout* layout, const sdr_ddc_array* array,
                        int n_taps, const double* w, sdr_ddc** out);
/* w = [T][K][2]; from the next push on; ordered on the stream */
int sdr_ddc_stap_weights(sdr_engine* e, sdr_ddc* d, const double* w);
/* C = [T][K][K][2]; waits for the stream */
int sdr_ddc_stap_covariance(sdr_engine* e, sdr_ddc* d, double* C, int64_t* n, int clear);

/* ------------------------------------------------- beams: several weight sets over one push, each into its own ring
 * An array or space-time converter decodes one recording; sdr_ddc_beam_attach gives it further weight sets -- a beam per
 * satellite, or the K element streams side by side -- without a second push: the push stages its bytes once (one copy command,
 * as ever), and every beam decodes them from HBM.  Beam 0 is the converter as it is: engine e, the weights of
 * sdr_ddc_array_weights / sdr_ddc_stap_weights.  Beam b >= 1 has a weight set of its own, of the converter's shape ([K][2], or
 * [T][K][2] of a space-time converter), and its output goes into the ring of `target`, another engine on the same device.
 * The definition needs no new arithmetic.  Take an independent converter on `target`, made with the same constructor arguments
 * and the weights w_b, given the same pushes at the same ring_offset and the same weight changes at the same input indices:
 * beam b's ring holds, byte for byte, what that converter writes -- in every ring format (a beam's ring has its own, any of the
 * four), whatever the cut into pushes.  The NumPy form is sydr_amd/signal/array.py `statement` / sydr_amd/signal/stap.py
 * `Statement` applied once per beam (`beams_statement` there).  What follows from it: every push writes the same number of
 * outputs at the same ring_offset of every beam's ring, and nothing else; sdr_ddc_beam_weights takes effect with the first
 * input of the next push (it is ordered on e's stream behind the pushes queued so far, which keep the weights they were queued
 * with); sdr_ddc_reset zeroes every beam's history of combined inputs and keeps every beam's weights; the raw tail of a
 * space-time converter holds elements, not beams, and is shared; the covariance pass (SDR_DDC_ARRAY_MEASURE) is unchanged, once
 * per push over the raw elements.
 * Attaching and clearing are allowed only while the converter has seen no input since creation or reset (SDR_ERR_STATE
 * otherwise, as for sdr_ddc_mitigate).  A mitigator and attached beams exclude each other: the mitigator's state is per stream
 * and a converter has one, so whichever of sdr_ddc_mitigate(cfg != NULL) and sdr_ddc_beam_attach comes second is refused with
 * SDR_ERR_UNSUPPORTED.  SDR_ERR_INVALID: NULL arguments (`beam`, the result, may be NULL), a converter that is neither an array
 * nor a space-time converter, a target on another device, without a ring, with a ring of another capacity than e's, target == e,
 * a target attached twice, more than SDR_DDC_MAX_BEAMS - 1 attached beams, a non-finite weight, a beam outside 1 .. count - 1.
 * A refused call changes nothing.
 * A push does for every target what it does for e: a resident tick server leaves, a slab parked for the next tick goes into the
 * ring first, and SDR_ERR_RANGE is checked before anything is queued; a target whose ring has been released or re-allocated at
 * another capacity since the attachment makes the push fail with SDR_ERR_STATE.  sdr_ddc_push_queue stays asynchronous: before
 * the beams' kernels write, e's stream waits for an event recorded on each target's stream (what the target queued on its ring
 * comes first); behind them each target's stream waits for an event recorded on e's stream, and the target's other streams order
 * themselves as they do behind its own uploads.  sdr_ddc_push returns once every beam's ring holds the push.
 * Destroying a target engine while it is attached is the caller's error: sdr_ddc_beams_clear or sdr_ddc_destroy release the
 * attachments first.  Scopes: the attached beams' one launch per push is "ddc_beam_kernel" / "resample_beam_kernel", their
 * histories are written inside "ddc_history_kernel"; "call_ddc_push" brackets everything.  A converter without attached beams
 * makes exactly the launches, and writes exactly the bytes, it always made. */
#define SDR_DDC_MAX_BEAMS 16            /* the converter's own stream included */
/* w: [K][2] (array converter) or [T][K][2] (space-time converter); *beam (nullable) = the new beam's index, 1 .. */
int sdr_ddc_beam_attach(sdr_engine* e, sdr_ddc* d, sdr_engine* target, const double* w, int* beam);
/* beam in 1 .. count - 1; from the next push on; ordered on the stream */
int sdr_ddc_beam_weights(sdr_engine* e, sdr_ddc* d, int beam, const double* w);
int sdr_ddc_beam_count(const sdr_ddc* d);          /* 1 + attached beams */
int sdr_ddc_beams_clear(sdr_engine* e, sdr_ddc* d);

/* ------------------------------------------------- pulse blanking and narrow-band excision in front of the ring
 * An opt-in stage of a converter, between the filter's fp64 output v and the ring's format: a threshold blanker against pulsed
 * interference (DME, radar, a switching supply) and a frequency-domain excisor with windowed overlap-add against carrier-wave
 * interferers.  Nothing downstream of the ring learns of it; a converter without it makes the launches and writes the bytes it
 * always did.  The NumPy form of what follows is sydr_amd/signal/mitigate.py `Statement`; it is the only yardstick.
 * v_m is the converter's output m = 0, 1, ... since creation or reset (above), v_m = 0 for m < 0.
 * Blanker (blank_level > 0; blank_lead, blank_hold in 0..1024 samples, taken as 0 without a blanker):
 *   p_m = re*re + im*im                               (two products, one sum, each rounded)
 *   t_m = p_m > blank_level * blank_level             (the square formed once, on the host)
 *   b_m = any t_j with m - blank_hold <= j <= m + blank_lead
 *   u_m = 0 where b_m, else v_m
 * Excisor (nfft = N, a power of two in 64..4096; limit[k] >= 0, k < N in FFT order, +inf allowed), hop H = N / 2, periodic Hann
 * window w[j] = 0.5 - 0.5 cos(2 pi j / N) (sdr_iq_probe's; w[j] + w[j + H] = 1), segment s >= -1 = u[s H .. s H + N):
 *   A_s = FFT(w * u_s);  P = re^2 + im^2 of A_s[k];  G[k] = 0 where P > limit[k], else 1;  B_s = IFFT(G * A_s)   (1 / N included)
 *   y_m = B_{q-1}[m - (q-1) H] + B_q[m - q H],  q = floor(m / H)        (y = u without the excisor)
 * Delay L = (N with the excisor, else 0) + blank_lead: output i of the stream is format(y_{i - L}) and format(0) for i < L, format
 * being the converter's (cf64 as is, cf32 rounded, integer rings clip(rint), a ci8 ring's bytes sign-flipped).  A push of n_in
 * inputs writes exactly the outputs the converter alone would (sdr_ddc_out_count unchanged) at the same ring samples; the
 * constant delay of L ring samples, common to all channels, is reported (sdr_ddc_delay) and not compensated -- as the filter's
 * group delay.  The tail of a stream comes out when the caller pushes L more zeros; there is no flush call.  The mitigator keeps
 * the last 2 N - 1 + blank_lead + blank_hold values of v (blank_lead + blank_hold without the excisor) and a segment's transform
 * is a function of its N inputs alone: what the ring holds does not depend on how the stream was cut into pushes, bit for bit.
 * Against the statement the device's y differs by at most 16 log2(N) N 2^-53 max|u| per component (two radix-2 transforms
 * against NumPy's) plus what the converter's own tolerance becomes; a gate is a discontinuity, so a bin or a sample within
 * that of its limit may fall on either side.
 * Counters, since creation or reset, functions of the number n of outputs delivered alone (so they do not depend on the cut):
 *   n_outputs = n;  n_triggers = #{0 <= j < n - L : t_j};  n_blanked = #{0 <= m < n - L : b_m};
 *   n_segments = #{s >= -1 : s H + N <= n - L} (finished segments);  bins[k] = #{finished segments with G[k] = 0};
 *   n_bins_excised = sum of bins.
 * sdr_ddc_mitigate attaches a mitigator (cfg is copied, limit included) or, with cfg == NULL, detaches it; either only while the
 * converter has seen no input since creation or reset (SDR_ERR_STATE otherwise).  sdr_ddc_reset clears the mitigator's state and
 * counters too.  sdr_ddc_mitigation_stats waits for the engine's stream; SDR_ERR_STATE without a mitigator.
 * SDR_ERR_INVALID: nfft neither 0 nor a power of two in 64..4096, blank_lead or blank_hold outside 0..1024, a negative or NaN
 * limit or blank_level, nfft > 0 with limit == NULL, non-zero flags, both stages off (nfft = 0 and blank_level = 0).  A refused
 * call changes nothing.  sdr_prof_enable scopes: "mit_blank_kernel", "mit_excise_kernel", "mit_combine_kernel". */
typedef struct sdr_mit_cfg {
    int32_t nfft, blank_lead, blank_hold, flags; /* flags: 0 */
    double blank_level;
    const double* limit;                         /* [nfft]; copied by sdr_ddc_mitigate */
} sdr_mit_cfg;
typedef struct sdr_mit_stats {
    int64_t n_outputs, n_triggers, n_blanked, n_segments, n_bins_excised;
} sdr_mit_stats;
int sdr_ddc_mitigate(sdr_engine* e, sdr_ddc* d, const sdr_mit_cfg* cfg);   /* NULL detaches */
int64_t sdr_ddc_delay(const sdr_ddc* d);                                   /* L; 0 without a mitigator */
int sdr_ddc_mitigation_stats(sdr_engine* e, sdr_ddc* d, sdr_mit_stats* stats, int64_t* bins /* nullable [nfft] */);

/* ------------------------------------------------- what the ring holds: levels, histogram, spectrum
 * The first look at a new recording and the look a running receiver keeps taking at its front end -- are the bits used, is
 * anything on the rails, is there a DC offset or an I/Q imbalance, is the level table of a packed file the right one, is there
 * a carrier-wave interferer in the band, where does the noise floor sit -- taken where the samples lie: one pass over the
 * window on the device, a few kilobytes back (the reference only had an off-line Welch plot, sydr/old/dsplib.py:100-110).
 * The window is ring samples start_sample .. start_sample + n_samples - 1: any start_sample >= 0, taken modulo the capacity;
 * the window may cross the ring's end; 1 <= n_samples <= min(capacity, 2^31).  Synchronous on the engine's stream, behind every
 * ring write queued before it (sdr_iq_upload_begin / _queue, the packed uploads and their unpack kernels, a parked slab).  The
 * call reads the ring and writes nothing into it; two identical calls return identical bits.  A probe is a call of its own,
 * not a part of the tick's launch: like every non-tick call it tells a resident tick server to leave first.
 * Moments, integer rings (ci8, ci16): every sum is the exact integer, accumulated in 64-bit integers and converted to double
 * once at the end (round to nearest even); min / max exact; n_rail counts the components equal to -128 / 127 (ci8) or
 * -32768 / 32767 (ci16).  A ci8 ring stores its bytes sign-flipped; the call reports the samples' values.
 * Moments, float rings (cf32, cf64): a sample with a NaN / Inf component is counted in n_nonfinite and left out of everything
 * else; the sums are fp64, added in a fixed order; min / max exact (NaN when no finite sample is left); n_rail = 0.
 * Histogram (hist != NULL, integer rings only): hist[c][b] counts the components c (0 = I, 1 = Q) whose bin is
 *   b = min(255, max(0, (value >> hist_shift) + 128))    (arithmetic shift; hist_shift 0 for ci8, 0..8 for ci16).
 * Power spectral density (psd != NULL): Welch's method, segments of nfft samples (a power of two in 64..4096), hop nfft / 2:
 *   S = (n_samples - nfft) / (nfft / 2) + 1 segments (integer division; what lies behind the last whole one is not used),
 *   the periodic Hann window w[j] = 0.5 - 0.5*cos(2*pi*j/nfft), no detrending (a DC offset is something to see), fp64:
 *   psd[k] = ( sum_s |FFT(w * x_s)[k]|^2 ) / (S * fs * sum_j w[j]^2),   k = 0..nfft-1 in FFT order
 *   (bin k stands for k*fs/nfft below nfft/2 and for (k-nfft)*fs/nfft from there on) -- scipy.signal.welch(x, fs, 'hann',
 *   nfft, nfft//2, detrend=False, return_onesided=False, scaling='density').  A non-finite sample in a used segment makes
 *   every psd[k] NaN (reported, not guessed); the moments are still reported.
 * SDR_ERR_INVALID: NULL e or res, n_samples < 1, a negative hist_shift or one too large for the ring, and with psd != NULL an
 * nfft that is no power of two in 64..4096, fs <= 0 or non-finite, n_samples < nfft; SDR_ERR_UNSUPPORTED: hist != NULL on a
 * float ring, n_samples > 2^31 (whatever the ring holds); SDR_ERR_RANGE: a negative start_sample, a window longer than the
 * ring; SDR_ERR_STATE: no ring.  A refused call leaves res, hist and psd untouched.
 * sdr_prof_enable scopes: "probe_moments_kernel", "probe_psd_kernel" (with its row reduction), "call_iq_probe". */
typedef struct sdr_probe_result {
    int64_t n_samples;      /* samples of the window                                                        */
    int64_t n_segments;     /* Welch segments averaged (0 when psd == NULL)                                 */
    int64_t n_nonfinite;    /* float rings: samples with a NaN / Inf component; they enter no sum, min, max  */
    int64_t n_rail[2];      /* integer rings: I / Q components equal to the type's minimum or maximum        */
    double  min[2], max[2]; /* I, Q                                                                          */
    double  sum[2];         /* sum I, sum Q                                                                  */
    double  sum_sq[2];      /* sum I*I, sum Q*Q                                                              */
    double  sum_iq;         /* sum I*Q                                                                       */
} sdr_probe_result;
int sdr_iq_probe(sdr_engine* e, int64_t start_sample, int64_t n_samples, int hist_shift, int nfft, double fs,
                 sdr_probe_result* res, int64_t* hist /* nullable [2][256] */, double* psd /* nullable [nfft] */);

/* Host-only helper of a receiver that tracks ahead (no device work): `records[n_ch][n_cols]` hold `done[r]` epochs per channel
 * computed in one sdr_bank_step while the host still feeds its per-millisecond loop (receiver.py:120-131); this works out
 * which tick releases which epoch -- the first tick k whose slab completes it (channel.py:137-146): unread_now[r] +
 * (k + 1) * samples_per_tick >= the samples up to its end, one epoch per channel and tick (channelManager.py:149-188) -- and
 * what every tick's CHANNEL_UPDATE reports (channel.py:205-228).  Outputs (caller-allocated): first[n_ch][n_cols] = the tick
 * of each epoch (-1: not run); *n_ticks; the epochs in tick order (channels ascending inside a tick) as order_rows /
 * order_cols / records_sorted [sum of done], tick k's slice being [starts[k], starts[k + 1]) (starts: max_ticks + 1 entries);
 * last_records[n_ch] = each channel's newest record; per tick and channel [max_ticks][n_ch] (row stride n_ch): unread samples
 * after the tick, the device's TrackingFlags bits (flags0 before the channel's first epoch) and code_since0 + epochs released
 * so far; last_tick[n_ch] = the tick of each channel's last epoch (-1: none); the navigation bits the block decided, channel by
 * channel in epoch order: bit_rows / bit_cols / bit_values [up to sum of done], *n_bits of them.  SDR_ERR_RANGE when an epoch
 * would fall beyond max_ticks. */
int sdr_block_schedule(const sdr_track_epoch* records, int n_ch, int n_cols, const int32_t* done, const int64_t* unread_now,
                       int64_t samples_per_tick, const int64_t* flags0, const int64_t* code_since0, int max_ticks,
                       int32_t* first, int32_t* n_ticks, int32_t* order_rows, int32_t* order_cols, int32_t* starts,
                       sdr_track_epoch* records_sorted, sdr_track_epoch* last_records, int64_t* unread, int64_t* dev_flags,
                       int64_t* code_count, int32_t* last_tick, int32_t* bit_rows, int32_t* bit_cols, int32_t* bit_values,
                       int32_t* n_bits);

/* ------------------------------------------------- streams (one per channel batch)
 * north_star: "one HIP stream per channel batch".  Stream ids are small positive integers owned by the engine;
 * 0 always names the engine's default stream. */
int sdr_stream_create(sdr_engine* e, int* stream_id);
int sdr_stream_sync(sdr_engine* e, int stream_id);
/* sdr_epl_plan_run_range on a chosen stream (asynchronous; sdr_stream_sync or sdr_epl_plan_fetch completes it). */
int sdr_epl_plan_run_range_on(sdr_engine* e, sdr_epl_plan* p, int64_t first, int64_t count, int stream_id);
/* Diagnostics: which correlator variant the plan's items selected -- 0 per-sample, 8 / 16 boundary variant with that
 * many samples per lane, 26 chip-aligned; + KM when the block length is compiled in (every epoch KM.x samples per chip,
 * KM = 16 .. 25; 15 on the half-chip view) and with it + 256 * floor(KM / 2) when the outer taps' switch position is too
 * (three taps half a chip apart: both switch floor(KM / 2).x samples into the prompt tap's chip) or + 4096 when the taps sit
 * whole (half-)chips apart; 26 + 16 alone: two block lengths compiled in (every epoch 15.x or 16.x samples per chip:
 * 16.368 MHz); + 8192 * k: several chips per lane (k = 1, 2: two chips of 9.5 - 10 / 11.5 - 12 samples; k = 3: four of 3.75 - 4);
 * + 65536 when the plan runs on the half-chip view of its replicas (32-52 samples per chip: every chip twice).  The
 * results do not depend on it beyond the tolerance of the free arithmetic. */
int sdr_epl_plan_variant(const sdr_epl_plan* p);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* SYDR_AMD_H */
