/*
 * mi_airband.h -- C ABI of the MI355X-native channelizer/demodulator (libmi_airband.so).
 *
 * This is the drop-in boundary for ONE path of Boondock-Airband: the body of demodulate()
 * (reference src/rtl_airband.cpp:308-694) -- sample conversion x window, sliding FFT, bin pick,
 * and the per-channel squelch / AM / NFM / CTCSS / filter loop -- between the reference's two
 * shared-memory contracts: the input_t byte ring upstream (src/input-common.h:39-57) and
 * channel_t.{waveout, iq_out, axcindicate} + device_t.waveavail downstream
 * (src/boondock_airband.h:243-297).  Plain pointers and sizes only; no C++ types, no exceptions,
 * never exits the process.  Every function returns 0 on success or a negative mi_status;
 * mi_last_error() gives the message (the reference's own convention for inputs is int 0/-1,
 * src/input-common.cpp:56-131; its VideoCore FFT seam returns -1/-2/-3, src/rtl_airband.cpp:318-332).
 *
 * Precedent seam in the reference: gpu_fft_prepare/gpu_fft_execute/gpu_fft_release
 * (src/hello_fft/gpu_fft.h:60-74) + samplefft() (src/boondock_airband.h:87-92).  This ABI replaces
 * the whole batch body, not only the FFT, so nothing but u8 IQ goes down and audio comes up.
 */
#ifndef MI_AIRBAND_H
#define MI_AIRBAND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* build-time constants of the reference's NFM build (src/boondock_airband.h:64-75) */
#define MI_WAVE_RATE 16000
#define MI_WAVE_BATCH 2000
#define MI_AGC_EXTRA 100

typedef enum {
    MI_OK = 0,
    MI_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    MI_ERR_NO_DEVICE = -2,   /* HIP runtime or GPU missing: the product path never falls back to CPU */
    MI_ERR_NOMEM = -3,       /* host or device allocation failed */
    MI_ERR_HIP = -4,         /* a HIP call or kernel launch failed */
    MI_ERR_UNSUPPORTED = -5  /* valid in the reference, not built in this library */
} mi_status;

enum { MI_MOD_AM = 0, MI_MOD_NFM = 1 };                                        /* enum modulations, boondock_airband.h:202-208 */
enum { MI_SFMT_U8 = 1, MI_SFMT_S8 = 2, MI_SFMT_S16 = 3, MI_SFMT_F32 = 4 };     /* sample_format_t, input-common.h:31 */
enum { MI_NO_SIGNAL = ' ', MI_SIGNAL = '*', MI_AFC_UP = '<', MI_AFC_DOWN = '>' }; /* enum status, boondock_airband.h:101 */

/* The DSP-relevant subset of a `devices` entry (src/config.cpp:731-808). */
typedef struct mi_device_cfg {
    int sample_rate;  /* Hz, input_t.sample_rate */
    int centerfreq;   /* Hz, input_t.centerfreq */
    int fft_size_log; /* global fft_size = 1<<log, 8..13 (boondock_airband.h:80-82) */
    int sfmt;         /* MI_SFMT_*, input_t.sfmt */
    float fullscale;  /* input_t.fullscale (s16/f32 only) */
    int tau;          /* device `tau` in us; <0: the global default 200 us (rtl_airband.cpp:87) */
    int fm_quadri;    /* 0: FM_FAST_ATAN2; 1: FM_QUADRI_DEMOD (the -Q flag) */
} mi_device_cfg;

/* The DSP-relevant subset of a `channels` entry (src/config.cpp:312-729), multichannel mode. */
typedef struct mi_channel_cfg {
    int freq;                   /* Hz */
    int modulation;             /* MI_MOD_* */
    int squelch_threshold_dbfs; /* `squelch_threshold`: 0 = unset/auto, <0 manual level in dBFS */
    int has_snr_threshold;      /* `squelch_snr_threshold` present */
    float squelch_snr_db;       /*   its value; -1 keeps the default 9.54 dB */
    float notch_freq;           /* `notch` Hz, 0 = none */
    float notch_q;              /* `notch_q`, 0 = default 10 */
    float ctcss_freq;           /* `ctcss` Hz, 0 = none */
    int bandwidth;              /* `bandwidth` Hz: 0 = key absent; > 0 derotation + low-pass at bandwidth/2; < 0 = key present with the
                                 * value 0 or a negative one: the reference sets needs_raw_iq and builds no filter (config.cpp:595-622) */
    float ampfactor;            /* `ampfactor`, default 1 */
    int tau;                    /* channel `tau` us, <0 inherit the device's */
    int afc;                    /* `afc` 0..255 (rtl_airband.cpp:180-251): >0 lets the picked bin follow the carrier; such a
                                 * handle processes its batches one at a time on the device and reports MI_AFC_UP / MI_AFC_DOWN */
    int has_iq_outputs;         /* the channel has a rawfile output (config.cpp:162) */
} mi_channel_cfg;

/* What the reference's stats file / TUI / JSON status read through Squelch getters on freq_t
 * (src/output.cpp:634-811, rtl_airband.cpp:654-665), mirrored back once per call. */
typedef struct mi_channel_stats {
    float noise_level;   /* Squelch::noise_level() */
    float signal_level;  /* Squelch::signal_level() */
    float squelch_level; /* Squelch::squelch_level(), evaluated without touching its cache */
    float agcavgfast;    /* freq_t.agcavgfast */
    uint64_t open_count, flappy_count, ctcss_count, no_ctcss_count;
    uint64_t active_counter; /* freq_t.active_counter (batches with axcindicate != NO_SIGNAL) */
    int32_t squelch_state;   /* Squelch::State of current_state_ */
    int32_t signal_outside_filter;
} mi_channel_stats;

typedef struct mi_demod mi_demod; /* nstreams independent device streams x nch channels, state resident in HBM */

const char* mi_last_error(void);
/* number of visible GPUs (0 if none / no runtime) -- never initialises more than the HIP runtime */
int mi_device_count(void);

/* Replaces init_demod() + the per-thread setup at the top of demodulate() (rtl_airband.cpp:253-266,
 * 338-373): builds window, level LUTs, twiddles, per-channel derived parameters exactly as the
 * reference derives them on the host, allocates device memory for up to max_batches WAVE_BATCHes per
 * call, and resets every channel to the reference's initial state (config.cpp:271-287,319-334).
 * All nstreams streams share the channel plan (the reference's "several dongles, same config" case). */
int mi_demod_create(const mi_device_cfg* dev, const mi_channel_cfg* chans, int nch, int nstreams, int max_batches, int gpu,
                    mi_demod** out);
void mi_demod_destroy(mi_demod* h);

/* Everything slow happens before the first batch: like init_demod() (rtl_airband.cpp:1058-1082) this runs before the input
 * threads start, because the reference's ring holds only 0.5 s of u8 IQ (config.cpp:799-805; overflow: input-helpers.cpp:56-61).
 *   mi_demod_create   also obtains the stage-1 kernel of the handle's own channel plan (fft_size 512): compiled with hipRTC
 *                     (0.3-0.6 s) or, from the second process start on, loaded from the code-object cache (milliseconds).
 *   mi_demod_prepare  additionally allocates the page-locked staging of `host_slots` (0 .. 3) host-buffer calls in flight
 *                     (mi_demod_process needs 1, mi_demod_submit / _wait up to 3); without it a slot is allocated by the first
 *                     call that uses it.  The first mi_demod_process of a prepared handle does no allocation and no compilation.
 *   mi_set_cache_dir  where code objects are kept (process-wide; call before mi_demod_create).  NULL or "" switches the cache
 *                     off.  Default: $MI_AIRBAND_CACHE_DIR, else $XDG_CACHE_HOME/mi_airband, else ~/.cache/mi_airband.  A file
 *                     is keyed by GPU architecture, runtime version, plan and kernel source, written atomically, checked on load.
 *   mi_jit_counts     kernels this process compiled / loaded from the cache (diagnostic). */
int mi_demod_prepare(mi_demod* h, int host_slots);
int mi_set_cache_dir(const char* dir);
int mi_jit_counts(int* compiled, int* from_cache);

/* Ring accounting for the caller (rtl_airband.cpp:416-417, 691).  A call producing nbatches batches
 * runs n_fft windows, hop_bytes apart, the last one fft_size samples long:
 *   needed   = (n_fft-1)*hop_bytes + 2*bytes_per_sample*fft_size   contiguous bytes from the stream position
 *   consumed = n_fft*hop_bytes                                     how far input_t.bufs advances
 * n_fft = nbatches*WAVE_BATCH (+AGC_EXTRA on a handle's first call, as waveend starts at 0). */
size_t mi_demod_bytes_needed(const mi_demod* h, int nbatches);
size_t mi_demod_bytes_consumed(const mi_demod* h, int nbatches);
size_t mi_demod_hop_bytes(const mi_demod* h);

/* Host-buffer entry: the batch body of demodulate() for all streams of the handle.
 *   iq[s]      -> first byte of stream s at its current position (mi_demod_bytes_needed() readable bytes)
 *   waveout    [nstreams][nch][nbatches*WAVE_BATCH + AGC_EXTRA]: exactly channel_t.waveout after the
 *              reference's loop -- [0, nbatches*WAVE_BATCH) is what the output thread emits
 *              (output.cpp:945-950), the last AGC_EXTRA samples are the not-yet-final lookahead
 *   iq_out     [nstreams][nch][nbatches*WAVE_BATCH][2] or NULL; rows of channels without iq outputs are untouched
 *   axc        [nstreams][nch][nbatches] MI_NO_SIGNAL / MI_SIGNAL (/ MI_AFC_UP / MI_AFC_DOWN on afc channels) per batch
 *              (channel_t.axcindicate)
 *   stats      [nstreams][nch] or NULL
 * Synchronous: on return the outputs are complete (publish waveavail after this returns). */
int mi_demod_process(mi_demod* h, const uint8_t* const* iq, int nbatches, float* waveout, float* iq_out, char* axc,
                     mi_channel_stats* stats);

/* The same call split in two, so that a host can keep up to three calls in flight: mi_demod_submit() starts the upload of the IQ, both
 * stages and the download of the results and returns; mi_demod_wait() completes the OLDEST submitted call -- on return that
 * call's waveout / iq_out / axc / stats hold its results.  The upload of call k+1 (its own copy stream and device buffer)
 * then runs under the compute of call k, and the download of call k under the compute of call k+1 (on plans that take the
 * time-parallel stage 2, consecutive calls also overlap on the device as with MI_OPT_EARLY_INPUT); results are identical
 * to the same calls made one after the other.  At most three calls are in flight: a fourth mi_demod_submit() first completes
 * the oldest one.  The IQ bytes must stay valid until the call has been waited for only if they live in pinned memory (see
 * mi_host_alloc); any other source is copied into the handle's staging before mi_demod_submit() returns.
 * mi_demod_process() == mi_demod_submit() + mi_demod_wait() (after completing whatever was in flight). */
int mi_demod_submit(mi_demod* h, const uint8_t* const* iq, int nbatches, float* waveout, float* iq_out, char* axc,
                    mi_channel_stats* stats);
int mi_demod_wait(mi_demod* h);

/* Page-locked host memory the copy engine reads directly: an input_t ring (input-common.h:39-57, allocated in
 * config.cpp:804) placed here is uploaded without the staging memcpy, which is what bounds the host-buffer entries on long
 * calls (a single thread copies ~12 GB/s, the link moves ~50).  Pointers from hipHostMalloc / hipHostRegister are recognised
 * as well, also for `waveout` (the audio is then downloaded straight into it).  mi_host_alloc returns NULL on failure. */
void* mi_host_alloc(size_t bytes);
void mi_host_free(void* p);

/* Device-resident entry (capture already in HBM; used for bulk replay and by bench.py).
 *   d_iq            device pointer, stream s starts at d_iq + s*stream_stride_bytes
 *   d_waveout       device [nstreams][nch][nbatches*WAVE_BATCH] -- the emitted samples only; the
 *                   AGC_EXTRA lookahead stays in the handle; 16-byte aligned (so is d_iq_out)
 *   d_iq_out        device [nstreams][nch][nbatches*WAVE_BATCH][2] or NULL
 *   d_axc           device [nstreams][nch][nbatches]
 *   hip_stream      hipStream_t to enqueue on (NULL = default stream); asynchronous */
int mi_demod_process_device(mi_demod* h, const void* d_iq, size_t stream_stride_bytes, int nbatches, float* d_waveout,
                            float* d_iq_out, char* d_axc, void* hip_stream);

/* Which streams of the handle take part in the calls made from now on (mi_demod_process, _submit, _process_device), until it is
 * changed: active[s] != 0 -- stream s takes part; NULL -- all streams (the default).  A live host lets a device whose ring is short,
 * or which has been retired, sit a turn out (the reference visits each device on its own and skips a short ring,
 * rtl_airband.cpp:381-422); a bulk replay puts captures of unequal length on one handle.
 * For a stream that is inactive in a call:
 *   - its IQ is not read: iq[s] may be NULL on the host entries, nothing is staged or uploaded for it, and the device entry
 *     touches nothing at d_iq + s*stream_stride_bytes;
 *   - its regions of waveout / d_waveout, iq_out, axc and stats are not written;
 *   - everything it carries between calls keeps its bytes (channel state, audio lookahead, the AGC_EXTRA carried samples, squelch
 *     ring, CTCSS detectors, AFC bin): when it is active again it continues as if the calls in between had never been made, bit for
 *     bit what the stream would have produced on a handle of its own.
 * mi_demod_bytes_needed / _consumed / _hop_bytes are per stream and do not change.  A call with a stream set aside takes the serial
 * stage 2 (mi_demod_last_path reports 0) and does not overlap its neighbours; calls of all streams keep every path they have.
 * Setting a mask first completes whatever mi_demod_submit has in flight.  MI_ERR_INVALID: no stream active; also returned by the
 * handle's first call (the one with AGC_EXTRA more windows) while a stream is set aside -- it needs every stream.
 * mi_demod_process_planes returns MI_ERR_UNSUPPORTED while a stream is set aside.
 * The first mask of a handle that sets a stream aside obtains the stage-1 kernel instance that takes a stream list (hipRTC, 0.3-0.6 s,
 * or the code-object cache): like mi_demod_prepare, do it once before the input threads start. */
int mi_demod_set_active_streams(mi_demod* h, const uint8_t* active /* [nstreams] or NULL */);
int mi_demod_get_active_streams(const mi_demod* h, uint8_t* active /* [nstreams] */);

/* stats of the last completed call (synchronises the handle's stream) */
int mi_demod_get_stats(mi_demod* h, mi_channel_stats* stats /* [nstreams][nch] */);

/* Checkpoint / resume of the complete per-channel DSP state (the reference has none). */
size_t mi_demod_state_size(const mi_demod* h);
int mi_demod_get_state(mi_demod* h, void* buf, size_t len);
int mi_demod_set_state(mi_demod* h, const void* buf, size_t len);

/* Which stage-2 path the last call took: the serial per-channel kernel (0) or the time-parallel one (1,
 * plain AM channels and long enough calls; DESIGN.md "Time-parallel stage 2").  unverified_rows counts
 * channels whose segment chain was not fully accepted after the serial fallback -- always 0; it exists so
 * the tests can assert that.  Synchronises. */
int mi_demod_last_path(mi_demod* h, int* time_parallel, int* unverified_rows);

/* Which stage-1 kernel the last call ran (diagnostic; every one of them yields the same bits): the radix-8 exchange kernels
 * (full graph, or pruned to the picked bins at N = 512), or the lane-resident kernel at N = 512, 1024 and 2048 (prebuilt full
 * graph, or compiled for this plan's own FFT nodes by hipRTC -- MI_OPT_LANE_FFT / MI_OPT_LANE_FFT_JIT). */
enum { MI_STAGE1_EXCHANGE_FULL = 0, MI_STAGE1_EXCHANGE_PRUNED = 1, MI_STAGE1_LANE_FULL = 2, MI_STAGE1_LANE_PLAN = 3 };
int mi_demod_last_stage1(mi_demod* h, int* kind);
/* (diagnostic) how often, since the handle was created, a channel's wave of the serial kernel gave up waiting for the wave that walks
 * its squelch pre-filter ahead (k_demod_pw; it then computes everything itself, same results): expected 0 */
int mi_demod_pre_wave_timeouts(mi_demod* h, unsigned* count);

/* TEST ENTRY -- stage 2 alone over caller-supplied planes: the per-channel loop of demodulate() (rtl_airband.cpp:517-669 with Squelch,
 * CTCSS, filters) run by the same kernels and along the same paths as mi_demod_process (serial / time-parallel by nbatches),
 * with stage 1 (convert x window -> FFT -> bin pick) replaced by a copy.  It exists so that the reference's own vectors for this
 * part of the path (tests/golden/components_ref.npz: outputs of the reference's squelch.cpp / filters.cpp compiled unmodified) can
 * be fed to the HIP code directly; a host never needs it.
 *   mag   [nstreams*nch][count] the values channel_t.wavein would receive from the FFT, count = nbatches*WAVE_BATCH (+ AGC_EXTRA on the
 *         handle's first call, as waveend starts at 0): entry AGC_EXTRA + i of the handle's running sequence is the squelch's raw
 *         sample of step i (rtl_airband.cpp:529), entry i the AM audio sample (:580)
 *   cplx  [nstreams*n_iq_rows][count][2] fftout of the channels with needs_raw_iq, in channel order (NULL if the plan has none)
 *   waveout / iq_out / axc / stats  exactly as mi_demod_process.  Synchronous.  Not for AFC plans (MI_ERR_UNSUPPORTED). */
int mi_demod_process_planes(mi_demod* h, const float* mag, const float* cplx, int nbatches, float* waveout, float* iq_out, char* axc,
                            mi_channel_stats* stats);

/* Diagnostics of the time-parallel path after a call that took it (synchronises): the exact Squelch core
 * state {noise_floor_, moving_avg_cap_, pre_filter_.capped_, pre_filter_.full_} before each segment (512 .. 4096 steps, by row count)
 * (core4: [nseg+1][4]) and diag8[0..3] = segments not accepted in verification scans 0..3 (scan 3 runs after the
 * serial fallback and is always 0; diag4[2] != 0 means the fallback had to run). */
int mi_demod_tp_debug(mi_demod* h, int row, float* core4, int max_entries, int* diag8, int* nseg);

/* Diagnostic view of stage 1's output as stage 2 left it after the last call (synchronises): the
 * magnitude plane of (stream, ch), plane index 0 = the oldest carried sample; after a call of n steps
 * indices [0, AGC_EXTRA) hold the carry for the next call.  iq may be NULL; it is only filled for
 * channels that need raw I/Q. Used by the stage-1 parity tests (channel_t.wavein / iq_in). */
int mi_demod_read_planes(mi_demod* h, int stream, int ch, int first, int count, float* mag, float* iq);

/* Timing of the kernels of the last mi_demod_process_device() call on its stream, from HIP events
 * recorded around each launch (ms; synchronises). */
int mi_demod_last_kernel_ms(mi_demod* h, float* channelize_ms, float* demod_ms);

/* Per-kernel timing of the last call, from HIP events recorded on the launch streams around the launches.
 * index 0 is the channelize kernel; then "k_demod" (serial path) or the kernels of the time-parallel path
 * ("k_tp_full", "k_tp_core", "k_tp_seg", "k_tp_scan#0", "k_tp_fix#0", "k_tp_rest" = the remaining small launches).
 * The time-parallel path runs a long call in chunks, so a kernel is launched *launches times; *ms_total is the
 * sum over those launches (kernels of different chunks and calls overlap on several streams, so the sums exceed the wall time).
 * Returns MI_ERR_INVALID past the last index: iterate from 0 until it fails.  *name is a static string. */
int mi_demod_kernel_time(mi_demod* h, int index, const char** name, float* ms_total, int* launches);
/* The same for an earlier call: age 1 = the call before the last one, age 2 .. 5 = the ones before that (while the event set has
 * not been reused: six sets cycle; serial calls reuse the set of the call before them).  Lets a caller that keeps calls in flight
 * read the timings of call k after it has enqueued calls k+1 .. k+4, without draining the pipeline (reading them earlier makes the
 * host wait for the end of call k's tail and the front of the following calls start late: DESIGN.md section 6). */
int mi_demod_kernel_time_prev(mi_demod* h, int age, int index, const char** name, float* ms_total, int* launches);
/* (diagnostic) Where a launch of a time-parallel call sat in time: milliseconds from the start of the core chain of the call
 * `ref_age` calls back to event `event` of chunk `chunk` of the call `age` calls back (events per chunk: 0 / 1 stage 1 begin / end,
 * 11 / 2 k_tp_full begin / end, 3 / 4 core chain begin / end, 5 / 12 segment pass begin / end, 10 / 7 scan begin / end, 8 fix end,
 * 9 finish end).  tools/call_timeline.py prints the table. */
int mi_demod_event_ms(mi_demod* h, int ref_age, int age, int chunk, int event, float* ms);

/* Options.  MI_OPT_EARLY_INPUT (default 0): the caller guarantees that the IQ bytes handed to
 * mi_demod_process_device() are valid when the call is made (not merely in the order of `hip_stream`), e.g. a capture
 * already resident in HBM or a ring filled by a copy engine the caller has synchronised with.  The library may then read
 * them before the work queued earlier on `hip_stream` has finished, which lets stage 1 and the serial core chain of a call
 * overlap the segment / fix passes of the previous call (time-parallel path), or stage 1 overlap the channel loop of the
 * previous call (serial path; a second set of planes is allocated on first use).  Outputs still complete in stream order.
 * The audio buffer of a call must then also be free when the call is made (no reader of an earlier result still pending on
 * another stream): when it is not the buffer of the previous call, the segment passes may write it early.
 * MI_OPT_STEADY_BLOCKS (default 1): the serial stage 2 takes runs
 * of steps during which the squelch stays CLOSED or OPEN 64 at a time; 0 = every step in the sample loop.  Results are
 * bit-identical either way (audio, flags, statistics, checkpoint state); the switch exists for measurements and tests. */
enum {
    MI_OPT_EARLY_INPUT = 1,
    MI_OPT_STEADY_BLOCKS = 2,
    /* Tuning switches, all result-neutral (every combination is bit-identical; they exist for measurements and tests).
     * A handle takes its defaults from the caller's environment when it is created (MI_AIRBAND_TP, _PRUNE, _L64, _L64_JIT, _CORE_SPLIT, _CONV=lut|arith,
     * _STEADY, _UNI_ROWS, _TP_CHUNKS, _TP_RATIO, _TP_LPW); the library itself keeps no process-wide state. */
    MI_OPT_TIME_PARALLEL = 3, /* -1 auto (plain AM plans of up to 256 rows, calls of >= 8 batches), 0 serial kernel, 1 whenever eligible */
    MI_OPT_PRUNE_FFT = 4,     /* 1 (default): at N = 512 evaluate only the FFT nodes the picked bins need */
    MI_OPT_U8_CONVERSION = 5, /* -1 auto, 0 level table in LDS, 1 arithmetic (checked against the table by the plan) */
    MI_OPT_UNI_ROWS = 6,      /* rows (stream x channel) up to which the serial kernel keeps one channel per wave (4096) */
    MI_OPT_TP_CHUNKS = 7,     /* chunks a time-parallel call is cut into, 0 = default */
    MI_OPT_TP_RATIO_PCT = 8,  /* growth of consecutive chunks in percent (150 = 1.5x), 0 = default */
    MI_OPT_TP_SEG_LANES = 9,  /* lanes per wave of the segment pass, 0 = auto */
    MI_OPT_LANE_FFT = 10,     /* 1 (default): at N = 512, 1024 and 2048 the first six FFT stages stay in the lanes (l64_kernel.h) where the plan allows */
    MI_OPT_CORE_SPLIT = 12,   /* 1 (default): the exact squelch core chain of the time-parallel path runs on three waves per channel -- one walks
                               * the noise-floor recurrence, one verifies, snapshots and steps, one fetches (tp.hip, k_tp_core2); 0: one wave */
    MI_OPT_SPEC_HEAD = 13,    /* 1 (default): when consecutive calls overlap (MI_OPT_EARLY_INPUT, alternating audio buffers) the first segments
                               * of a call warm up on the previous call's samples from a guessed state, as all others do, instead of waiting
                               * for the state that call's tail leaves; the scan checks them against it afterwards */
    MI_OPT_PRE_WAVE = 14,     /* serial stage 2 with one channel per wave: further waves of the channel's workgroup walk the squelch's pre-filter
                               * averages and noise floor over the call ahead of the channel's own wave (demod.hip, k_demod_pw: the full_ wave
                               * and the pre-filter wave).  -1 (default): up to 256 rows (streams x channels: one channel per CU) four waves per
                               * channel, up to 1 024 rows two (k_demod_pw2: the channel with its audio, and one wave for the pre-filter pair),
                               * beyond that none; 0 never, 1 four waves, 2 two waves */
    MI_OPT_RESERVE_CUS = 15,  /* time-parallel path: the wide passes of a call (stage 1, aggregates, segment pass) keep off this many CUs, which stay
                               * free for the core chains and the latency-bound tail kernels of the neighbouring calls (they need few waves but
                               * most of a SIMD's registers each, and otherwise wait for a wide wave to retire).  -1 (default): 32 on handles of
                               * up to 64 rows, 0 beyond; 0 never.  Takes effect only when the stream handed to mi_demod_process_device is not
                               * the NULL stream (the restricted streams are blocking ones: hipExtStreamCreateWithCUMask); set before the first
                               * time-parallel call.  The host-buffer entries use the handle's own stream and always qualify. */
    MI_OPT_AUDIO_WAVE = 16,   /* 1 (default): where MI_OPT_PRE_WAVE applies, an NFM channel gets a third wave that takes everything behind the
                               * filtered I/Q -- discriminator, DC block, de-emphasis, the CTCSS detector banks, output gate, notch filter,
                               * axcindicate and the audio / raw-I/Q stores -- from the channel's own wave (demod.hip, audio_wave) */
    MI_OPT_MIXED_PLAN = 17,   /* 1 (default): a plan that holds plain AM channels beside others (NFM, CTCSS, notch, low-pass, raw I/Q) sends the
                               * plain AM rows down the time-parallel path and the rest through the serial kernel, side by side in the same
                               * call (by itself in calls of >= 64 batches -- the time-parallel half has a fixed latency --, in any call under
                               * MI_OPT_TIME_PARALLEL = 1); 0: such a plan takes the serial kernel for every row */
    MI_OPT_SPLIT_CUS = 18,    /* Calls that take the serial kernel and overlap (MI_OPT_EARLY_INPUT): n > 0: k_demod runs alone on the last n CUs and
                               * stage 1 of the next call on the others (two CU-restricted streams, as under MI_OPT_RESERVE_CUS: only for calls whose
                               * stream is not the NULL stream); 0: the two share every CU; -1 (default): 128 for plans of 449 .. 512 rows -- two waves
                               * per row then fill 128 CUs two to a SIMD and stage 1 of as many streams is as long as the serial kernel: 64 streams x 8
                               * AM channels 344 -> 378 GS/s; with fewer rows the call is the serial kernel's latency either way.
                               * Set before the handle's first such call. */
    MI_OPT_LANE_FFT_JIT = 11  /* 1 (default): that kernel is compiled for the plan's own FFT nodes by hipRTC on first use (the code object is
                               * cached per (device, fft size, hop, masks) for the life of the process); 0, or hipRTC missing: the prebuilt full graph */
};
int mi_demod_set_option(mi_demod* h, int option, int value);

/* ---- host-only views of the derived plan (no GPU needed; used by the CPU test-suite) ---- */
typedef struct mi_plan mi_plan;
typedef struct mi_channel_derived {
    uint32_t bin;       /* dev->bins[i], config.cpp:669-670 */
    uint32_t dm_dphi;   /* channel_t.dm_dphi, config.cpp:682-713 */
    int32_t needs_raw_iq, has_iq_outputs, modulation;
    int32_t using_manual_level;
    float manual_signal_level, normal_signal_ratio, flappy_signal_ratio;
    float ampfactor, alpha;
    int32_t notch_enabled;
    float notch_d[3];
    int32_t lowpass_enabled;
    float lowpass_gain, lowpass_ycoeffs[2];
    int32_t ctcss_enabled, ctcss_fast_window, ctcss_slow_window, ctcss_fast_ndet, ctcss_slow_ndet;
} mi_channel_derived;

int mi_plan_create(const mi_device_cfg* dev, const mi_channel_cfg* chans, int nch, mi_plan** out);
void mi_plan_destroy(mi_plan* p);
int mi_plan_fft_size(const mi_plan* p);
int mi_plan_window(const mi_plan* p, float* out /* fft_size */);
int mi_plan_twiddles(const mi_plan* p, float* out /* fft_size/2 x {re,im} */);
int mi_plan_levels(const mi_plan* p, float* out /* 256, the LUT of the device's sample format */);
int mi_plan_sincos_lut(const mi_plan* p, float* sin_out /* 257 */, float* cos_out /* 257 */);
int mi_plan_channel(const mi_plan* p, int ch, mi_channel_derived* out);
/* The lane-resident stage 1 as the plan derives it (l64_kernel.h).  *enabled: the plan allows that kernel (fft_size 512, 1024 or
 * 2048, hop 160 or 128, no AFC, at most 64 channels, the kernel's twiddle literals equal to the plan's table); when it is 0 the
 * other outputs are zeroed.  need[s-1]: bit r is set when residue r = bin mod 2^s is live after in-lane stage s = 1..6.
 * *lanes_per_window = fft_size / 64.  slots[ch]: rank of the channel's class (bin mod 64) among the live classes.  stage_tw: for
 * each channel the twiddles of the combining stages s = 7 .. log2(fft_size) in that order, W_{2^s}^(bin mod 2^(s-1)) from the
 * plan's table, negated when the bin is an upper output of the stage (bit s-1 set).  Any output pointer may be NULL. */
int mi_plan_lane_fft(const mi_plan* p, int* enabled, uint64_t need[6], int* lanes_per_window, int* slots /* nch */,
                     float* stage_tw /* nch x (log2n-6) x {re,im} */);
int mi_plan_ctcss_coeffs(const mi_plan* p, int ch, int slow, float* out /* ndet */);

/* ---- synthetic IQ: integer-only, counter-based, identical on host and device ---- */
typedef struct mi_iqgen_carrier {
    int32_t offset_hz;   /* carrier offset from centre */
    int32_t kind;        /* 0 AM (1 kHz tone, 50 % depth); 1 NFM (1 kHz tone, 2.5 kHz dev); 2 NFM + 100 Hz CTCSS */
    int32_t amp_q8;      /* amplitude in 1/256 LSB (12 LSB = 3072) */
    int32_t gate_phase;  /* carrier is on while ((n / gate_samples) + gate_phase) is odd; gate_samples 0 = always on */
} mi_iqgen_carrier;

typedef struct mi_iqgen_cfg {
    int32_t sample_rate;
    uint64_t seed;
    int32_t noise_q8_mul;  /* noise scale: 111 gives sigma = 2.0 LSB */
    uint64_t gate_samples; /* on/off period in samples (sample_rate = 1 s) */
    int32_t ncarriers;
    mi_iqgen_carrier carriers[64];
} mi_iqgen_cfg;

/* u8 interleaved IQ for samples [first, first+count) of stream `stream_id` */
int mi_iqgen_host(const mi_iqgen_cfg* cfg, uint32_t stream_id, uint64_t first, uint64_t count, uint8_t* out);
int mi_iqgen_device(const mi_iqgen_cfg* cfg, uint32_t first_stream_id, uint32_t nstreams, size_t stream_stride_bytes, uint64_t first,
                    uint64_t count, void* d_out, void* hip_stream);

/* ---------------- mixer (src/mixer.cpp:56-98 connect, :114-140 put/mix, :157-261 thread) ----------------
 * One mixer_t: per WAVE_BATCH the output is zeroed, then every input that had a signal in that batch
 * (channel->axcindicate != NO_SIGNAL, output.cpp:564) is added as `sum[s] += in[s] * (ampfactor * ampl)` -- and
 * `* (ampfactor * ampr)` into the right channel when the mixer is stereo (some input has balance != 0,
 * mixer.cpp:82-83) -- in input order; an input whose multiplier is 0.0f is skipped (mixer.cpp:133-136); the mixer's
 * axcindicate is SIGNAL iff some input had one.  The reference mixes inputs in arrival order under jitter; this is the
 * jitter-free order (input index).  Inputs are rows of the audio the demod entry points write
 * ([row][row_stride] floats with row = stream * nch + channel, flags [row][axc_stride]), so on a multi-GPU job the
 * mixer runs on rank 0 over the gathered audio. */
typedef struct {
    int row;         /* stream * nch + channel of the audio buffer handed to mi_mixer_process_device */
    float ampfactor; /* mixer output's `ampfactor` (config.cpp:181), default 1 */
    float balance;   /* -1 .. 1 (config.cpp:182-186), default 0 */
} mi_mix_input;
typedef struct mi_mixer mi_mixer;

int mi_mixer_create(const mi_mix_input* inputs, int ninputs, int gpu, mi_mixer** out);
void mi_mixer_destroy(mi_mixer* m);
int mi_mixer_is_stereo(const mi_mixer* m);
/* d_waveout/d_axc: device buffers as written by mi_demod_process_device (nbatches batches); d_left / d_right:
 * [nbatches * WAVE_BATCH] (d_right may be NULL for a mono mixer, must not be for a stereo one); d_axc_out: [nbatches].
 * A row_stride below nbatches * WAVE_BATCH or an axc_stride below nbatches is refused with MI_ERR_INVALID, as every other
 * post-stage refuses it.  Enqueued on `hip_stream`, asynchronous. */
int mi_mixer_process_device(mi_mixer* m, const float* d_waveout, size_t row_stride, const char* d_axc, size_t axc_stride, int nbatches,
                            float* d_left, float* d_right, char* d_axc_out, void* hip_stream);

/* ---------------- output gate: the batches the outputs consume, compacted on the device ----------------
 * Every output of the reference except a `continuous` one drops a batch whose axcindicate is NO_SIGNAL; the gate applies that
 * rule on the device to the buffers mi_demod_process_device wrote and packs the (row, batch) blocks that travel, so that only
 * they cross the link.  One rule per row (row = stream * nch + channel):
 *   MI_GATE_NONE        nothing travels, and the row's carried flag is not touched (a row whose stream sits a call out under
 *                       mi_demod_set_active_streams keeps its state)
 *   MI_GATE_OPEN        axc[row][b] != MI_NO_SIGNAL: udp_stream and pulse, src/output.cpp:568-570, :581-582 (MI_AFC_UP / MI_AFC_DOWN
 *                       are signal)
 *   MI_GATE_OPEN_TRAIL  as MI_GATE_OPEN, or the batch before it was not MI_NO_SIGNAL: file and rawfile, src/output.cpp:518-520 with
 *                       output_t::active set at :560.  "Before" crosses call boundaries through a carried flag per row, which
 *                       starts false as output_t::active does
 *   MI_GATE_ALL         every batch: a `continuous` output (the same lines, continuous == true)
 * After a call the carried flag of every row whose rule is not MI_GATE_NONE is "the last batch of this call had a signal".
 * (The wall-clock file rotation of close_if_necessary stays with the host; its split_on_transmission rule in signal time is the
 * transmission splitter below.) */
enum { MI_GATE_NONE = 0, MI_GATE_OPEN = 1, MI_GATE_OPEN_TRAIL = 2, MI_GATE_ALL = 3 };
typedef struct { uint32_t row, batch; } mi_gate_block;
typedef struct mi_outgate mi_outgate;

/* row_rule [rows] MI_GATE_*; row_has_iq [rows] or NULL (no row has raw I/Q); 1 <= rows < 2^20, rows * max_batches < 2^24.
 * max_blocks: capacity of the caller's destination buffers in blocks, 0 = rows * max_batches. */
int mi_outgate_create(const uint8_t* row_rule, const uint8_t* row_has_iq, int rows, int max_batches, size_t max_blocks, int gpu,
                      mi_outgate** out);
void mi_outgate_destroy(mi_outgate* g);
/* Other rules from the next call on; the carried flags stay.  Completes the work queued on the device first. */
int mi_outgate_set_rules(mi_outgate* g, const uint8_t* row_rule /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches.  Inputs as mi_demod_process_device wrote them, strides as in
 * mi_mixer_process_device: d_waveout [rows][row_stride] floats, d_iq_out [rows][iq_row_stride] floats ({re, im} pairs,
 * 2 * WAVE_BATCH floats a batch) or NULL, d_axc [rows][axc_stride]; audio and I/Q 16-byte aligned with strides that are multiples
 * of 4 floats.  Outputs, all in device memory:
 *   d_blocks     [max_blocks][WAVE_BATCH]  the travelling audio blocks densely packed, rows ascending and batches ascending within
 *                a row: one row's blocks are one contiguous slice in time order (16-byte aligned)
 *   d_iq_blocks  [max_blocks][WAVE_BATCH][2]  for the same k the block of d_iq_out where row_has_iq[row] is set, untouched where it
 *                is not; may be NULL when d_iq_out is NULL or no row has raw I/Q (16-byte aligned)
 *   d_index      [max_blocks]  {row, batch} of block k (8-byte aligned)
 *   d_row_first  [rows + 1]  exclusive prefix of the rows' block counts
 *   d_count      [2]  number of travelling blocks, and min(that, max_blocks) = the number stored
 * A block whose position is at or beyond max_blocks is not stored and nothing is written there in any destination.
 * Asynchronous on `hip_stream`, no host synchronisation; three kernels without atomics, so the order is deterministic. */
int mi_outgate_process_device(mi_outgate* g, const float* d_waveout, size_t row_stride, const float* d_iq_out, size_t iq_row_stride,
                              const char* d_axc, size_t axc_stride, int nbatches, float* d_blocks, float* d_iq_blocks,
                              mi_gate_block* d_index, uint32_t* d_row_first, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_outgate_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the two
 * counts, then copies exactly count[1] blocks (and their raw I/Q blocks if iq_blocks is not NULL), their index entries and
 * row_first to the host.  The destinations hold max_blocks blocks / entries (row_first: rows + 1); pinned ones are written by the
 * copy engine directly.  blocks, iq_blocks, index and row_first may each be NULL (not wanted).  The one place that synchronises. */
int mi_outgate_download(mi_outgate* g, void* hip_stream, float* blocks, float* iq_blocks, mi_gate_block* index, uint32_t* row_first,
                        uint32_t* count /* [2] */);
/* Checkpoint / resume of the carried flags, `rows` bytes (0 / 1): the companion of mi_demod_get_state, so that a checkpointed
 * replay resumes with the same trailing batches.  Both complete the work queued on the device first. */
size_t mi_outgate_state_size(const mi_outgate* g);
int mi_outgate_get_state(mi_outgate* g, void* buf, size_t len);
int mi_outgate_set_state(mi_outgate* g, const void* buf, size_t len);
/* (diagnostic) on != 0: HIP events are recorded around each of the three launches of the calls made from now on;
 * mi_outgate_last_launch_ms waits for the last such call and gives ms[3] = {rank pass, scan, block copy}.  tools/gate_rate.py. */
int mi_outgate_set_timing(mi_outgate* g, int on);
int mi_outgate_last_launch_ms(mi_outgate* g, float* ms /* [3] */);
/* The same index on the host, for a caller that already has the flags: no GPU and no HIP call.  axc [rows][axc_stride];
 * carried_inout [rows] (0 / 1) is read and updated as the gate's own flags are; index holds up to rows * nbatches entries;
 * row_first [rows + 1]; count[0] = count[1] = the number of travelling blocks (there is no capacity here). */
int mi_gate_plan_host(const uint8_t* row_rule, int rows, const char* axc, size_t axc_stride, int nbatches, uint8_t* carried_inout,
                      mi_gate_block* index, uint32_t* row_first, uint32_t* count /* [2] */);

/* ---------------- transmission splitter: one recording per transmission, decided in signal time on the device ----------------
 * `split_on_transmission` (src/output.cpp:353-376) closes a transmission's file by gettimeofday(): duration > 1.0 s and idle > 0.5 s,
 * or duration > 3600 s.  A replay has no meaningful wall clock, so the rule is restated on the jitter-free schedule: batch b of a
 * row is handled at t0 + b * MI_WAVE_BATCH / MI_WAVE_RATE, and every time becomes a count of batches.  Per row the carried state is
 *   open (fdata->f != NULL), active (output_t::active), seq (the running file number, 0 before the first file), the batch at which
 *   the file was opened, the batch of the last write, and the row's own 64-bit batch clock.
 * For each batch, with signal = (axc != MI_NO_SIGNAL):
 *   check():  if open, d = clock - opened, i = clock - last write; the file closes when d > max or (d > min and i > idle)   :367-375
 *   !signal && !active:  check(); the batch does not travel                                                               :518-520
 *   otherwise:           check(); if not open: seq += 1, open, both stamps = clock (:404-414, :454); the batch travels into file
 *                        seq; active = signal (:560); last write = clock (:561)
 *   clock += 1
 * Thresholds in batches, from the reference's constants through MI_WAVE_BATCH / MI_WAVE_RATE in integers: d * 2000 > 1.0 * 16000
 * gives min = 8, i * 2000 > 0.5 * 16000 gives idle = 4, d * 2000 > 3600 * 16000 gives max = 28800.  The travelling set is exactly
 * MI_GATE_OPEN_TRAIL's, so an MI_GATE_OPEN_TRAIL gate run over the same call packs the blocks the records slice: file seq's audio
 * is blocks[row_first[row] + first_block ..][nblocks], its raw I/Q the same slice of d_iq_blocks.
 *
 * Order of `energy` (the device, mi_tx_plan_host and the tests' model all follow it).  Per block of 2000 floats = 500 float4, with
 * q = (double)x * (double)x (exact): thread t < 256 adds in sequence the four elements of float4 number t and, if t < 244, then
 * the four of float4 number 256 + t; the 256 partial sums are reduced by acc[t] += acc[t + d] for t < d, d = 128, 64, ..., 1; a
 * record's energy is the sequential double sum of its blocks' sums in block order.  peak = max |x| is order-free.  Inputs are the
 * demod's audio (finite, |x| <= 1, rtl_airband.cpp:625-632); NaN and Inf are unspecified.
 *
 * State blob: rows * 32 bytes, per row little-endian { uint64 clock; uint64 opened; uint64 last_write; uint32 seq; uint8 open;
 * uint8 active; uint16 zero } -- the stamps are values of the row's clock and keep their last value while no file is open. */
typedef struct { uint32_t min_batches, idle_batches, max_batches; } mi_tx_cfg; /* 0 = the reference's 8 / 4 / 28800 */
typedef struct {
    uint32_t row, seq;             /* seq: the row's file number since creation, 1-based */
    uint32_t first_block, nblocks; /* slice of the row's travelling blocks OF THIS CALL (rank under MI_GATE_OPEN_TRAIL); nblocks may be 0 */
    uint32_t first_batch;          /* call-relative batch of the first block; 0xFFFFFFFF when nblocks == 0 */
    uint32_t close_batch;          /* call-relative batch whose check closed the file; 0xFFFFFFFF = still open after the call */
    uint32_t flags;                /* bit 0: the file was open when the call began (these blocks are appended) */
    float peak;                    /* max |x| over the record's blocks of this call */
    double energy;                 /* sum of x * x over them, in the order above */
} mi_tx_record;                    /* 40 bytes */
typedef struct mi_txsplit mi_txsplit;
enum { MI_TX_STATE_ROW_BYTES = 32 };

/* row_enabled [rows] (0 = the row sits out: no record, and every byte of its state stays, clock included -- the companion of
 * mi_demod_set_active_streams, as MI_GATE_NONE is); 1 <= rows < 2^20, rows * (max_batches + 1) < 2^24.  One record per row and
 * file that a call touched (the file received a block or was closed), so a row has at most nbatches + 1 of them;
 * max_records: capacity of the caller's record buffer, 0 = rows * (max_batches + 1). */
int mi_txsplit_create(const mi_tx_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_records, int gpu,
                      mi_txsplit** out);
void mi_txsplit_destroy(mi_txsplit* t);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_txsplit_set_rows(mi_txsplit* t, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the buffers mi_demod_process_device wrote; alignment and strides as for
 * mi_outgate_process_device.  d_waveout may be NULL (a rawfile-only host): peak = 0 and energy = 0.  Outputs in device memory:
 *   d_records           [max_records]  rows ascending, seq ascending within a row (8-byte aligned)
 *   d_row_first_record  [rows + 1]     exclusive prefix of the rows' record counts
 *   d_count             [2]            number of records, and min(that, max_records) = the number stored
 * Nothing is written at or beyond max_records.  Asynchronous on `hip_stream`, no host synchronisation; four kernels (walk, scan,
 * block statistics, combine) without atomics, so every byte is the same on every run. */
int mi_txsplit_process_device(mi_txsplit* t, const float* d_waveout, size_t row_stride, const char* d_axc, size_t axc_stride, int nbatches,
                              mi_tx_record* d_records, uint32_t* d_row_first_record, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_txsplit_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] records.  records and row_first_record may each be NULL.  The one place that synchronises. */
int mi_txsplit_download(mi_txsplit* t, void* hip_stream, mi_tx_record* records, uint32_t* row_first_record, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_TX_STATE_ROW_BYTES bytes in the layout above (mi_tx_plan_host reads and writes the same bytes).
 * set_state refuses a blob whose open / active bytes are not 0 / 1 or whose padding is not zero.  Both complete queued work first. */
size_t mi_txsplit_state_size(const mi_txsplit* t);
int mi_txsplit_get_state(mi_txsplit* t, void* buf, size_t len);
int mi_txsplit_set_state(mi_txsplit* t, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[4] = {walk, scan, block statistics, combine}.  tools/tx_rate.py. */
int mi_txsplit_set_timing(mi_txsplit* t, int on);
int mi_txsplit_last_launch_ms(mi_txsplit* t, float* ms /* [4] */);
/* The host twin: no GPU and no HIP call; the same state blob byte for byte and the same records, peak and energy included.
 * axc [rows][axc_stride]; waveout [rows][row_stride] or NULL; state_inout rows * MI_TX_STATE_ROW_BYTES bytes, read and updated;
 * records holds max_records entries (max_records >= 1), of which min(count[0], max_records) = count[1] are written. */
int mi_tx_plan_host(const mi_tx_cfg* cfg, const uint8_t* row_enabled, int rows, const char* axc, size_t axc_stride, int nbatches,
                    const float* waveout, size_t row_stride, void* state_inout, mi_tx_record* records, size_t max_records,
                    uint32_t* row_first_record, uint32_t* count /* [2] */);

/* ---------------- band survey: per-bin mean and peak magnitude per cell, the pass that comes before a channel plan ----------------
 * The demodulator evaluates only the bins its plan picks; the survey looks at every bin of the full fft_size-point FFT, for a caller
 * who holds a wide-band capture and no channel list yet.  It reads the device-resident IQ mi_demod_process_device reads and runs the
 * same windows -- the plan's Blackman-7 window, the device's sample conversion (fullscale as in stage 1), hop_bytes apart, fft_size
 * long -- and reduces every run of windows_per_cell consecutive windows (a cell) to two floats per bin:
 *   peak[stream][cell][bin] = the maximum over the cell's windows of sqrtf(re * re + im * im)
 *   mean[stream][cell][bin] = (float)(S / windows_per_cell), S = the sum of the same float magnitudes accumulated in float64
 * A window's spectrum is the documented FFT, so a magnitude has the bits stage 1 would give the bin.
 * Window placement: cell c of stream s covers windows c * wpc .. (c + 1) * wpc - 1, counted from d_iq + s * stream_stride_bytes.  The
 *   stage keeps no state between calls.  A caller who wants the cells aligned with the demodulator's audio batches offsets the
 *   pointer: the first call of a demod handle runs MI_AGC_EXTRA more windows (mi_demod_bytes_needed), so batch b of that handle's
 *   audio is made of the windows MI_AGC_EXTRA + b * MI_WAVE_BATCH .. of the capture -- hand the survey d_iq + MI_AGC_EXTRA * hop_bytes.
 * Bin order: FFT order 0 .. fft_size - 1, the index mi_plan_channel().bin reports (bin 0 = centerfreq, the upper half = below it).
 * Supported: fft_size_log 8 .. 13, all four sample formats, any hop the plan derives (160, 128, 150, ...); d_iq and the stream stride
 *   aligned to one complex sample.  Stateless, no option or environment switch; nothing is shared with a demod handle.
 * The hop is bounded by the LDS: a workgroup keeps a piece of 64 windows (32 at fft 2048, 16 at 4096, 8 at 8192) of IQ there beside
 *   its exchange slots, and may ask for 160 KiB (163 840 bytes) at most.  mi_survey_create refuses a configuration that needs more, with
 *   MI_ERR_INVALID and both figures in mi_last_error(), before it looks for a device.  The need grows with hop_bytes: at fft 256
 *   the largest hop is 568 samples with s16 (9.088 MS/s; a 10 MS/s capture is refused), 1141 with u8 / s8, 282 with f32 (4.512 MS/s);
 *   fft 1024 allows the least (1129 / 556 / 270), the sizes above it more, their pieces being shorter.
 * Disabled streams (mi_survey_set_streams; the companion of mi_demod_set_active_streams, as MI_GATE_NONE is): a disabled stream's IQ
 *   is not read and its regions of d_mean / d_peak are not written.  NULL enables all (the default).  Completes queued work first.
 * Execution: asynchronous on `hip_stream`, no host synchronisation; two kernels (the windows; the fold of a cell's partial sums).  The
 *   partial sums live in the handle: calls of one handle go to one stream, or are ordered by the caller.
 * Determinism: no floating-point atomics; the partial sums of a cell are combined in a fixed order (csrc/survey.hip), so two runs give
 *   the same bytes.  With f32 input, NaN and Inf are unspecified.
 * MI_ERR_NO_DEVICE without a GPU; MI_ERR_INVALID for bad arguments, a hop over the LDS bound, d_mean / d_peak not 16-byte aligned,
 * ncells outside 1 .. max_cells, or a mask that enables no stream (the mask then stays as it was). */
typedef struct mi_survey mi_survey;
/* 1 <= nstreams < 2^16, 1 <= max_cells < 2^24; windows_per_cell 0 = MI_WAVE_BATCH (one audio batch), at most 2^20 */
int mi_survey_create(const mi_device_cfg* dev, int nstreams, int max_cells, int windows_per_cell, int gpu, mi_survey** out);
void mi_survey_destroy(mi_survey* s);
int mi_survey_set_streams(mi_survey* s, const uint8_t* stream_enabled /* [nstreams] or NULL = all */);
/* contiguous bytes a call over ncells cells reads per stream: (ncells * wpc - 1) * hop_bytes + 2 * bytes_per_sample * fft_size */
size_t mi_survey_bytes_needed(const mi_survey* s, int ncells);
/* d_mean, d_peak: device [nstreams][ncells][fft_size] each, 16-byte aligned */
int mi_survey_process_device(mi_survey* s, const void* d_iq, size_t stream_stride_bytes, int ncells, float* d_mean, float* d_peak,
                             void* hip_stream);
/* (diagnostic) as mi_outgate_set_timing; ms[2] = {windows, fold}.  tools/survey_rate.py. */
int mi_survey_set_timing(mi_survey* s, int on);
int mi_survey_last_launch_ms(mi_survey* s, float* ms /* [2] */);
/* From a bin back to frequencies a plan can be given: no GPU and no HIP call.  The plan's bin rule (config.cpp:669-670) is
 * bin = ceil((freq + sample_rate - centerfreq) / (sample_rate / fft_size) - 1.0) % fft_size with the INTEGER quotient
 * q = sample_rate / fft_size: the unwrapped index B owns the q frequencies B q + 1 .. (B + 1) q above centerfreq - sample_rate, upper
 * end included, lower end not.  A frequency exactly on an FFT bin's centre therefore lands in the bin BELOW it, which is why this
 * returns a range and not "the bin's frequency".  [*lo_hz, *hi_hz] is a closed range of integer frequencies inside the band
 * [centerfreq - sample_rate / 2, centerfreq + sample_rate / 2) that all map to `bin`, and *lo_hz - 1 and *hi_hz + 1 do not (where they
 * lie in the band).  The band is half open at the other end than the rule, and wider than fft_size * q where the quotient truncates,
 * so it holds fft_size + 1 values of B or a few more: a bin next to fft_size / 2 can own a second, shorter piece at the opposite
 * edge of the band (at 2.56 MS/s and fft 256 the one frequency centerfreq - 1280000 maps to bin 127, whose range lies at the top of
 * the band).  The range returned is the bin's longest piece, the lower one of two equal ones; the ranges of all bins are disjoint,
 * and what they leave uncovered is those second pieces at the band's edges, fewer than 2 q + fft_size frequencies in all.
 * MI_ERR_INVALID: bin outside 0 .. fft_size - 1, or a device configuration the plan refuses. */
int mi_survey_bin_range(const mi_device_cfg* dev, int bin, int* lo_hz, int* hi_hz);

/* ---------------- channel finder: occupancy and channel candidates from the survey's planes ----------------
 * The link between the band survey and a channel plan: which bins carry something, and when.  It reads the two planes
 * mi_survey_process_device wrote -- d_mean, d_peak [nstreams][ncells][fft_size] float32, FFT bin order -- and keeps no state between
 * calls: one call looks at the ncells cells it is given.  Values are non-negative and finite, as the survey emits them; a set sign
 * bit, NaN and Inf are unspecified.  With N = fft_size, per (stream, bin):
 *   floor      the element at index k = (ncells - 1) * floor_permille / 1000 (integer division) of the bin's `mean` over the call's
 *              cells sorted ascending: an exact order statistic, not an estimate
 *   threshold  floor * ratio, one float32 multiply
 *   cell c is active iff mean[c][bin] > threshold
 *   mi_occ_bin: the floor, the threshold, the number of active cells, the first and the last of them (0xFFFFFFFF when none), the
 *              number of maximal runs of consecutive active cells ("transmissions" at cell resolution), and the maxima of mean and of
 *              peak over the active cells (0.0f when none)
 * Per stream, the candidates.  Bins are walked in frequency order: position p = (bin + N / 2) % N, so position 0 is bin N / 2, the
 * bottom of the band, bins N - 1 and 0 are neighbours in the middle, and the band does not wrap.  A bin is occupied iff
 * active_cells >= min_cells; a candidate is a maximal run of occupied positions (the Blackman-7 main lobe spreads one strong
 * carrier over up to about 13 bins, which is why the clustering is done here).  mi_occ_candidate: the stream, best_bin = the run's
 * bin with the largest max_mean (ties: the lowest position), lo_bin / hi_bin = the FFT-order bins at the run's lowest and highest
 * position, nbins, and best_bin's active_cells, first_cell, last_cell, max_mean and max_peak.  Candidates are stored streams
 * ascending, positions ascending within a stream.  mi_survey_bin_range(best_bin) gives frequencies mi_plan_create maps to that bin.
 * Configuration (mi_occ_cfg, a field that is 0 takes its default): floor_permille 250 (at most 1000); ratio 3.0f, the amplitude ratio
 * of the reference's default squelch SNR of 9.54 dB (squelch.cpp constructor defaults) -- a caller's setting, not a tolerance, and
 * not validated on a real band; min_cells 1 (at most max_cells).
 * Disabled streams (mi_occupancy_set_streams, the companion of mi_survey_set_streams): a disabled stream's planes are not read, its
 *   mi_occ_bin region is not written and it has no candidates (its d_stream_first entries repeat).  NULL enables all (the default).
 *   A mask that enables no stream is refused and the mask stays as it was.  Completes queued work first.
 * Execution: asynchronous on `hip_stream`, no host synchronisation; four kernels (bin records; run starts; scan; candidates).  The
 *   run starts of a call live in the handle: calls of one handle go to one stream, or are ordered by the caller.
 * Determinism: no floating-point atomics (integer counts in LDS only, which are order-free): every output byte is the same on every
 *   run, and equals mi_occupancy_plan_host's.
 * Only fft_size_log of the device configuration enters the arithmetic; the rest is checked as the plan checks it.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, floor_permille > 1000, a ratio that is negative or
 * not finite, min_cells > max_cells, misaligned buffers, ncells outside 1 .. max_cells, or a device configuration the plan refuses. */
typedef struct { uint32_t floor_permille; float ratio; uint32_t min_cells; } mi_occ_cfg; /* 0 = 250 / 3.0f / 1 */
typedef struct {
    float floor, threshold;
    uint32_t active_cells;
    uint32_t first_cell, last_cell; /* 0xFFFFFFFF when no cell is active */
    uint32_t runs;                  /* maximal runs of consecutive active cells */
    float max_mean, max_peak;       /* over the active cells; 0.0f when none */
} mi_occ_bin;                       /* 32 bytes */
typedef struct {
    uint32_t stream;
    uint32_t best_bin;                            /* largest max_mean of the run; ties: the lowest position */
    uint32_t lo_bin, hi_bin;                      /* FFT-order bins at the run's lowest and highest position */
    uint32_t nbins;
    uint32_t active_cells, first_cell, last_cell; /* best_bin's */
    float max_mean, max_peak;                     /* best_bin's */
} mi_occ_candidate;                               /* 40 bytes */
typedef struct mi_occupancy mi_occupancy;
/* cfg NULL = all defaults; 1 <= nstreams < 2^16, 1 <= max_cells < 2^24; max_candidates: capacity of the caller's candidate buffer,
 * 0 = nstreams * fft_size / 2, the most that alternating bins can give */
int mi_occupancy_create(const mi_device_cfg* dev, const mi_occ_cfg* cfg, int nstreams, int max_cells, size_t max_candidates, int gpu,
                        mi_occupancy** out);
void mi_occupancy_destroy(mi_occupancy* o);
int mi_occupancy_set_streams(mi_occupancy* o, const uint8_t* stream_enabled /* [nstreams] or NULL = all */);
/* One call over ncells (1 .. max_cells) cells.  d_mean, d_peak: device [nstreams][ncells][fft_size], 16-byte aligned.  Outputs, all
 * in device memory:
 *   d_bins          [nstreams][fft_size]  in FFT bin order (16-byte aligned)
 *   d_cands         [max_candidates]      (8-byte aligned)
 *   d_stream_first  [nstreams + 1]        exclusive prefix of the streams' candidate counts
 *   d_count         [2]                   candidates found, and min(that, max_candidates) = the number stored
 * Nothing is written at or beyond max_candidates. */
int mi_occupancy_process_device(mi_occupancy* o, const float* d_mean, const float* d_peak, int ncells, mi_occ_bin* d_bins,
                                mi_occ_candidate* d_cands, uint32_t* d_stream_first, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_occupancy_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] candidates; bins holds nstreams * fft_size records (a disabled stream's are copied as they lie in d_bins),
 * stream_first nstreams + 1.  bins, cands and stream_first may each be NULL.  The one place that synchronises. */
int mi_occupancy_download(mi_occupancy* o, void* hip_stream, mi_occ_bin* bins, mi_occ_candidate* cands, uint32_t* stream_first,
                          uint32_t* count /* [2] */);
/* (diagnostic) as mi_outgate_set_timing; ms[4] = {bin records, run starts, scan, candidates}.  tools/occupancy_rate.py. */
int mi_occupancy_set_timing(mi_occupancy* o, int on);
int mi_occupancy_last_launch_ms(mi_occupancy* o, float* ms /* [4] */);
/* The host twin: no GPU and no HIP call; the same bytes in every output, and nothing written in a disabled stream's region of bins.
 * stream_enabled [nstreams] or NULL = all; mean, peak [nstreams][ncells][fft_size]; bins [nstreams][fft_size]; cands holds
 * max_candidates entries (0 = nstreams * fft_size / 2), of which count[1] are written.  There is no max_cells here, so min_cells is
 * not bounded: a min_cells above ncells leaves no bin occupied, as it does on the device. */
int mi_occupancy_plan_host(const mi_device_cfg* dev, const mi_occ_cfg* cfg, const uint8_t* stream_enabled, int nstreams, const float* mean,
                           const float* peak, int ncells, mi_occ_bin* bins, mi_occ_candidate* cands, size_t max_candidates,
                           uint32_t* stream_first, uint32_t* count /* [2] */);

/* ---------------- channel probe: per-candidate envelope and phase statistics, the step between the finder and a channel plan ----------------
 * The finder says which bins carry something and when; a mi_channel_cfg also needs a modulation and, for NFM, a carrier frequency
 * inside the bin.  The survey's planes keep magnitudes only; the probe keeps, for a caller-given list of targets {stream, bin}, the
 * complex value of that bin in every window and reduces it per cell.  It reads the device-resident IQ the survey reads and runs the
 * same windows (the plan's window, the device's conversion, hop_bytes apart, fft_size long, windows_per_cell to a cell; cell c of a
 * stream covers windows c * wpc .. (c + 1) * wpc - 1 counted from d_iq + s * stream_stride_bytes).
 * Arithmetic.  For target k and window w, re and im are the float32 parts of bin bin_k of the documented FFT: the bits
 * the survey and stage 1 give.  m_w = sqrtf(re * re + im * im) in float32, each operation rounded.  Per (target, cell), over the
 * cell's windows, in float64:
 *   s1   = sum of (double)m_w
 *   s2   = sum of (double)m_w * (double)m_w                                  (each product is exact)
 *   r_re = sum of (double)re_w * (double)re_p + (double)im_w * (double)im_p  (p = w - 1; exact products, their sum rounded once)
 *   r_im = sum of (double)im_w * (double)re_p - (double)re_w * (double)im_p  (the same)
 *   so r_re + j r_im = sum of z_w * conj(z_p): its angle is the mean phase advance of the bin per hop.
 * A pair (w, p) belongs to the cell of w.  The first window of the call has no predecessor and contributes no pair: cell 0 has
 * wpc - 1 pairs, every other cell wpc.  `windows` = wpc and `pairs` say over how many terms the sums run.  The stage keeps no state
 * between calls.  Order of the sums: fixed, documented in csrc/probe.hip; no floating-point atomics, so two runs give the same bytes.
 * It is not window order: a float64 model that adds in window order differs by the reordering of at most wpc terms.
 * Targets (mi_probe_set_targets): 1 .. max_targets of them, strictly ascending by (stream, bin) -- a duplicate is refused as an
 *   unsorted list is --, stream < nstreams, bin < fft_size.  The list is copied to the device; queued work completes first; after a
 *   refusal the old list stays.  Targets of one stream share one pass over that stream's IQ; a stream with no target is not read.
 *   mi_probe_targets_from_candidates (host only) makes the list from the finder's candidates: best_bin of each, sorted.
 * Output: d_cells [ntargets][ncells] of mi_probe_cell, 8-byte aligned, in the order of the target list.
 * Execution: asynchronous on `hip_stream`, no host synchronisation; two kernels (the windows; the reduction of each (target, cell)).
 *   Between them the bins' values lie in a scratch plane in the handle, 8 bytes per (target, window): calls of one handle go to one
 *   stream, or are ordered by the caller.  mi_probe_download is the one place that synchronises.
 * Supported: what the survey supports, its bound on the hop included: the windows kernel keeps the same piece of IQ in LDS, and
 *   mi_probe_create refuses a configuration whose workgroup would need more than 160 KiB in the survey's way (at fft 256: hop 568
 *   samples with s16, 1141 with u8 / s8, 282 with f32).  With f32 input, NaN and Inf are unspecified.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, a refused target list, a call before any list was
 * set, d_cells not 8-byte aligned, ncells outside 1 .. max_cells, or a device configuration the plan refuses. */
typedef struct { uint32_t stream, bin; } mi_probe_target; /* 8 bytes */
typedef struct {
    double s1, s2, r_re, r_im;
    uint32_t windows, pairs;
} mi_probe_cell; /* 40 bytes */
typedef struct mi_probe mi_probe;
/* 1 <= nstreams < 2^16, 1 <= max_cells < 2^24, windows_per_cell 0 = MI_WAVE_BATCH, at most 2^20 (the survey's limits);
 * 1 <= max_targets <= nstreams * fft_size, max_targets * max_cells < 2^31.  Allocates the scratch plane:
 * 8 * max_targets * max_cells * windows_per_cell bytes. */
int mi_probe_create(const mi_device_cfg* dev, int nstreams, int max_cells, int windows_per_cell, int max_targets, int gpu, mi_probe** out);
void mi_probe_destroy(mi_probe* p);
int mi_probe_set_targets(mi_probe* p, const mi_probe_target* targets, int ntargets);
/* contiguous bytes a call over ncells cells reads per stream: mi_survey_bytes_needed's formula */
size_t mi_probe_bytes_needed(const mi_probe* p, int ncells);
int mi_probe_process_device(mi_probe* p, const void* d_iq, size_t stream_stride_bytes, int ncells, mi_probe_cell* d_cells, void* hip_stream);
/* The records of the last mi_probe_process_device, which must have been enqueued on `hip_stream`: waits for it and copies
 * ntargets * ncells records of that call. */
int mi_probe_download(mi_probe* p, void* hip_stream, mi_probe_cell* cells);
/* (diagnostic) as mi_outgate_set_timing; ms[2] = {windows, reduce}.  tools/probe_rate.py. */
int mi_probe_set_timing(mi_probe* p, int on);
int mi_probe_last_launch_ms(mi_probe* p, float* ms /* [2] */);
/* Host only, no HIP call: out[i] = {cands[i].stream, cands[i].best_bin}, then sorted by (stream, bin).  The finder stores its
 * candidates by stream and by position (bin N / 2 first), so the order changes within a stream. */
int mi_probe_targets_from_candidates(const mi_occ_candidate* cands, size_t n, mi_probe_target* out /* [n] */);

/* From the cells of one target to what a channel plan asks for: no GPU and no HIP call.
 * mi_probe_features_host adds the sums of the selected cells (cell_mask[c] != 0; NULL = all) in cell order -- S1, S2, R_re, R_im, the
 * window count n and the pair count -- and derives, in float64:
 *   cv2        = n * S2 / (S1 * S1) - 1    the squared coefficient of variation of the envelope: about 0 for a constant envelope
 *   coherence  = hypot(R_re, R_im) / S2    how steadily the phase advances from window to window; at most about 1
 *   dphi       = atan2(R_im, R_re)         the mean phase advance per hop, in (-pi, pi]
 *   carrier_hz : with hop = the plan's hop in samples (sample_rate / MI_WAVE_RATE rounded to the nearest integer) and the window rate
 *                fw = (double)sample_rate / hop (MI_WAVE_RATE exactly where sample_rate == hop * MI_WAVE_RATE, else not: 2.4 MS/s has
 *                hop 150 and fw = 16000, 2.5 MS/s has hop 156 and fw = 16025.64...), a carrier at centerfreq + f advances the bin's
 *                phase by 2 pi f / fw per hop, so f is known modulo fw: f0 = dphi / (2 pi) * fw.  With [lo, hi] =
 *                mi_survey_bin_range(dev, bin) and mid = (lo + hi) / 2.0,
 *                  carrier_hz = centerfreq + f0 + fw * nearbyint((mid - centerfreq - f0) / fw)
 *                the frequency congruent to f0 nearest to the middle of the bin's range.  Unambiguous while a bin is narrower than fw
 *                (fft_size > hop).  It is an estimate of the power-weighted mean frequency in the bin, not a bound.
 * A caller masks cells with the finder's threshold: cell c is selected iff mean[c][bin] > mi_occ_bin.threshold.  If no cell is
 * selected, or S1 == 0, every field is 0.  MI_ERR_INVALID: NULL arguments, ncells < 1, bin out of range, a configuration the plan refuses.
 * mi_probe_classify_host: *modulation = MI_MOD_NFM iff coherence < rule.coherence_max or cv2 < rule.cv2_min, else MI_MOD_AM; with
 * n == 0 it is refused (nothing to classify).  rule NULL or a field that is 0 takes its default, coherence_max 0.9314 and cv2_min
 * 0.1005: the geometric middles between the two classes' nearest values over synthetic captures (DESIGN.md 5g has the table).  They
 * are a caller's settings like the finder's ratio, measured on mi_iqgen signals only: they have NOT been tried on a real band. */
typedef struct {
    double s1, s2, r_re, r_im;  /* totals over the selected cells */
    uint64_t n, pairs;          /* windows and pairs in them */
    double cv2, coherence, dphi, carrier_hz;
} mi_probe_features;            /* 80 bytes */
typedef struct { double coherence_max, cv2_min; } mi_probe_rule; /* 0 = the default */
int mi_probe_features_host(const mi_device_cfg* dev, int bin, const mi_probe_cell* cells, int ncells, const uint8_t* cell_mask /* [ncells] or NULL = all */,
                           mi_probe_features* out);
int mi_probe_classify_host(const mi_probe_features* f, const mi_probe_rule* rule /* NULL = defaults */, int* modulation);

/* ---------------- CTCSS tone finder: all 51 standard tones per window, on the device ----------------
 * The demodulator answers "is THIS tone present?" (Squelch::set_ctcss_freq, src/ctcss.cpp:105-163): one Goertzel detector for the
 * target, one for every standard tone at least 5 Hz away, and the target must be the strongest.  The finder answers "which tone?":
 * the whole bank of the reference's 51 CTCSS::standard_tones (ctcss.cpp:101-103) over the audio mi_demod_process_device wrote, one
 * record per row and window of window_samples samples.  A post-stage like the gate and the splitter: rows of d_waveout plus d_axc,
 * state carried in the handle, a host twin, every byte the same on every run, no host synchronisation.
 *
 * Tone table: the 51 tones in the reference's table order, index 0 = 67.0 Hz .. 50 = 254.1 Hz.  Coefficient of tone t at window W:
 * ToneDetector's (ctcss.cpp:31-42) at sample rate MI_WAVE_RATE: k = (int)(0.5 + W * freq / 16000), omega = (float)(2 pi k / W),
 * coeff = (float)(2 cos(omega)) -- the value mi_plan_ctcss_coeffs gives for a channel with that ctcss_freq.  Below W = 6400 tones
 * share a k and so a coefficient: mi_tones_table reports the aliases (11 distinct coefficients at 800, 25 at 2000, 37 at 3200, 51
 * at 6400 and above).  Aliased tones have equal powers; the lowest index of the group is the one `best` and `second` name.
 *
 * Per row the state is { uint32 count; uint32 seq; float q1[64]; float q2[64] }, lane t < 51 = tone t, lanes 51 .. 63 zero.  For
 * each batch b of an enabled row, in order:
 *   axc[row][b] == MI_NO_SIGNAL:  count = 0 and q1 = q2 = 0 -- CTCSS::reset on the way to CLOSED (squelch.cpp:287, ctcss.cpp:165-172),
 *                                 restated at batch resolution
 *   otherwise:  each of the batch's 2000 samples x in order:  for every tone  q0 = coeff * q1 - q2 + x; q2 = q1; q1 = q0;  count++;
 *               when count == window:  p[t] = q1 * q1 + q2 * q2 - q1 * q2 * coeff for every tone, one record is emitted, then
 *               q1 = q2 = 0, count = 0, seq++
 * Every operation is float32 and rounds on its own (no fused multiply-add).  In a record, mean_power is the sequential float32 sum
 * p[0] + p[1] + .. + p[50] in index order divided by 51.0f; best is the index of the largest p, the lowest index on ties; second the
 * same over the other 50.  Records are stored rows ascending, seq ascending within a row.  A disabled row produces no record and
 * every byte of its state stays.  Inputs are the demodulator's audio (finite, |x| <= 1); NaN and Inf are unspecified.
 *
 * State blob: rows * MI_TONES_STATE_ROW_BYTES bytes, per row little-endian in the layout above. */
enum { MI_TONES_STANDARD = 51, MI_TONES_LANES = 64, MI_TONES_STATE_ROW_BYTES = 520 };
typedef struct { uint32_t window_samples; } mi_tones_cfg; /* 0 = 6400 = (int)(MI_WAVE_RATE * 0.4), squelch.cpp:115; 800 .. 64000 */
typedef struct {
    uint32_t row, seq;              /* seq: the row's window number since creation / set_state, 0-based; a reset does not reset it */
    uint32_t end_batch, end_sample; /* call-relative batch and offset (0 .. 1999) of the window's last sample */
    uint32_t best, second;          /* indices into the tone table; ties: the lowest index */
    float best_power, second_power, mean_power;
    uint32_t zero;
} mi_tone_record;                   /* 40 bytes */
typedef struct mi_tones mi_tones;

/* cfg NULL = the default window.  row_enabled [rows] as for mi_txsplit_create; 1 <= rows < 2^20, 1 <= max_batches <= 2^20 and
 * rows * ((window - 1 + 2000 * max_batches) / window) < 2^24: the second factor is the most windows one row can complete in a call.
 * max_records: capacity of the caller's record (and powers) buffer, 0 = that product. */
int mi_tones_create(const mi_tones_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_records, int gpu, mi_tones** out);
void mi_tones_destroy(mi_tones* t);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_tones_set_rows(mi_tones* t, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the buffers mi_demod_process_device wrote; alignment and strides as for
 * mi_outgate_process_device (d_waveout is required).  Outputs in device memory:
 *   d_records           [max_records]      rows ascending, seq ascending within a row (8-byte aligned)
 *   d_powers            [max_records][64]  or NULL (not wanted): p[0 .. 50] of record k, entries 51 .. 63 zero (4-byte aligned)
 *   d_row_first_record  [rows + 1]         exclusive prefix of the rows' record counts
 *   d_count             [2]                number of records, and min(that, max_records) = the number stored
 * Nothing is written at or beyond max_records.  Asynchronous on `hip_stream`, no host synchronisation; three kernels (walk, scan,
 * bank) without atomics, so every byte is the same on every run. */
int mi_tones_process_device(mi_tones* t, const float* d_waveout, size_t row_stride, const char* d_axc, size_t axc_stride, int nbatches,
                            mi_tone_record* d_records, float* d_powers, uint32_t* d_row_first_record, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_tones_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] records (and their powers, if the call had a d_powers and powers is not NULL; with powers not NULL after
 * a call without d_powers it is refused).  records, powers and row_first_record may each be NULL.  The one place that synchronises. */
int mi_tones_download(mi_tones* t, void* hip_stream, mi_tone_record* records, float* powers, uint32_t* row_first_record, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_TONES_STATE_ROW_BYTES bytes in the layout above (mi_tones_plan_host reads and writes the same
 * bytes).  set_state refuses a blob with count >= window or a padding lane that is not zero.  Both complete queued work first. */
size_t mi_tones_state_size(const mi_tones* t);
int mi_tones_get_state(mi_tones* t, void* buf, size_t len);
int mi_tones_set_state(mi_tones* t, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[3] = {walk, scan, bank}.  tools/tones_rate.py. */
int mi_tones_set_timing(mi_tones* t, int on);
int mi_tones_last_launch_ms(mi_tones* t, float* ms /* [3] */);
/* The host twin: no GPU and no HIP call; the same state blob byte for byte, the same records and powers.  axc [rows][axc_stride];
 * waveout [rows][row_stride]; state_inout rows * MI_TONES_STATE_ROW_BYTES bytes, read and updated; records holds max_records
 * entries (max_records >= 1) and powers, if not NULL, max_records * 64 floats, of which min(count[0], max_records) = count[1] are
 * written. */
int mi_tones_plan_host(const mi_tones_cfg* cfg, const uint8_t* row_enabled, int rows, const char* axc, size_t axc_stride, int nbatches,
                       const float* waveout, size_t row_stride, void* state_inout, mi_tone_record* records, float* powers, size_t max_records,
                       uint32_t* row_first_record, uint32_t* count /* [2] */);
/* The tone table at `window` (0 = the default): freq[t], coeff[t] and alias_of[t] = the lowest index with the same coefficient
 * (t itself where the tone has a coefficient of its own).  Each output may be NULL. */
int mi_tones_table(uint32_t window, float* freq /* [51] */, float* coeff /* [51] */, uint32_t* alias_of /* [51] */);
/* From one row's records to a ctcss_freq.  A window votes for its `best` iff best_power > mean_power (the reference's second
 * condition, ctcss.cpp:150; the first, "the target is the strongest", holds for `best` by construction).  out describes the tone
 * with the most votes, the lowest index on ties (tone = freq_hz = share = 0 without any vote): windows = n, votes = that tone's,
 * share = votes / (double)windows, found iff windows >= min_windows and votes * 1000 >= min_share_permille * windows.
 * rule NULL or a field that is 0 takes its default, min_windows 2 and min_share_permille 500; min_share_permille <= 1000.  On noise
 * alone the strongest of 51 powers is several times their mean, so one window is no detection: the vote is.  The defaults are a
 * caller's settings like the finder's ratio, not tolerances; they have been tried on synthetic signals only. */
typedef struct { uint32_t min_windows, min_share_permille; } mi_tones_rule;
typedef struct {
    uint32_t windows, votes, tone;
    float freq_hz;
    double share;
    uint32_t found, zero;
} mi_tones_vote;                    /* 32 bytes */
int mi_tones_vote_host(const mi_tone_record* records, size_t n, const mi_tones_rule* rule /* NULL = defaults */, mi_tones_vote* out);

/* ---------------- PCM stage: the gate's blocks as 8 kHz int16 or IMA ADPCM, on the device ----------------
 * The reference hands its audio to LAME (airlame_init, src/output.cpp:147-171: in MI_WAVE_RATE 16000, out MP3_RATE 8000;
 * lame_encode_buffer_ieee_float at :478 and :534).  MP3 stays with the host.  This stage is the arithmetic between
 * the gate and a file whose every byte can be defined: a 2:1 decimating FIR, an int16 quantiser and WAV-container IMA ADPCM, which
 * any player opens.  A post-stage like the gate and the splitter: it reads the audio mi_demod_process_device wrote and the index and
 * counts mi_outgate_process_device left in device memory, and writes one encoded block per travelling block.  Block k of the output
 * encodes block k of the index for k < min(d_count[1], max_blocks); nothing is written at or beyond that.  An index entry with
 * row >= rows or batch >= nbatches cannot be reported by the device: its block is all zero bytes and nothing is read out of range.
 *
 * cfg.rate is 0 or 8000 (the default, MP3_RATE) or 16000; cfg.format is 0 or MI_PCM_S16 (the default) or MI_PCM_IMA4.  Samples per
 * block S = 1000 at 8000, 2000 at 16000; block bytes 2 S for S16 and 16 * S / 25 for IMA4 (640 or 1280): mi_pcm_block_bytes.
 *
 * Stream model.  A row's audio is one running sequence x over all batches of all calls the row was enabled in (the demodulator writes
 * every batch, whether it travels or not); samples before the handle's first call are 0.
 *   rate 16000:  y[n] = x[n]
 *   rate 8000:   output m (0 .. 999) of batch b is  y = sum over k = 0 .. 62 of h[k] * x[2000 b + 2 m - k]  in float32, every product
 *                and every sum rounded on its own, k ascending, starting from 0.0f.  Indices below 0 reach into batch b - 1 of the
 *                same row in the same call; for b = 0 into the 62 samples the handle carries for the row.
 * Taps h (mi_pcm_taps), designed in float64 and cast to float32 once, with c = k - 31: c even and not 0 gives exactly 0.0f; otherwise
 * g[k] = 0.5 * sinc(c / 2) * (0.42 - 0.5 cos(2 pi k / 62) + 0.08 cos(4 pi k / 62)) with sinc(t) = sin(pi t) / (pi t), sinc(0) = 1, and
 * h[k] = (float)(g[k] / sum g), with g[62 - k] taken from g[k] for k < 31 so that h is symmetric bit for bit: a half-band low-pass under a Blackman window, flat to 3 kHz and below -70 dB from 4.7 kHz.
 * Quantiser: v = y * 32767.0f (one float32 multiply), clamped to [-32767, 32767], rounded to nearest, ties to even.  NaN and Inf are
 * unspecified; the demodulator's audio is finite with |x| <= 1.
 *
 * MI_PCM_S16: the block is S little-endian int16.
 * MI_PCM_IMA4: the block is S / 25 sub-blocks of 16 bytes, each a complete mono block of WAV format 0x0011 with nBlockAlign 16 and
 * wSamplesPerBlock 25, so sub-blocks do not depend on each other.  Over samples s[0 .. 24]: header int16 LE s[0]; uint8 index0;
 * uint8 0, where with d = |s[1] - s[0]| index0 is the smallest i in 0 .. 88 with 7 * T[i] >= 4 * d, or 88 if there is none (T: the
 * standard 89-entry IMA step table); then 12 bytes with the codes of s[1] .. s[24], two a byte, the earlier sample in the LOW nibble.
 * The encoder step is the standard one, predictor p starting at s[0], index i at index0:
 *   step = T[i]; diff = s - p; sign = diff < 0 ? 8 : 0; diff = |diff|; vp = step >> 3; code = 0
 *   if diff >= step: code |= 4, diff -= step, vp += step;   step >>= 1
 *   if diff >= step: code |= 2, diff -= step, vp += step;   step >>= 1
 *   if diff >= step: code |= 1, vp += step
 *   p = sign ? p - vp : p + vp, clamped to [-32768, 32767];  i += {-1,-1,-1,-1,2,4,6,8}[code], clamped to 0 .. 88;  nibble = code | sign
 *
 * State: per row the last 62 samples of the last batch of the last call the row was enabled in, zeros at first; the blob is
 * rows * MI_PCM_STATE_ROW_BYTES bytes of little-endian float32, oldest sample first.  A disabled row's carried samples keep their
 * bytes; blocks of a disabled row that the index names anyway are encoded from whatever is there (a caller gives such rows
 * MI_GATE_NONE).  At rate 16000 the state is carried all the same, so that a checkpoint does not depend on the rate.
 * The defaults and the filter have been tried on synthetic signals only. */
enum { MI_PCM_S16 = 1, MI_PCM_IMA4 = 2, MI_PCM_TAPS = 63, MI_PCM_HISTORY = 62, MI_PCM_STATE_ROW_BYTES = 248, MI_PCM_IMA_SAMPLES = 25, MI_PCM_IMA_BYTES = 16 };
typedef struct { uint32_t rate; uint32_t format; } mi_pcm_cfg; /* 0 = 8000 / MI_PCM_S16 */
typedef struct mi_pcm mi_pcm;

/* cfg NULL = the defaults.  row_enabled [rows] as for mi_txsplit_create; rows and max_batches within the gate's limits (1 <= rows <
 * 2^20, rows * max_batches < 2^24); max_blocks: capacity of the caller's d_out in blocks, 0 = rows * max_batches. */
int mi_pcm_create(const mi_pcm_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_blocks, int gpu, mi_pcm** out);
void mi_pcm_destroy(mi_pcm* p);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_pcm_set_rows(mi_pcm* p, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches: d_waveout [rows][row_stride] with alignment and strides as for
 * mi_outgate_process_device; d_index (8-byte aligned) and d_count [2] in device memory exactly as mi_outgate_process_device left
 * them; d_out [max_blocks][mi_pcm_block_bytes] (16-byte aligned).  Asynchronous on `hip_stream`, no host synchronisation; two
 * kernels without atomics -- the encoder, then the copy of the enabled rows' new tails into the carried state -- so every byte is
 * the same on every run. */
int mi_pcm_process_device(mi_pcm* p, const float* d_waveout, size_t row_stride, int nbatches, const mi_gate_block* d_index,
                          const uint32_t* d_count, void* d_out, void* hip_stream);
/* Results of the last mi_pcm_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the two counts it
 * was given and copies exactly min(count[1], max_blocks) blocks; on return count[0] is the gate's count[0] and count[1] the number
 * of blocks copied.  out may be NULL.  The one place that synchronises. */
int mi_pcm_download(mi_pcm* p, void* hip_stream, void* out, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_PCM_STATE_ROW_BYTES bytes in the layout above (mi_pcm_plan_host reads and writes the same bytes).
 * Both complete queued work first. */
size_t mi_pcm_state_size(const mi_pcm* p);
int mi_pcm_get_state(mi_pcm* p, void* buf, size_t len);
int mi_pcm_set_state(mi_pcm* p, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[2] = {encode, tails}.  tools/pcm_rate.py. */
int mi_pcm_set_timing(mi_pcm* p, int on);
int mi_pcm_last_launch_ms(mi_pcm* p, float* ms /* [2] */);
/* Bytes of one encoded block under cfg (NULL = the defaults), 0 for a rate or format outside the sets above.  Host only. */
size_t mi_pcm_block_bytes(const mi_pcm_cfg* cfg);
/* The 63 taps h[0 .. 62].  Host only. */
int mi_pcm_taps(float* out /* [MI_PCM_TAPS] */);
/* The host twin: no GPU and no HIP call; the same bytes and the same state blob.  waveout [rows][row_stride]; index [nblocks] from
 * the host (any order, repeats allowed); out holds nblocks blocks, all of which are written; state_inout rows *
 * MI_PCM_STATE_ROW_BYTES bytes, read and updated. */
int mi_pcm_plan_host(const mi_pcm_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* waveout, size_t row_stride,
                     const mi_gate_block* index, size_t nblocks, void* state_inout, void* out);
/* The header of a WAV file of nblocks blocks: header followed by the blocks of one record of the splitter is a complete file.  S16:
 * the 44-byte PCM header.  IMA4: RIFF / WAVE with a 20-byte `fmt ` body (wFormatTag 0x0011, 1 channel, nAvgBytesPerSec = rate * 16 /
 * 25, nBlockAlign 16, wBitsPerSample 4, cbSize 2, wSamplesPerBlock 25), a `fact` chunk with the sample count, then `data`: 60 bytes.
 * *len = the header's length; MI_ERR_INVALID if cap is below it or the file would pass 2^32 - 1 bytes. */
int mi_pcm_wav_header(const mi_pcm_cfg* cfg, uint64_t nblocks, void* buf, size_t cap, size_t* len);

/* ---------------- audio spectrum stage: a power spectrum per travelling block, a long-term spectrum per row ----------------
 * Every channel of the reference has a `notch` key (config.cpp:388-392, 519-567; filters.cpp:30-64) and stage 2 honours
 * mi_channel_cfg.notch_freq / notch_q; this stage is what tells a caller what to put there.  What a notch removes -- the whistle of
 * offset-carrier (CLIMAX) AM operation, a sub-audible tone that leaks through, mains hum -- is a steady narrow line in the open
 * audio, which the 51-tone bank of mi_tones_* cannot see.  A post-stage like the PCM stage: it reads the audio
 * mi_demod_process_device wrote and the index, row starts and counts mi_outgate_process_device left in device memory, and writes one
 * record (and optionally one power row) per travelling block and one mean spectrum per row.  It is stateless: nothing is carried
 * between calls, there is no row mask and no state blob.
 *
 * Frame.  Block k of the index, (row, batch), is the 2000 samples x[0 .. 1999] of d_waveout at row * row_stride + batch * 2000.
 * Window.  w[i] = (float)(0.5 - 0.5 cos(2 pi i / 1999)), i = 0 .. 1999 (Hann), evaluated in float64 for i <= 999 and mirrored,
 *   w[1999 - i] = w[i], so that it is symmetric bit for bit: mi_aspec_window.  The device gets that table from the host.
 * Input.  u[i] = x[i] * w[i], one float32 multiply; u[2000 .. 2047] = 0.0f; the FFT input is the complex sequence (u[i], 0.0f).
 * Spectrum.  X = the documented FFT at N = MI_ASPEC_FFT = 2048 with the twiddles mi_plan_twiddles gives at
 *   fft_size_log 11 (the table depends on N only).  P[j] = X[j].re * X[j].re + X[j].im * X[j].im for j = 0 .. MI_ASPEC_BINS - 1, both
 *   products and the sum rounded on their own in float32; no square root.  Bin j is j * MI_WAVE_RATE / 2048 = j * 7.8125 Hz.  The
 *   real-input halving trick is not used and nothing is pruned for the zero imaginary parts: the full graph is the definition.
 * Band.  mi_aspec_cfg { lo_hz, hi_hz }, 0 = the default 60 / 3800.  lo_bin = (lo_hz * 2048 + 15999) / 16000 and hi_bin = hi_hz * 2048
 *   / 16000 in integers; a configuration is refused unless 1 <= lo_bin <= hi_bin <= 1023.  mi_aspec_band returns the two bins; the
 *   defaults give 8 and 486.
 * Record of block k (mi_aspec_record, 32 bytes):
 *   peak_bin    the bin in [lo_bin, hi_bin] with the largest P, the lowest bin on ties;  peak_power = its P
 *   band_power  a float64 sum of P over the band in this order: thread t of 256 adds, bins ascending, those of the bins t, t + 256,
 *               t + 512, t + 768 that lie in the band (starting from 0.0); then acc[t] += acc[t + d] for t < d, d = 128, 64, .., 1;
 *               band_power = acc[0]
 *   line_power  the float64 sum of P[peak_bin - MI_ASPEC_LINE_HALF .. peak_bin + MI_ASPEC_LINE_HALF], clipped to the band, bins ascending
 *   An index entry with row >= rows or batch >= nbatches gives the record {row, batch, 0xFFFFFFFF, 0, 0, 0} and a power row of
 *   zeros; nothing is read out of range.  NaN and Inf in the audio are unspecified, as everywhere behind the demodulator.
 * Power rows.  d_power [max_blocks][1024], optional: row k holds P[0 .. 1023] of block k.
 * Row mean.  d_row_mean [rows][1024] and d_row_blocks [rows], optional (both or neither).  With stored = min(d_count[1], max_blocks),
 *   row r's blocks are the k in [d_row_first[r], d_row_first[r + 1]) that lie in [0, stored), n of them: row_blocks[r] = n and
 *   row_mean[r][j] = (float)(S / n) with S the float64 sum of d_power[k][j] over those k ascending; n = 0 gives zeros.  A non-NULL
 *   d_row_mean needs d_power, d_row_first and d_row_blocks, else the call is refused: the handle allocates no per-block scratch.
 * Nothing is written at or beyond `stored` in d_records or d_power.
 * Execution: asynchronous on `hip_stream`, no host synchronisation; one kernel (one workgroup per block), and a second one (one
 *   thread per row and bin) only when a row mean is wanted.  No atomics: every byte is the same on every run and equals
 *   mi_aspec_plan_host's.  mi_aspec_download is the one place that synchronises.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, a refused band, misaligned buffers, nbatches
 * outside 1 .. max_batches, or a row mean without what it needs. */
enum { MI_ASPEC_FFT_LOG = 11, MI_ASPEC_FFT = 2048, MI_ASPEC_BINS = 1024, MI_ASPEC_LINE_HALF = 2 };
typedef struct { uint32_t lo_hz, hi_hz; } mi_aspec_cfg; /* 0 = 60 / 3800 */
typedef struct {
    uint32_t row, batch;
    uint32_t peak_bin;  /* 0xFFFFFFFF: not an entry of this call */
    float peak_power;
    double band_power, line_power;
} mi_aspec_record; /* 32 bytes */
typedef struct mi_aspec mi_aspec;

/* cfg NULL = the defaults.  rows and max_batches within the gate's limits (1 <= rows < 2^20, rows * max_batches < 2^24);
 * max_blocks: capacity of the caller's d_records (and d_power) in blocks, 0 = rows * max_batches. */
int mi_aspec_create(const mi_aspec_cfg* cfg, int rows, int max_batches, size_t max_blocks, int gpu, mi_aspec** out);
void mi_aspec_destroy(mi_aspec* a);
/* One call over nbatches (1 .. max_batches) batches: d_waveout [rows][row_stride] with alignment and strides as for
 * mi_outgate_process_device; d_index (8-byte aligned), d_row_first [rows + 1] (may be NULL without a row mean) and d_count [2] in
 * device memory exactly as mi_outgate_process_device left them; d_records [max_blocks] (8-byte aligned); d_power [max_blocks][1024]
 * or NULL and d_row_mean [rows][1024] or NULL (16-byte aligned); d_row_blocks [rows], non-NULL exactly when d_row_mean is. */
int mi_aspec_process_device(mi_aspec* a, const float* d_waveout, size_t row_stride, int nbatches, const mi_gate_block* d_index,
                            const uint32_t* d_row_first, const uint32_t* d_count, mi_aspec_record* d_records, float* d_power, float* d_row_mean,
                            uint32_t* d_row_blocks, void* hip_stream);
/* Results of the last mi_aspec_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the two counts it
 * was given and copies exactly min(count[1], max_blocks) records and power rows, rows * 1024 means and rows block counts; on return
 * count[0] is the gate's count[0] and count[1] the number of records copied.  Each destination may be NULL; one the call did not
 * write (power, row_mean, row_blocks) is refused.  The one place that synchronises. */
int mi_aspec_download(mi_aspec* a, void* hip_stream, mi_aspec_record* records, float* power, float* row_mean, uint32_t* row_blocks,
                      uint32_t* count /* [2] */);
/* (diagnostic) as mi_outgate_set_timing; ms[2] = {blocks, rows}; rows is 0 for a call without a row mean.  tools/aspec_rate.py. */
int mi_aspec_set_timing(mi_aspec* a, int on);
int mi_aspec_last_launch_ms(mi_aspec* a, float* ms /* [2] */);
/* The 2000 window coefficients.  Host only. */
int mi_aspec_window(float* out /* [MI_WAVE_BATCH] */);
/* lo_bin and hi_bin under cfg (NULL = the defaults), or the refusal.  Host only. */
int mi_aspec_band(const mi_aspec_cfg* cfg, uint32_t* lo_bin, uint32_t* hi_bin);
/* The host twin: no GPU and no HIP call; the same bytes.  waveout [rows][row_stride]; index [nblocks] from the host (any order,
 * repeats allowed), stored = nblocks; records holds nblocks entries and power, if not NULL, nblocks * 1024 floats, all of which are
 * written; row_first [rows + 1], row_mean [rows][1024] and row_blocks [rows] follow the rule above (row_mean needs power, row_first
 * and row_blocks).  The rows are cut by row_first alone, whatever rows the entries name. */
int mi_aspec_plan_host(const mi_aspec_cfg* cfg, int rows, int nbatches, const float* waveout, size_t row_stride, const mi_gate_block* index,
                       size_t nblocks, const uint32_t* row_first, mi_aspec_record* records, float* power, float* row_mean, uint32_t* row_blocks);

/* From a row's mean spectrum to a notch_freq: no GPU and no HIP call, float64 except where stated.  With [lo_bin, hi_bin] of cfg:
 *   p        the band bin with the largest mean, the lowest bin on ties
 *   floor    the median of the means of the band bins j with 3 <= |j - p| <= 34 (a line under the Hann window covers p - 2 .. p + 2;
 *            34 bins are 266 Hz): the element at index (m - 1) / 2 of those m values sorted ascending; 0 when m = 0
 *   found    iff row_blocks >= min_blocks and mean[p] > 0 and mean[p] > ratio * floor, the product one float32 multiply
 *   freq_hz  7.8125 * (sum of j * mean[j]) / (sum of mean[j]) over j = p - 1 .. p + 1 clipped to the band, j ascending; 7.8125 * p
 *            where the second sum is 0
 *   votes    the number of the given records (the row's: records[row_first[r] .. row_first[r + 1])) with |peak_bin - p| <= 1; it is
 *            reported, it is not a condition
 *   peak = mean[p], blocks = row_blocks.
 * rule NULL or a field that is 0 takes its default: min_blocks 8 (one second of open audio), ratio 16.0f.  The defaults are a
 * caller's settings like the finder's ratio, not tolerances; they have been tried on synthetic signals only (DESIGN.md 5j has the
 * table).  The function suggests no Q: the reference's default notch_q of 10 stays the caller's choice.  records may be NULL with
 * n = 0.  MI_ERR_INVALID: NULL arguments, a refused band, a ratio that is negative or not finite. */
typedef struct { uint32_t min_blocks; float ratio; } mi_aspec_rule; /* 0 = 8 / 16.0f */
typedef struct {
    uint32_t found, bin;
    double freq_hz, peak, floor;
    uint32_t votes, blocks;
} mi_aspec_notch; /* 40 bytes */
int mi_aspec_notch_host(const float* row_mean /* [1024] */, uint32_t row_blocks, const mi_aspec_record* records, size_t n,
                        const mi_aspec_cfg* cfg /* NULL = defaults */, const mi_aspec_rule* rule /* NULL = defaults */, mi_aspec_notch* out);

/* ---------------- voice band stage: per-row highpass / lowpass FIR over the demodulator's audio, on the device ----------------
 * Every channel and every mixer of the reference has a `highpass` and a `lowpass` key (config.cpp:327-328, defaults 100 and 2500 Hz,
 * checked at :336-338) whose only effect is in airlame_init (output.cpp:147-171: lame_set_highpassfreq / lame_set_lowpassfreq): the
 * reference shapes the audio band inside the MP3 encoder.  The device chain has no encoder; this stage is where the two keys act.  A
 * post-stage like the PCM stage: it reads the audio mi_demod_process_device wrote and writes a filtered plane in the same layout,
 * d_out [rows][out_stride], so the gate, the splitter, the PCM stage, the spectrum stage and the mixer run on it unchanged.  The
 * stage filters every batch of every enabled row, whether it travels or not: there is no index and no download entry, and the PCM
 * stage's 62-sample reach into a batch that does not travel reads defined values.  mi_tones_* and mi_aspec_* are meant to keep
 * reading the unfiltered plane: what they look for is what this stage removes.
 *
 * Stream model.  As for the PCM stage: a row's audio is one running sequence x over all batches of all calls the row was enabled in;
 * samples before the handle's first call are 0.
 * Row settings.  mi_vband_row { hp_hz, lp_hz } per row: hp_hz = 0 means no lower edge, lp_hz = 0 no upper edge, both 0 a pure delay,
 * which keeps rows aligned for the mixer.  Settings are refused unless hp_hz == 0 || 50 <= hp_hz <= 4000, lp_hz == 0 || 500 <= lp_hz
 * <= 7800, and lp_hz == 0 || lp_hz >= hp_hz + 200 -- those of a disabled row too.  mi_vband_default_row gives 100 / 2500, the
 * reference's defaults.
 * Taps h (mi_vband_taps), MI_VBAND_TAPS = 511 with the centre at 255, designed in float64 and cast to float32 once.  With c = k - 255,
 * fl = hp_hz / 16000.0 and fh = lp_hz / 16000.0:
 *   g[k] = (U(c) - 2 fl sinc(2 fl c)) * (0.42 - 0.5 cos(2 pi k / 510) + 0.08 cos(4 pi k / 510))
 *   U(c) = 2 fh sinc(2 fh c) where lp_hz != 0; where lp_hz == 0 (fh = 0.5: the whole band) U(0) = 1 and U(c) = 0 otherwise, exactly
 * with sinc(t) = sin(pi t) / (pi t) and sinc(0) = 1, evaluated for k <= 255; h[k] = (float)g[k] and h[510 - k] = h[k], so that h is
 * symmetric bit for bit.  There is no normalisation.  Both settings 0 give exactly a unit impulse at tap 255.  A windowed-sinc band
 * filter under a Blackman window: within +-0.01 dB from 100 Hz inside each edge, below -70 dB from 100 Hz outside it (DESIGN.md has
 * the measured table).
 * Output.  Sample n of the row's sequence:  y[n] = sum over k = 0 .. 510 of h[k] * x[n - k]  in float32, every product and every sum
 * rounded on its own, k ascending, starting from 0.0f; no fused multiply-add and no folding of the symmetric taps.  Then
 * out = fminf(fmaxf(y, -1.0f), 1.0f): sum |h| is 2.5 to 3.0 for usual settings and everything behind the demodulator relies on
 * |x| <= 1 (the reference clamps at the same place in its own gate, rtl_airband.cpp:612-641).  Indices below the call's first sample
 * reach into the 510 samples the handle carries for the row.  NaN and Inf are unspecified, as everywhere behind the demodulator.
 *   Where all 2510 samples a block's outputs depend on compare equal to zero, the definition gives +0.0f throughout (products of +-0
 *   added to +0.0f stay +0.0f); the device writes that without summing.  No byte depends on it.
 * Delay.  The filter is causal and delays the audio by 255 samples (15.9 ms) against the demodulator's flags: the last samples of a
 * transmission can land in the batch after the one whose flag closes.  A caller keeps them with the gate's open trail
 * (MI_GATE_OPEN_TRAIL), which lets that batch travel.
 * State: per row the last 510 input samples of the last batch of the last call the row was enabled in, zeros at first; the blob is
 * rows * MI_VBAND_STATE_ROW_BYTES bytes of little-endian float32, oldest sample first.  A disabled row's output row is not written
 * and its carried samples keep their bytes.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned or overlapping
 * buffers, nbatches outside 1 .. max_batches. */
enum { MI_VBAND_TAPS = 511, MI_VBAND_HISTORY = 510, MI_VBAND_STATE_ROW_BYTES = 2040 };
typedef struct { uint32_t hp_hz, lp_hz; } mi_vband_row; /* 0 = no edge on that side */
typedef struct mi_vband mi_vband;

/* { 100, 2500 }: the reference's defaults (config.cpp:327-328). */
mi_vband_row mi_vband_default_row(void);
/* row_cfg [rows] (NULL = the default row everywhere); row_enabled [rows] as for mi_pcm_create; rows and max_batches within the
 * gate's limits (1 <= rows < 2^20, rows * max_batches < 2^24).  Rows with equal settings share one tap table on the device. */
int mi_vband_create(const mi_vband_row* row_cfg /* [rows] */, const uint8_t* row_enabled, int rows, int max_batches, int gpu, mi_vband** out);
void mi_vband_destroy(mi_vband* v);
/* Other settings (row_cfg [rows], NULL = keep) and / or other rows (row_enabled [rows], NULL = keep) from the next call on; at least
 * one of the two.  All state stays.  Completes the work queued on the device first. */
int mi_vband_set_rows(mi_vband* v, const mi_vband_row* row_cfg, const uint8_t* row_enabled);
/* One call over nbatches (1 .. max_batches) batches: d_waveout [rows][row_stride] and d_out [rows][out_stride], both 16-byte
 * aligned with strides that are multiples of 4 floats and at least nbatches * 2000; the two planes must not overlap (the call is
 * refused when they do).  Asynchronous on `hip_stream`, no host synchronisation; two kernels without atomics -- the filter, then the
 * copy of the enabled rows' last 510 input samples into the carried state -- so every byte is the same on every run and equals
 * mi_vband_plan_host's. */
int mi_vband_process_device(mi_vband* v, const float* d_waveout, size_t row_stride, int nbatches, float* d_out, size_t out_stride, void* hip_stream);
/* Checkpoint / resume, rows * MI_VBAND_STATE_ROW_BYTES bytes in the layout above (mi_vband_plan_host reads and writes the same
 * bytes).  Both complete queued work first. */
size_t mi_vband_state_size(const mi_vband* v);
int mi_vband_get_state(mi_vband* v, void* buf, size_t len);
int mi_vband_set_state(mi_vband* v, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[2] = {filter, tails}.  tools/vband_rate.py. */
int mi_vband_set_timing(mi_vband* v, int on);
int mi_vband_last_launch_ms(mi_vband* v, float* ms /* [2] */);
/* The 511 taps h[0 .. 510] of a row with these settings, or the settings' refusal.  Host only. */
int mi_vband_taps(uint32_t hp_hz, uint32_t lp_hz, float* out /* [MI_VBAND_TAPS] */);
/* The host twin: no GPU and no HIP call; the same bytes and the same state blob.  waveout [rows][row_stride], out [rows][out_stride]
 * (no alignment asked, no overlap allowed); state_inout rows * MI_VBAND_STATE_ROW_BYTES bytes, read and updated. */
int mi_vband_plan_host(const mi_vband_row* row_cfg /* [rows], NULL = defaults */, const uint8_t* row_enabled, int rows, int nbatches,
                       const float* waveout, size_t row_stride, void* state_inout, float* out, size_t out_stride);

/* ---------------- peak limiter stage: look-ahead gain per row, on the device ----------------
 * Nothing else behind the demodulator bounds the level of the audio without clipping it: mi_mixer_process_device adds its open inputs
 * and does not clamp (the reference leaves that to LAME), a channel's ampfactor (config.cpp:623) is multiplied in just before the
 * demodulator's hard clamp, mi_vband_* ends in a clamp, and the PCM stage's int16 quantiser saturates.  This stage keeps peaks inside
 * a ceiling by turning the gain down ahead of them.  A post-stage like the voice band stage: it reads a plane [rows][row_stride] of
 * float32 audio -- what mi_demod_process_device, mi_vband_process_device or mi_mixer_process_device wrote; a mixer's d_left is a plane
 * of one row -- and writes a plane d_out [rows][out_stride] of the same layout, which the gate, the splitter, the PCM stage and the
 * mixer take in its place.  Every batch of every enabled row is handled: there is no index and no download entry.
 *
 * Stream model.  As for the voice band stage: a row's audio is one running sequence x over all batches of all calls the row was
 * enabled in; samples before the handle's first call are 0.
 * Constants.  The look-ahead and delay D = MI_LIMIT_LOOKAHEAD = 63 samples (3.9 ms).  The peak window W = MI_LIMIT_WINDOW = 1024
 * samples: 63 ahead of the sample being scaled, that sample, and 960 behind it (a hold of 60 ms).  The gain is the mean of D + 1 = 64
 * values, a power of two, so the division is exact.  The history is D + W - 1 = MI_LIMIT_HISTORY = 1086 samples.
 * Row settings.  mi_limit_row { pregain, ceiling } per row.  Settings are refused unless both are finite, 2^-10 <= pregain <= 2^10
 * and 0.0625f <= ceiling <= 1.0f -- those of a disabled row too.  mi_limit_default_row gives { 1.0f, 0.89125094f } (-1 dBFS).
 * Output.  Sample n of the row's sequence, everything float32, every operation rounded on its own, no fused multiply-add:
 *   u[n] = x[n] * pregain
 *   a[n] = fabsf(u[n])
 *   p[n] = max over k = 0 .. 1023 of a[n - k]                      (order-free)
 *   r[n] = p[n] > ceiling ? ceiling / p[n] : 1.0f                  (the correctly rounded IEEE division)
 *   s[n] = ((0.0f + r[n - 63]) + r[n - 62]) + ... + r[n]           (m ascending)
 *   g[n] = s[n] * 0.015625f                                        (exact)
 *   y[n] = u[n - 63] * g[n]
 *   out[n] = fminf(fmaxf(y[n], -ceiling), ceiling)
 * Indices below the call's first sample reach into the 1086 input samples x the handle carries for the row -- x, not u: after
 * mi_limit_set_rows the carried samples count under the new pregain.  NaN and Inf are unspecified, as everywhere behind the
 * demodulator.  Inputs beyond +-1, such as a mixer's sum, are what the stage is for and are fully specified.
 * What follows from the definition:
 *   1. Ceiling.  Each r[m] with m in [n - 63, n] has u[n - 63] inside its window, so in exact arithmetic g[n] * |u[n - 63]| <= ceiling.
 *      The float32 chain adds at most about 70 relative roundings of 2^-24 (one division, 63 additions, one product): |y| exceeds the
 *      ceiling by a few parts in 10^6 at most, and the final clamp moves such a value by a few float32 steps.  |out| <= ceiling holds
 *      exactly.
 *   2. Transparency.  Where no a[] within a sample's reach exceeds the ceiling, every r is 1.0f, s exactly 64.0f and g exactly 1.0f:
 *      out[n] is u[n - 63] bit for bit, signed zeros and subnormal values included.  The device writes a block whose 3086 staged
 *      values a[] have a maximum that is not over the ceiling without the sliding maximum, the division and the sum.  No byte depends
 *      on which path ran.
 *   3. A lone peak at index q of a row that is otherwise under the ceiling.  The gain leaves 1.0f first for the output that carries
 *      input sample q - 63; it is lowest, <= ceiling / a[q] apart from the rounding of item 1, for input samples q .. q + 960; it is
 *      exactly 1.0f again from input sample q + 1024 on.
 *   4. Steady signal.  A steady tone or square wave over the ceiling gives a constant p from sample 1023 of its steady part, hence
 *      constant r and g: the output is the input times one number, without distortion.
 * Delay.  Output sample n carries input sample n - 63.  Behind mi_vband_* the two delays add to 318 samples; a caller keeps a
 * transmission's tail with the gate's open trail (MI_GATE_OPEN_TRAIL), as for the voice band stage.
 * Rows are independent: there is no stereo link between a mixer's left and right row, so a peak on one side leaves the other side's
 * gain alone and the image may shift for the length of the hold.  A linked mode is not part of this stage.
 * State: per row the last 1086 input samples of the last batch of the last call the row was enabled in, zeros at first; the blob is
 * rows * MI_LIMIT_STATE_ROW_BYTES bytes of little-endian float32, oldest sample first.  A disabled row's output row is not written
 * and its carried samples keep their bytes.
 * The defaults (ceiling, look-ahead, window) and mi_limit_pregain_host were tried on synthetic signals only.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned or overlapping
 * buffers, nbatches outside 1 .. max_batches. */
enum { MI_LIMIT_LOOKAHEAD = 63, MI_LIMIT_WINDOW = 1024, MI_LIMIT_HISTORY = 1086, MI_LIMIT_STATE_ROW_BYTES = 4344 };
typedef struct { float pregain; float ceiling; } mi_limit_row;
typedef struct mi_limit mi_limit;

/* { 1.0f, 0.89125094f }: no gain in front, a ceiling of -1 dBFS. */
mi_limit_row mi_limit_default_row(void);
/* row_cfg [rows] (NULL = the default row everywhere); row_enabled [rows] as for mi_vband_create; rows and max_batches within the
 * gate's limits (1 <= rows < 2^20, rows * max_batches < 2^24). */
int mi_limit_create(const mi_limit_row* row_cfg /* [rows] */, const uint8_t* row_enabled, int rows, int max_batches, int gpu, mi_limit** out);
void mi_limit_destroy(mi_limit* l);
/* Other settings (row_cfg [rows], NULL = keep) and / or other rows (row_enabled [rows], NULL = keep) from the next call on; at least
 * one of the two.  All state stays.  Completes the work queued on the device first. */
int mi_limit_set_rows(mi_limit* l, const mi_limit_row* row_cfg, const uint8_t* row_enabled);
/* One call over nbatches (1 .. max_batches) batches: d_in [rows][row_stride] and d_out [rows][out_stride], both 16-byte aligned with
 * strides that are multiples of 4 floats and at least nbatches * 2000; the two planes must not overlap (the call is refused when
 * they do).  Asynchronous on `hip_stream`, no host synchronisation; two kernels without atomics -- the limiter, then the copy of the
 * enabled rows' last 1086 input samples into the carried state -- so every byte is the same on every run and equals
 * mi_limit_plan_host's. */
int mi_limit_process_device(mi_limit* l, const float* d_in, size_t row_stride, int nbatches, float* d_out, size_t out_stride, void* hip_stream);
/* Checkpoint / resume, rows * MI_LIMIT_STATE_ROW_BYTES bytes in the layout above (mi_limit_plan_host reads and writes the same
 * bytes).  Both complete queued work first. */
size_t mi_limit_state_size(const mi_limit* l);
int mi_limit_get_state(mi_limit* l, void* buf, size_t len);
int mi_limit_set_state(mi_limit* l, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[2] = {limit, tails}.  tools/limit_rate.py. */
int mi_limit_set_timing(mi_limit* l, int on);
int mi_limit_last_launch_ms(mi_limit* l, float* ms /* [2] */);
/* The host twin: no GPU and no HIP call; the same bytes and the same state blob.  in [rows][row_stride], out [rows][out_stride] (no
 * alignment asked, no overlap allowed); state_inout rows * MI_LIMIT_STATE_ROW_BYTES bytes, read and updated. */
int mi_limit_plan_host(const mi_limit_row* row_cfg /* [rows], NULL = defaults */, const uint8_t* row_enabled, int rows, int nbatches,
                       const float* in, size_t row_stride, void* state_inout, float* out, size_t out_stride);
/* A pregain for one row from what the splitter recorded of it, host only.  Of records[0 .. n) those with this row, nblocks > 0 and
 * peak > 0 count, *used of them; their peaks are sorted ascending and the one at index (used - 1) * percentile / 100 (in integers;
 * percentile 1 .. 100, 0 = 90) is taken: *pregain = ceiling / that peak as a float32 division, clamped into [2^-10, 2^10], or 1.0f
 * where used == 0.  records may be NULL with n = 0.  MI_ERR_INVALID: NULL arguments, a ceiling mi_limit_create would refuse, a
 * percentile over 100.  Tried on synthetic signals only. */
int mi_limit_pregain_host(const mi_tx_record* records, size_t n, uint32_t row, float ceiling, uint32_t percentile, float* pregain, uint32_t* used);

/* ---------------- noise reduction stage: spectral gate per row, on the device ----------------
 * Nothing else behind the demodulator lowers the broadband hiss under an open AM transmission: the squelch chooses between a whole
 * batch and silence, and the reference hands waveout to LAME as it is (output.cpp:147-171).  This stage estimates the noise floor of
 * a row per frequency bin from the minima of its own recent short-time spectra and turns every bin down that does not stand above
 * it.  A post-stage like the voice band stage: it reads a plane [rows][row_stride] of float32 audio and writes a plane d_out
 * [rows][out_stride] of the same layout, which the voice band stage, the limiter, the gate, the splitter, the PCM stage and the mixer
 * take in its place.  Every batch of every enabled row is handled: there is no index and no download entry.  There is no recursion
 * in time -- minima over a window stand where running averages would --, so every (row, batch) block is computed on its own.
 *
 * Stream model.  As for the voice band stage: a row's audio is one running sequence x over all batches of all calls the row was
 * enabled in; samples before the handle's first call are 0.
 * Frames are aligned to batches: hop H = MI_DENOISE_HOP = 250 (eight per batch), length MI_DENOISE_FRAME = 500, transform length
 * MI_DENOISE_FFT = 512, bins k = 0 .. 256 (MI_DENOISE_BINS = 257, 31.25 Hz each).  Frame f covers x[250 (f - 1) .. 250 (f + 1)): with
 * b the batch, frames 8b .. 8b + 7 begin in the 250 samples before each eighth of batch b and frame 8b - 1 is the last 500 samples
 * before it.
 * Window w (mi_denoise_window): w[i] = (float) sin(pi (i + 0.5) / 500), evaluated in float64 for i <= 249; w[499 - i] = w[i], so that w
 * is symmetric bit for bit.  u[i] = x[250 (f - 1) + i] * w[i] for i < 500, twelve zeros behind them.  The same window is used for
 * synthesis: w[i]^2 + w[i + 250]^2 = 1, so gains of 1 give back x delayed by 250 samples, up to rounding.
 * Per frame.  X = the FFT spec of DESIGN.md 2 at log2n 9 of (u, 0.0f).  P[k] = re * re + im * im for k = 0 .. 256, three float32
 * operations.  A frame is SILENT when all 500 of its samples x compare equal to zero.  With T_f[k] = (P_f[k - 1] + P_f[k]) + P_f[k + 1]
 * in that order, the bin index mirrored at the ends (k - 1 at k = 0 is bin 1, k + 1 at k = 256 is bin 255), the smoothed power is
 *   S_f[k] = T_{f-1}[k] + T_f[k]
 * and frame f COUNTS when neither f - 1 nor f is silent.
 * Noise estimate, per row and batch b.  M_b[k] = the minimum of S_f[k] over the counting frames f = 8b .. 8b + 7, +Inf when none
 * counts.  m[k] = the minimum of M_{b-7} .. M_b: MI_DENOISE_DEPTH = 8 batches, one second of history with the current batch.
 * N_b[k] = over * m[k], and 0.0f where m[k] is +Inf: with no evidence the stage is transparent.
 * Gain.  A block -- the nine frames f = 8b - 1 .. 8b + 7 that batch b's outputs are made of -- uses the noise estimate of its own batch
 * for all nine, and nothing outside x[2000 b - 500 .. 2000 b + 2000): its first frame 8b - 1 has no frame in front of it there and
 * takes the smoothed power of the frame behind it, S_{8b}, which covers its span as well.  Per frame and bin, with S that power:
 *   g[k] = g_min                                    where N_b[k] >= S[k]
 *   g[k] = fmaxf(g_min, 1.0f - N_b[k] / S[k])       otherwise (the correctly rounded IEEE division, then one subtraction)
 * g_min = (float) 10^(-reduction_db / 20), computed in float64 on the host.  Frame 8b - 1 gets the gains of batch b here, for the
 * half of it that batch b's outputs hold, and it got those of batch b - 1 as frame 8 (b - 1) + 7 of the block before, for the other
 * half: both halves are well defined because each block uses only its own gains, and no block waits for another.
 * Synthesis.  Y[k] = g[min(k, 512 - k)] * X[k] for all 512 bins, two float32 products.  z = Re(FFT(conj(Y))) * (1.0f / 512): the same
 * forward graph on (Y.re, -Y.im), the scale an exact power of two.  v_f[i] = z[i] * w[i] for i < 500.  Sample n of the row's sequence
 * lies in segment s = n div 250:  y[n] = v_s[i + 250] + v_{s+1}[i]  with i = n mod 250, one float32 addition.  The plane holds
 *   out[n] = fminf(fmaxf(y[n - 250], -1.0f), 1.0f)
 * A batch's outputs depend on x from 500 samples before the batch to its end.  NaN and Inf are unspecified, as everywhere behind the
 * demodulator.
 * Delay.  250 samples (15.6 ms) against the demodulator's flags; a caller keeps a transmission's last samples with the gate's open
 * trail (MI_GATE_OPEN_TRAIL), as for the voice band stage.
 * Row settings.  mi_denoise_row { reduction_db, over } per row, refused unless 0 <= reduction_db <= 40 and 0 <= over <= 64 (NaN is
 * refused) -- those of a disabled row too.  reduction_db = 0 or over = 0 gives a pure delay, up to rounding, which keeps rows aligned
 * for the mixer.
 * State: per row the last 500 input samples of the last batch of the last call the row was enabled in, oldest first, zeros at first;
 * then M of the last seven batches, oldest first, 7 x 257 float32, +Inf at first.  The blob is rows * MI_DENOISE_STATE_ROW_BYTES bytes,
 * little-endian.  A disabled row's output row is not written and its state keeps its bytes.
 * The defaults were tried on synthetic signals only (tools/denoise_classes.py).
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned or overlapping
 * buffers, nbatches outside 1 .. max_batches. */
enum { MI_DENOISE_HOP = 250, MI_DENOISE_FRAME = 500, MI_DENOISE_FFT_LOG = 9, MI_DENOISE_FFT = 512, MI_DENOISE_BINS = 257, MI_DENOISE_DEPTH = 8,
       MI_DENOISE_STATE_ROW_BYTES = 9196 };
typedef struct { float reduction_db; float over; } mi_denoise_row;
typedef struct mi_denoise mi_denoise;

/* { 12.0f, 4.5f }.  over: mean(S) / mean(m) on seeded white Gaussian noise (20 s; sigma 0.003, 0.03, 0.3: 4.26, 4.29, 4.25, mean
 * 4.27), rounded up to the next 0.5 so that the estimate sits slightly above the floor and residual "musical" noise stays down
 * (tools/denoise_classes.py through the host twin, on the CPU).  At this row white noise comes out 9.2 dB lower after a second, and
 * so does whatever else stands still for a second: a steady 1 kHz tone 10 dB above the noise in its bin loses 12.0 dB. */
mi_denoise_row mi_denoise_default_row(void);
/* row_cfg [rows] (NULL = the default row everywhere); row_enabled [rows] as for mi_vband_create; rows and max_batches within the
 * gate's limits (1 <= rows < 2^20, rows * max_batches < 2^24).  The handle owns the scratch for M of a call's batches,
 * [rows][max_batches][257] float32. */
int mi_denoise_create(const mi_denoise_row* row_cfg /* [rows] */, const uint8_t* row_enabled, int rows, int max_batches, int gpu, mi_denoise** out);
void mi_denoise_destroy(mi_denoise* d);
/* Other settings (row_cfg [rows], NULL = keep) and / or other rows (row_enabled [rows], NULL = keep) from the next call on; at least
 * one of the two.  All state stays.  Completes the work queued on the device first. */
int mi_denoise_set_rows(mi_denoise* d, const mi_denoise_row* row_cfg, const uint8_t* row_enabled);
/* One call over nbatches (1 .. max_batches) batches: d_in [rows][row_stride] and d_out [rows][out_stride], both 16-byte aligned with
 * strides that are multiples of 4 floats and at least nbatches * 2000; the two planes must not overlap (the call is refused when
 * they do).  Asynchronous on `hip_stream`, no host synchronisation; three kernels without atomics -- M of every block into the
 * scratch, then the gains and the synthesis, then the enabled rows' last 500 input samples and last seven M into the carried state
 * -- so every byte is the same on every run and equals mi_denoise_plan_host's. */
int mi_denoise_process_device(mi_denoise* d, const float* d_in, size_t row_stride, int nbatches, float* d_out, size_t out_stride, void* hip_stream);
/* Checkpoint / resume, rows * MI_DENOISE_STATE_ROW_BYTES bytes in the layout above (mi_denoise_plan_host reads and writes the same
 * bytes).  Both complete queued work first. */
size_t mi_denoise_state_size(const mi_denoise* d);
int mi_denoise_get_state(mi_denoise* d, void* buf, size_t len);
int mi_denoise_set_state(mi_denoise* d, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[3] = {floor, apply, tails}.  tools/denoise_rate.py. */
int mi_denoise_set_timing(mi_denoise* d, int on);
int mi_denoise_last_launch_ms(mi_denoise* d, float* ms /* [3] */);
/* The 500 window coefficients w[0 .. 499].  Host only. */
int mi_denoise_window(float* out /* [MI_DENOISE_FRAME] */);
/* The host twin: no GPU and no HIP call; the same bytes and the same state blob.  in [rows][row_stride], out [rows][out_stride] (no
 * alignment asked, no overlap allowed); state_inout rows * MI_DENOISE_STATE_ROW_BYTES bytes, read and updated (a fresh blob: zeros
 * in the samples, +Inf in M). */
int mi_denoise_plan_host(const mi_denoise_row* row_cfg /* [rows], NULL = defaults */, const uint8_t* row_enabled, int rows, int nbatches,
                         const float* in, size_t row_stride, void* state_inout, float* out, size_t out_stride);

/* ---------------- SELCAL decoder stage: tone-pair codes per row, on the device ----------------
 * SELCAL is the selective calling of the aeronautical bands: a call is two pulses of about 1 s, about 0.2 s apart, each pulse two
 * simultaneous audio tones out of a table of 16 (32 with the SELCAL 32 extension); the letters of the four tones are the code
 * ("AB-CD").  The reference leaves the chirps in the recording; mi_tones_* answers "which CTCSS tone?" and mi_aspec_* "which steady
 * whistle?", and neither sees two tones at once, a pulse's length or a sequence of pulses.  This stage answers "which aircraft was
 * called?": one code record per call, with row and time.  A post-stage in the tone finder's mould: it reads a plane
 * [rows][row_stride] of float32 audio -- the demodulator's d_waveout, or what the noise reduction, the voice band stage, the limiter
 * or a mixer wrote in its place -- and writes records.  It takes no d_axc: a closed batch is zeros and decides itself (item 0 below).
 *
 * Tone tables (mi_selcal_table).  Tones are indexed in ascending frequency; coeff[t] = (float)(2 cos(2 pi f_t / 16000)), evaluated
 * in float64 from the float32 literal.
 *   MI_SELCAL_16 (the default), the classic table:
 *     A 312.6  B 346.7  C 384.6  D 426.6  E 473.2  F 524.8  G 582.1  H 645.7  J 716.1  K 794.3  L 881.0  M 977.2  P 1083.9  Q 1202.3
 *     R 1333.5  S 1479.1
 *   MI_SELCAL_32, those sixteen and the sixteen that sit between them and above S, 32 tones in ascending frequency (A T B U C V ..):
 *     T 329.2  U 365.2  V 405.0  W 449.3  X 498.3  Y 552.7  Z 613.1  1 680.0  2 754.2  3 836.6  4 927.9  5 1029.2  6 1141.6  7 1266.2
 *     8 1404.4  9 1557.8
 *     These sixteen are written from memory of the extension: no document available when this was written could confirm them, and
 *     they have not been checked against a published table or an off-air call.  What is checked is that all 32 literals lie within
 *     0.15 Hz of 312.6 * 10^(0.0225 k), k = 0 .. 31 the position in ascending frequency (the classic tones are the even k); at
 *     analysis bins of 8 Hz an error of 0.1 Hz is harmless.
 *   MI_SELCAL_CUSTOM: cfg.ntones = 2 .. 32 frequencies cfg.freq[], strictly ascending, within 250 .. 2000 Hz, at least 16 Hz apart
 *     (NaN is refused); every letter is '?'.
 *
 * Stream model.  As for the voice band stage: a row's audio is one running sequence x over all batches of all calls the row was
 * enabled in; samples before the handle's first call are 0.
 * Windows are MI_SELCAL_WINDOW = 2000 samples at a hop of 1000: two per (row, batch), numbered per row from creation / set_state.
 * With b the call's batch and n0 the row's window counter when the call began, window n0 + 2b covers the last 1000 samples before
 * the batch and the batch's first 1000, window n0 + 2b + 1 the batch's samples 0 .. 1999.  The handle carries MI_SELCAL_HISTORY = 1002
 * samples per row, of which the two oldest are never read: the lead in front of a block (carry.hpp) is history + 2 floats and must be
 * whole float4.  The history length is ABI.
 * Per window, everything float32, every operation rounded on its own, no fused multiply-add:
 *   0. y[j] = x[j] * w[j], j = 0 .. 1999.  w (mi_selcal_window) is the 2000-point Hann window 0.5 - 0.5 cos(2 pi j / 1999), evaluated
 *      in float64 for j <= 999 and cast; w[1999 - j] = w[j], so that w is symmetric bit for bit.
 *   1. E, the window's energy: s_l = the sequential sum, j ascending over j = l (mod 64), of y[j] * y[j], starting from the first
 *      product, for l = 0 .. 63; then the butterfly s_l + s_{l+32} for l < 32, then + 16, 8, 4, 2, 1 in the same way; E is element 0.
 *      If E == 0.0f the window is SILENT: p[t] = +0.0f for every tone BY DEFINITION, and the recurrence of item 2 is not part of its
 *      definition.  Why: E == 0 says every product y[j] * y[j] rounded to zero, |y[j]| < 2^-75.  Where every y[j] is +-0 -- a closed
 *      batch, digital silence, -0.0f throughout -- the recurrence gives +0.0f everywhere anyway.  Where some are tiny but not zero it
 *      would give powers below 10^-36, which would carry no information and could never name a pair (min_energy > 0); fixing them at
 *      zero lets the device skip 2000 steps for every closed batch, and no byte depends on whether it did.
 *   2. For every tone t of the table: q1 = q2 = 0; for j = 0 .. 1999 in order: q0 = coeff[t] * q1 - q2 + y[j]; q2 = q1; q1 = q0 (a
 *      product, a subtraction, an addition).  p[t] = q1 * q1 + q2 * q2 - q1 * q2 * coeff[t], evaluated left to right:
 *      ((q1 * q1) + (q2 * q2)) - ((q1 * q2) * coeff[t]).
 *   3. best, second, third: the indices of the three largest p, in that order, a tie going to the lowest index (the first three of a
 *      stable descending sort).  A table of two tones has no third: third = MI_SELCAL_NONE8 and its power +0.0f.
 *   4. The window NAMES the pair {best, second} iff all four hold, and names no pair otherwise:
 *        E >= min_energy
 *        p[best] + p[second] >= tc * E              tc = min_tonality * c, one float32 product made on the host
 *        p[best] <= max_twist * p[second]
 *        p[second] >= min_separation * p[third]
 *      c = (float)((sum w)^2 / (2 sum w^2)), the sums in float64 over the float32 window: what two pure tones of equal level give
 *      for (p[best] + p[second]) / E, about N / 3 = 666.  The pair is stored lower index first, as lo | hi << 8; MI_SELCAL_NONE (0) = no pair.
 * The four thresholds are settings (mi_selcal_cfg, 0 = the default): min_energy 1e-3 (refused unless finite and 1e-12 ..
 * 1e6), min_tonality 0.5 (0.01 .. 1), max_twist 8.0 (1 .. 1000), min_separation 4.0 (1 .. 1000).  They are a caller's settings,
 * not tolerances, fixed from tools/selcal_classes.py and tried on synthetic signals only: no off-air SELCAL call
 * has been through this stage.
 *
 * Decoder.  Per row, sequentially over the row's windows in order, its state carried in the handle.  Settings in windows: min_run
 * (default 8, 2 .. 64), max_run (default 22, min_run .. 1024), max_gap (default 8, 1 .. 64).  "A pair" is what item 4 named.
 *   state    window seen                        action
 *   IDLE     a pair P                           -> FIRST with P, run1 = 1, first_window = this window
 *   IDLE     no pair                            stay
 *   FIRST    the same pair                      run1++; if run1 > max_run the pulse is overlong: -> OVER
 *   FIRST    another pair Q, run1 >= min_run    -> SECOND with Q, run2 = 1, gap = 0
 *   FIRST    another pair Q, run1 < min_run     restart FIRST with Q (run1 = 1, first_window = this window)
 *   FIRST    no pair, run1 >= min_run           -> GAP, gap = 1
 *   FIRST    no pair, run1 < min_run            -> IDLE
 *   OVER     the same pair                      stay
 *   OVER     anything else                      handle the window as from IDLE
 *   GAP      no pair                            gap++; if gap > max_gap -> IDLE
 *   GAP      the first pair again               a dropout: -> FIRST with run1 += gap + 1 (then overlong as above if run1 > max_run)
 *   GAP      another pair Q                     -> SECOND with Q, run2 = 1 (gap stays)
 *   SECOND   the same pair                      run2++; when run2 == min_run emit one code record, then -> DONE
 *   SECOND   anything else                      handle the window as from IDLE
 *   DONE     the second pair                    stay
 *   DONE     anything else                      handle the window as from IDLE
 * Decided where the table of the stage's specification left a choice, with tests/selcal_model.py the tie-breaker: an overlong
 * pulse is a state of its own (OVER), and the window that ends it is handled as from IDLE, so a pair that follows it directly begins a
 * new FIRST; a dropout that makes run1 exceed max_run is overlong too; min_run >= 2, so that SECOND never emits on entry; a dropout
 * inside the second pulse before the code is emitted loses the call (SECOND has no GAP); "the same pair" compares both indices.
 * A code record holds row, seq (the row's code number since creation / set_state), the four tone indices -- first pulse lower,
 * higher, second pulse lower, higher --, first_window and last_window (the row's numbers of the first window of the first pulse
 * and of the emitting window), run1 and gap as they stood, and batch, the call-relative batch of the emitting window.  With both
 * pulses clean the emitting window is the min_run-th of the second pulse.  Window numbers and seq wrap at 2^32.
 * State: per row MI_SELCAL_STATE_ROW_BYTES bytes, little-endian: float32 x[1002], the last 1002 input samples of the last batch of
 * the last call the row was enabled in, oldest first, zeros at first; then uint32 window (windows seen), seq (codes emitted), phase
 * (MI_SELCAL_IDLE ..), pair1, pair2 (lo | hi << 8, MI_SELCAL_NONE where the phase has none), run1, run2, gap, first_window, zero.
 * A disabled row writes nothing and every byte of its state stays.  NaN and Inf are unspecified, as everywhere behind the
 * demodulator.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned buffers, nbatches
 * outside 1 .. max_batches. */
enum { MI_SELCAL_16 = 0, MI_SELCAL_32 = 1, MI_SELCAL_CUSTOM = 2 };
enum { MI_SELCAL_WINDOW = 2000, MI_SELCAL_HOP = 1000, MI_SELCAL_HISTORY = 1002, MI_SELCAL_MAX_TONES = 32, MI_SELCAL_STATE_ROW_BYTES = 4048,
       MI_SELCAL_NONE8 = 0xFF };
enum { MI_SELCAL_IDLE = 0, MI_SELCAL_FIRST = 1, MI_SELCAL_OVER = 2, MI_SELCAL_GAP = 3, MI_SELCAL_SECOND = 4, MI_SELCAL_DONE = 5 };
#define MI_SELCAL_NONE 0u /* no pair: a pair has hi >= 1 and so is never 0; a blob of zeros is a fresh state */
typedef struct {
    uint32_t mode;                  /* MI_SELCAL_16 / _32 / _CUSTOM */
    uint32_t ntones;                /* MI_SELCAL_CUSTOM: 2 .. 32; otherwise ignored */
    float freq[32];                 /* MI_SELCAL_CUSTOM: Hz, ascending; otherwise ignored */
    float min_energy, min_tonality, max_twist, min_separation; /* 0 = the default */
    uint32_t min_run, max_run, max_gap;                        /* windows; 0 = the default */
    uint32_t zero;
} mi_selcal_cfg;                    /* 168 bytes */
typedef struct {
    uint8_t best, second, third, zero; /* indices into the tone table; third = MI_SELCAL_NONE8 in a table of two */
    float p_best, p_second, p_third;
    float energy;                   /* E */
    uint32_t pair;                  /* lo | hi << 8, or MI_SELCAL_NONE */
} mi_selcal_window_record;          /* 24 bytes */
typedef struct {
    uint32_t row, seq;              /* seq: the row's code number since creation / set_state, 0-based */
    uint8_t tone[4];                /* first pulse lower, higher; second pulse lower, higher */
    uint32_t first_window, last_window; /* the row's window numbers: first of the first pulse, the emitting one */
    uint32_t run1, gap;             /* windows of the first pulse (dropouts counted in), windows without a pair between the pulses */
    uint32_t batch;                 /* call-relative batch of the emitting window */
} mi_selcal_code;                   /* 32 bytes */
typedef struct mi_selcal mi_selcal;

/* cfg NULL = MI_SELCAL_16 with every default.  row_enabled [rows] as for mi_tones_create; rows and max_batches within the gate's
 * limits (1 <= rows < 2^20, rows * max_batches < 2^24).  max_codes: capacity of the caller's code buffer, 0 = rows * the most codes
 * a row can emit in max_batches batches, 1 + (2 * max_batches - 1) / (2 * min_run).  The handle owns the scratch for a call's
 * window decisions and codes. */
int mi_selcal_create(const mi_selcal_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_codes, int gpu, mi_selcal** out);
void mi_selcal_destroy(mi_selcal* s);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_selcal_set_rows(mi_selcal* s, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the plane d_plane [rows][row_stride]: 16-byte aligned, the stride a multiple
 * of 4 floats and at least nbatches * 2000.  Outputs in device memory:
 *   d_windows         [rows][2 * nbatches]  window records, window 2b and 2b + 1 of batch b, or NULL (not wanted); 8-byte aligned.
 *                                           A disabled row's are not written.
 *   d_codes           [max_codes]           rows ascending, seq ascending within a row (8-byte aligned)
 *   d_row_first_code  [rows + 1]            exclusive prefix of the rows' code counts
 *   d_count           [2]                   number of codes, and min(that, max_codes) = the number stored
 * Nothing is written at or beyond max_codes.  Asynchronous on `hip_stream`, no host synchronisation; five kernels without atomics
 * -- bank (one wave per (row, batch): the two windows' records and decisions), walk (one lane per row: the decoder over the call's
 * decisions, its codes into the handle's scratch, the row's count and new decoder state), scan, store (the codes to their places),
 * tails (the enabled rows' last 1002 samples into the carried state) -- so every byte is the same on every run and equals
 * mi_selcal_plan_host's. */
int mi_selcal_process_device(mi_selcal* s, const float* d_plane, size_t row_stride, int nbatches, mi_selcal_window_record* d_windows,
                             mi_selcal_code* d_codes, uint32_t* d_row_first_code, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_selcal_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] codes (and the rows * 2 * nbatches window records, if the call had a d_windows and windows is not NULL;
 * with windows not NULL after a call without d_windows it is refused).  codes, windows and row_first_code may each be NULL.  The one
 * place that synchronises. */
int mi_selcal_download(mi_selcal* s, void* hip_stream, mi_selcal_code* codes, mi_selcal_window_record* windows, uint32_t* row_first_code,
                       uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_SELCAL_STATE_ROW_BYTES bytes in the layout above (mi_selcal_plan_host reads and writes the same
 * bytes).  set_state refuses an impossible decoder state: a phase beyond MI_SELCAL_DONE, a pair the phase needs that is not two
 * ascending indices into the table, a pair or counter the phase has none of that is not MI_SELCAL_NONE / 0, run1 outside 1 .. max_run
 * (OVER: max_run + 1), run2 outside 1 .. min_run - 1 (DONE: min_run), gap over max_gap, pair2 equal to pair1, zero not 0.  Both
 * complete queued work first. */
size_t mi_selcal_state_size(const mi_selcal* s);
int mi_selcal_get_state(mi_selcal* s, void* buf, size_t len);
int mi_selcal_set_state(mi_selcal* s, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[5] = {bank, walk, scan, store, tails}.  tools/selcal_rate.py. */
int mi_selcal_set_timing(mi_selcal* s, int on);
int mi_selcal_last_launch_ms(mi_selcal* s, float* ms /* [5] */);
/* The host twin: no GPU and no HIP call; the same windows, codes and state blob byte for byte.  plane [rows][row_stride] (no
 * alignment asked); state_inout rows * MI_SELCAL_STATE_ROW_BYTES bytes, read and updated; windows [rows][2 * nbatches] or NULL;
 * codes holds max_codes entries (max_codes >= 1), of which min(count[0], max_codes) = count[1] are written. */
int mi_selcal_plan_host(const mi_selcal_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                        void* state_inout, mi_selcal_window_record* windows, mi_selcal_code* codes, size_t max_codes, uint32_t* row_first_code,
                        uint32_t* count /* [2] */);
/* The tone table of cfg (NULL = MI_SELCAL_16; only mode, ntones and freq are read): *ntones, freq[t], coeff[t] and letter[t] for
 * t < *ntones.  Each output may be NULL.  Refuses what mi_selcal_create would refuse of the table. */
int mi_selcal_table(const mi_selcal_cfg* cfg, uint32_t* ntones, float* freq /* [32] */, float* coeff /* [32] */, char* letter /* [32] */);
/* The settings of cfg (NULL = all defaults) with every default filled in, or the refusal mi_selcal_create would give; *c = the
 * constant of item 4 (may be NULL). */
int mi_selcal_settings(const mi_selcal_cfg* cfg, mi_selcal_cfg* out, float* c);
/* The 2000 window coefficients.  Host only. */
int mi_selcal_window(float* out /* [MI_SELCAL_WINDOW] */);
/* "AB-CD" from a code record's four tone indices under `mode`'s letters ("??-??" under MI_SELCAL_CUSTOM), NUL-terminated.  Refuses
 * an unknown mode and an index beyond the mode's table (32 under MI_SELCAL_CUSTOM). */
int mi_selcal_code_text(uint32_t mode, const uint8_t* tones /* [4] */, char* out /* [6] */);

/* ---------------- ACARS decoder stage: MSK frames per row, on the device ----------------
 * ACARS runs on plain AM airband channels at 2400 bit/s as MSK in the audio: a bit that differs from the previous one is half a
 * cycle of 1200 Hz, a bit that repeats it a full cycle of 2400 Hz, the tones locked in phase to the bit clock.  The reference leaves
 * the bursts in the recording.  This stage reads a plane [rows][row_stride] of float32 audio as mi_selcal_* does, needs no flags, and
 * writes one record per received block (a FRAME here).  Coherent detection bit by bit: it rests on that phase lock, keeps no phase
 * memory from bit to bit, and so gives away part of what a full MSK receiver has (DESIGN.md 5o has the measured sensitivity).
 * NOT CHECKED: no off-air ACARS has been through the stage.  The framing constants, the parity convention, the checksum's coverage
 * and the phase lock are written from memory of the air format and pinned only to the modulator of tests/acars_model.py.  No error
 * correction, no reassembly of multi-block messages, no decoding of labels.
 *
 * Stream model.  As for the SELCAL stage: a row's audio is one running sequence over all batches of all calls the row was enabled
 * in; samples before the handle's first call are 0.
 * Timing grid.  16000 / 2400 = 20 / 3 samples a bit, so time is counted in THIRDS of a sample; sample n sits at third 3 n.  Under
 * hypothesis tau = 0 .. 19, bit k covers the thirds [tau + 20 k, tau + 20 k + 20), k counted from the row's first sample, and sample n
 * contributes to it when rho = 3 n - (tau + 20 k) lies in 0 .. 19: seven samples where the first rho is 0 or 1, else six.  tau + 20 is
 * tau one bit later, exactly.  A batch is 6000 thirds; the bits of a (row, batch) are those whose last sample lies in the batch,
 * exactly 300 per hypothesis.  They are numbered by SLOT j = 0 .. 299: slot j of hypothesis tau is the bit that begins at third
 * tau + 20 (j - [tau > 0]) of the batch, so slot 0 of tau >= 1 begins at third tau - 20, before the batch.  The earliest sample any
 * bit of a batch reads is the sixth before it (tau = 1 .. 2), so the handle carries MI_ACARS_HISTORY = 6 samples per row: the
 * smallest H for which the lead H + 2 (carry.hpp) is whole float4.  In one slot, hypothesis tau begins a third after tau - 1 for
 * tau = 2 .. 19, and 0 a third after 19; hypothesis 1 begins a third after hypothesis 0 OF THE SLOT BEFORE.
 * Bit bank, per (row, batch, tau, slot); float32, every operation rounded on its own, no fused multiply-add.  Templates
 * (mi_acars_templates) h1[rho] = (float)sin(pi rho / 20), h2[rho] = (float)sin(2 pi rho / 20), rho = 0 .. 19, evaluated in double and
 * rounded once.  r1 = sum x[n] * h1[rho], r2 = sum x[n] * h2[rho] over the bit's samples in ascending n, each sum beginning with its
 * first product.  CHANGE bit c = 1 if |r1| >= |r2| (1200 Hz: the bit differs from the one before), else 0; quality q = max(r1 * r1,
 * r2 * r2).  Q[tau] of the block: s_l = the sequential sum over the slots j = l (mod 64) in ascending j of q, beginning with the
 * first, l = 0 .. 63; then s_l + s_{l + 32} for l < 32, then + 16, 8, 4, 2, 1 in the same way; Q is element 0 (the order of the SELCAL
 * stage's energy).  Packed: 10 words per (row, batch, tau), slot j in bit j % 32 of word j / 32, the upper 20 bits of word 9 zero.
 * A block whose 2000 samples and 6 carried samples are all +-0 gives c = 1 and Q = +0.0f everywhere (|0| >= |0|); the device writes
 * that without the sums.
 * Sync.  Characters are 7 bits and odd parity in bit 7, sent least significant bit first.  The pattern is the 39 change bits inside the
 * 40 bits of '+' '*' SYN SYN SOH (0xAB 0x2A 0x16 0x16 0x01 with parity); only changes are matched, so polarity never enters.  Every
 * hypothesis keeps its last 39 change bits.  While a row is IDLE, at every slot in order, a hypothesis HITS when its 39 bits differ
 * from the pattern in at most sync_errors places and Q[tau] of the slot's batch >= min_quality.  The first slot with a hit opens a
 * frame on the hitting hypothesis with the fewest mismatches, then the largest Q of that batch, then the lowest tau.  The bit
 * before the frame's first is SOH's last, 0: b_k = b_{k-1} xor c_k from there.  One frame at a time per row; hits inside a frame
 * are ignored.
 * Walker.  From the slot after the hit, the chosen hypothesis u's bits, 8 to a byte, least significant first: Mode, Address[7], Ack,
 * Label[2], Block id (12 bytes), then bytes up to and including the first whose low 7 bits are ETX (0x03) or ETB (0x17), then the
 * two bytes of the BCS.  The BCS is CRC-16/KERMIT (reflected polynomial 0x8408, initial value 0, mi_acars_crc) over the raw bytes,
 * parity bits included, from Mode through ETX / ETB, sent low byte first: the CRC over those bytes and the BCS is 0, which is
 * crc_ok.  parity_errors counts the bytes from Mode through ETX / ETB with an even number of ones.  When byte MI_ACARS_MAX_BYTES =
 * 240 behind SOH arrives and neither it nor one before it (from the 13th on) was ETX / ETB, the frame is dropped without a record
 * and the row goes idle.  A finished frame is a record if crc_ok or the setting keep_bad is 1; the row goes idle either way.
 * Timing moves.  At the first slot of every batch that begins inside a frame (unless hold_timing is 1), with Q of the new batch:
 * v = u; if Q[u - 1] > Q[v] then v = u - 1; if Q[u + 1] > Q[v] then v = u + 1 (indices mod 20; a tie keeps u, a tie between the
 * neighbours that beats u goes to u - 1); u = v, one third earlier or later.  By the grid's identity the walker stays in step except
 * between 0 and 1: moving 0 -> 1 it passes over slot 0 of the new batch (hypothesis 1's slot 1 is the bit a third later), moving
 * 1 -> 0 it first takes hypothesis 0's last bit of the batch before, out of the carried 38, then slot 0.
 * Settings (mi_acars_cfg, 0 = the default): sync_errors 1 .. 4, default 2, MI_ACARS_SYNC_EXACT for none (0 is taken by "the
 * default"); keep_bad 0 / 1; min_quality finite and >= 0, default 0 (no floor was justified by the measurement);
 * hold_timing 0 / 1 (a diagnostic: tools/acars_classes.py measures what the moves buy).
 * Record: row; batch and third, where the first bit behind SOH begins (the row's batch number since creation / set_state, wrapping
 * at 2^32, and the third within it, 0 .. 5999); tau_sync and tau_end, u at the hit and at the end; sync_errors, the hit's
 * mismatches; crc_ok; nbytes, Mode through ETX / ETB; parity_errors; end, 0x03 or 0x17; end_batch, the call's batch in which the
 * frame ended; bytes, the nbytes raw bytes and the two of the BCS behind them, zeros to the end.
 * State: per row MI_ACARS_STATE_ROW_BYTES = 496 bytes, little-endian, a blob of zeros being a fresh state: float32 x[6], the last 6
 * input samples, oldest first; uint32 batch (batches seen), phase (MI_ACARS_IDLE / MI_ACARS_FRAME); uint64 hist[20], per hypothesis
 * the last 38 change bits, the newest in bit 0; then uint32 u, prev (the last bit's value), nbits and cur (the bits of the running
 * byte), nbytes, tail (0 up to ETX / ETB; behind it 1 + the BCS bytes taken), crc (running), parity_errors, start_batch, start_third,
 * tau_sync, mismatches, end, zero; then bytes[248] as the record has them so far.  An idle row's fields from u on are all zero.
 * A disabled row writes nothing and every byte of its state stays.  NaN and Inf are unspecified.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned buffers, nbatches
 * outside 1 .. max_batches. */
enum { MI_ACARS_HISTORY = 6, MI_ACARS_HYPOTHESES = 20, MI_ACARS_BITS = 300, MI_ACARS_BIT_WORDS = 10, MI_ACARS_SYNC_BITS = 39, MI_ACARS_HEAD_BYTES = 12,
       MI_ACARS_MAX_BYTES = 240, MI_ACARS_RAW_BYTES = 248, MI_ACARS_STATE_ROW_BYTES = 496 };
enum { MI_ACARS_IDLE = 0, MI_ACARS_FRAME = 1 };
#define MI_ACARS_SYNC_EXACT 0x80000000u /* sync_errors: no mismatch allowed */
typedef struct {
    uint32_t sync_errors;           /* 0 = 2; 1 .. 4; MI_ACARS_SYNC_EXACT */
    uint32_t keep_bad;              /* 1: frames whose checksum fails are records too */
    float min_quality;              /* floor on Q[tau] of the batch of a sync hit */
    uint32_t hold_timing;           /* 1: no timing moves */
} mi_acars_cfg;                     /* 16 bytes */
typedef struct {
    uint32_t row;
    uint32_t batch, third;          /* where the first bit behind SOH begins */
    uint8_t tau_sync, tau_end, sync_errors, crc_ok;
    uint16_t nbytes;                /* Mode through ETX / ETB, 13 .. 240 */
    uint8_t parity_errors;
    uint8_t end;                    /* 0x03 (ETX) or 0x17 (ETB) */
    uint32_t end_batch;             /* call-relative */
    uint8_t bytes[248];             /* raw: nbytes, then the BCS low, high; then zeros */
} mi_acars_frame;                   /* 272 bytes */
typedef struct {                    /* the printable fields of a frame, parity stripped, NUL-terminated; a character outside 0x20 .. 0x7E is '.' */
    char mode[2], address[8], ack[2], label[3], block_id[2], text[231];
} mi_acars_text;                    /* 248 bytes */
typedef struct mi_acars mi_acars;

/* cfg NULL = every default.  row_enabled, rows and max_batches as for mi_selcal_create.  max_frames: capacity of the caller's frame
 * buffer, 0 = rows * the most frames a row can end in max_batches batches, 1 + 300 * max_batches / 119.  The handle owns the scratch
 * for a call's change bits, Q and frames. */
int mi_acars_create(const mi_acars_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_frames, int gpu, mi_acars** out);
void mi_acars_destroy(mi_acars* s);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_acars_set_rows(mi_acars* s, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the plane d_plane [rows][row_stride]: 16-byte aligned, the stride a multiple
 * of 4 floats and at least nbatches * 2000.  Outputs in device memory:
 *   d_bits             [rows][nbatches][20][10]  the packed change bits, or NULL (the handle's scratch); 4-byte aligned.
 *   d_q                [rows][nbatches][20]      Q, or NULL (the handle's scratch).  A disabled row's are not written.
 *   d_frames           [max_frames]              rows ascending, time order within a row (8-byte aligned)
 *   d_row_first_frame  [rows + 1]                exclusive prefix of the rows' frame counts
 *   d_count            [2]                       number of frames, and min(that, max_frames) = the number stored
 * Nothing is written at or beyond max_frames.  Asynchronous on `hip_stream`, no host synchronisation; five kernels without atomics
 * -- bits (one workgroup per (row, batch)), walk (one wave per row, a lane per hypothesis), scan, store, tails -- so every byte is
 * the same on every run and equals mi_acars_plan_host's. */
int mi_acars_process_device(mi_acars* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, float* d_q, mi_acars_frame* d_frames,
                            uint32_t* d_row_first_frame, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_acars_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] frames.  frames and row_first_frame may each be NULL.  The one place that synchronises. */
int mi_acars_download(mi_acars* s, void* hip_stream, mi_acars_frame* frames, uint32_t* row_first_frame, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_ACARS_STATE_ROW_BYTES bytes in the layout above (mi_acars_plan_host reads and writes the same
 * bytes).  set_state refuses an impossible state: history bits beyond the 38, an unknown phase, an idle row with a walker field or
 * byte set, and inside a frame u or tau_sync beyond 19, prev beyond 1, nbits beyond 7, cur beyond its nbits bits, tail beyond 2,
 * nbytes the frame cannot have (beyond 239 before ETX / ETB, under 13 behind it), an end that is not the byte it names, mismatches
 * beyond 4, start_third beyond 5999, a crc or parity_errors that the bytes do not give, a byte set behind the ones taken, zero
 * not 0.  Both complete queued work first. */
size_t mi_acars_state_size(const mi_acars* s);
int mi_acars_get_state(mi_acars* s, void* buf, size_t len);
int mi_acars_set_state(mi_acars* s, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[5] = {bits, walk, scan, store, tails}.  tools/acars_rate.py. */
int mi_acars_set_timing(mi_acars* s, int on);
int mi_acars_last_launch_ms(mi_acars* s, float* ms /* [5] */);
/* The host twin: no GPU and no HIP call; the same bits, Q, frames and state blob byte for byte.  plane [rows][row_stride] (no
 * alignment asked); state_inout rows * MI_ACARS_STATE_ROW_BYTES bytes, read and updated; bits [rows][nbatches][20][10] and
 * q [rows][nbatches][20], each or NULL; frames holds max_frames entries (max_frames >= 1), of which min(count[0], max_frames) =
 * count[1] are written. */
int mi_acars_plan_host(const mi_acars_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                       void* state_inout, uint32_t* bits, float* q, mi_acars_frame* frames, size_t max_frames, uint32_t* row_first_frame,
                       uint32_t* count /* [2] */);
/* The settings of cfg (NULL = all defaults) with every default filled in, or the refusal mi_acars_create would give. */
int mi_acars_settings(const mi_acars_cfg* cfg, mi_acars_cfg* out);
/* The two templates.  Host only. */
int mi_acars_templates(float* h1 /* [20] */, float* h2 /* [20] */);
/* CRC-16/KERMIT of n bytes (NULL with n = 0 is fine; NULL otherwise gives 0xFFFFFFFF, which no CRC is). */
uint32_t mi_acars_crc(const uint8_t* bytes, size_t n);
/* The printable fields of a record.  Refuses an nbytes outside 13 .. 240. */
int mi_acars_frame_text(const mi_acars_frame* f, mi_acars_text* out);

/* ---------------- SAME decoder stage: weather-alert headers per row, on the device ----------------
 * On NFM weather-radio channels an alert is announced in the audio by SAME (Specific Area Message Encoding) bursts: 520.83 bit/s AFSK,
 * a preamble of 0xAB bytes, then "ZCZC-ORG-EEE-PSSCCC(-PSSCCC..)+TTTT-JJJHHMM-LLLLLLLL-", sent three times about a second apart; behind
 * the voice message "NNNN" is sent three times.  This stage reads a plane [rows][row_stride] of float32 audio as mi_acars_* does,
 * needs no flags, and writes one record per received MESSAGE (up to three bursts of one kind, voted).
 * NOT CHECKED: no off-air SAME has been through the stage.  The format is restated from memory of 47 CFR 11.31 and pinned only to the
 * modulator of tests/same_model.py.  The 1050 Hz warning tone is mi_aspec_*'s to find; no event-code dictionary.
 *
 * Stream model.  As for the ACARS stage: a row's audio is one running sequence over all batches of all calls the row was enabled in;
 * samples before the handle's first call are 0.
 * Tones.  A bit lasts 16000 * 6 / 3125 = 30.72 samples; mark (1) is 4 cycles per bit (2083.3 Hz), space (0) 3 cycles (1562.5 Hz).
 * Bytes go least significant bit first, 8 bits, bit 7 zero, no parity.
 * Timing grid.  Time is counted in UNITS of 1/25 sample: sample n sits at unit 25 n, a bit is 768 units, a batch 50 000.  Hypotheses
 * tau = 0 .. 15 lie 48 units apart: bit k of tau covers the units [48 tau + 768 k, + 768), k counted from the row's first sample, and
 * tau + 16 is tau one bit later exactly.  50 000 = 65 * 768 + 80, so the grid moves 80 units a batch against the batch edge and
 * repeats every 48 batches; the state carries grid = (50 000 * batches seen) mod 768 itself (a multiple of 16), so a wrapping batch
 * counter changes nothing.  The bits of a (row, batch) are those whose last sample lies in the batch: with c = (48 tau - grid) mod 768
 * the first begins at unit r0 = c - 768 of the batch (r0 = 0 where c = 0), the others 768 apart up to unit 49 232: 65 or 66 per
 * hypothesis, bit j beginning at r = r0 + 768 j.  The earliest sample a batch's bits read is the 30th before it: MI_SAME_HISTORY = 30
 * carried samples per row, a lead of 32 (carry.hpp).
 * Bit bank, per (row, batch, tau, j); float32, every operation rounded on its own, no fused multiply-add.  Templates
 * (mi_same_templates) of 768 entries each, evaluated in double and rounded once: T0 = cos, T1 = sin of 2 pi 4 rho / 768, T2 = cos,
 * T3 = sin of 2 pi 3 rho / 768.  A bit's samples are n = ceil(r / 25) .. floor((r + 767) / 25), 30 or 31 of them, rho = 25 n - r;
 * the four sums S0 .. S3 of x[n] * T[rho] run in ascending n, each beginning with its first product.  Pm = S0 * S0 + S1 * S1,
 * Ps = S2 * S2 + S3 * S3; the bit is 1 if Pm >= space_gain * Ps; q = max(Pm, Ps).  Q[tau] of the block in the ACARS stage's order:
 * s_l = q_l (+ q_{l + 64} where there is one), l = 0 .. 63; then s_l + s_{l + 32} for l < 32, then + 16, 8, 4, 2, 1; Q is element 0.
 * Packed: 4 words per (row, batch, tau): bit j in bit j % 32 of word j / 32, the bits of word 2 from the count on zero, and the
 * count (65 or 66) in word 3.  A block whose 2000 samples and 30 carried samples are all +-0 holds every bit 1 (0 >= space_gain * 0),
 * its counts, and Q = +0.0f everywhere; the device writes that without the sums.
 * Sync.  Every hypothesis keeps its last 64 bits, the newest in bit 0 (zeros before the row's first bit).  The patterns are the 64
 * bits of AB AB AB AB 'Z' 'C' 'Z' 'C' (MI_SAME_HEADER) and of AB AB AB AB 'N' 'N' 'N' 'N' (MI_SAME_EOM); they differ in 10 places, so
 * with at most 4 mismatches allowed a history hits at most one.  Decisions are taken per bit index k in ascending order over the 16
 * bits (tau, k).  BOOKKEEPING AT A BATCH EDGE: the bits (tau, k) of one k begin 48 units apart, so a batch edge cuts one k in two:
 * the hypotheses tau <= grid / 48 (grid of the later batch; none where grid >= 720) have their bit in the earlier batch.  That k is
 * decided in the LATER batch: the earlier batch shifts those hypotheses' bit into their histories, where it waits, and decides
 * cnt(15) indices; Q in every decision is Q of the batch that decides.  An IDLE row that is not deaf opens a burst at the first k
 * where a hypothesis differs from a pattern in at most sync_errors places and Q[tau] >= min_quality; among the hitting hypotheses the
 * fewest mismatches, then the largest Q, then the lowest tau.  A row is DEAF for the 64 indices behind a burst's end: the next sync
 * has to arrive whole behind the burst.
 * Burst.  The record's bytes begin with the pattern's own "ZCZC" / "NNNN".  An NNNN burst ends at once.  Behind ZCZC the chosen
 * hypothesis u's bits are read 8 to a byte from index k + 1 on.  The burst ends with the third '-' behind the first '+'; as TRUNCATED
 * at MI_SAME_MAX_BYTES = 268 bytes counted from 'Z'; and as truncated at the max_bad-th consecutive byte with bit 7 set or under
 * 0x20, those max_bad bytes being dropped.  Timing moves by the ACARS rule at the first index of every batch that begins inside a
 * burst (unless hold_timing): v = u; if Q[u - 1] > Q[v] then v = u - 1; if Q[u + 1] > Q[v] then v = u + 1 (indices mod 16); u = v.
 * Moving 15 -> 0 the walker passes over the batch's first index; moving 0 -> 15 it first takes hypothesis 15's newest carried bit.
 * Message.  A row's assembler keeps the ended bursts of one kind.  The third burst closes the message: nbytes is the median of the
 * three lengths (the length two of them share, where two do), every byte the bitwise two-of-three majority of the bursts' bytes,
 * a burst shorter than the place counting as zeros there, truncated the majority of the three flags, voted = 1.  A message also
 * closes when a burst of the other kind opens, and at the first index of the gap_batches-th batch that begins since the last burst
 * ended with the row outside a burst: then it is the FIRST burst, voted = 0, nbursts 1 or 2.  agree counts the places below nbytes at
 * which all nbursts bursts hold the same byte.  fields_ok: an EOM is "NNNN"; a header matches the grammar above with ORG and EEE
 * three capitals, 1 to 31 locations of six digits, TTTT four digits, JJJHHMM seven digits and a station of eight printable characters
 * other than '-'.  batch / unit: where the first burst's 'Z' or 'N' begins (the row's batch number since creation / set_state,
 * wrapping at 2^32, and the unit within it); end_batch: the call's batch that closed the message.
 * The most messages a row closes in a call of n batches: every close but those of the gap rule belongs to one burst, bursts open at
 * least 65 indices apart, a batch decides at most 66 indices, so at most B = 2 + 66 n / 65 bursts touch the call and each refills the
 * assembler once for the gap rule: 2 B + 1 = MI_SAME_MAX_MESSAGES(n).
 * Settings (mi_same_cfg, 0 = the default): sync_errors 1 .. 4, default 4, MI_SAME_SYNC_EXACT for none; max_bad 1 .. 16, default 4;
 * gap_batches 1 .. 1000, default 20 (2.5 s); min_quality finite and >= 0, default 0; space_gain finite and > 0, default 1 (DESIGN.md
 * 5p: the de-emphasis tilt measured behind the demodulator asks for no other); hold_timing 0 / 1.
 * State: per row MI_SAME_STATE_ROW_BYTES = 1160 bytes, little-endian, a blob of zeros being a fresh state: float32 x[30]; uint32 batch,
 * grid; uint64 hist[16]; uint32 phase (MI_SAME_IDLE / MI_SAME_BURST), u, kind, nbits, cur, nbytes, nbad, plus, dashes, deaf,
 * start_batch, start_unit (the burst's); an, akind, alen[2], atrunc[2], aidle, astart_batch, astart_unit (the assembler's), zero;
 * then bytes[3][272]: the running burst and the assembler's two stored ones, zeros behind their lengths.
 * A disabled row writes nothing and every byte of its state stays.  NaN and Inf are unspecified.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned buffers, nbatches
 * outside 1 .. max_batches. */
enum { MI_SAME_HISTORY = 30, MI_SAME_HYPOTHESES = 16, MI_SAME_BIT_UNITS = 768, MI_SAME_BATCH_UNITS = 50000, MI_SAME_BIT_WORDS = 4, MI_SAME_MAX_BITS = 66,
       MI_SAME_SYNC_BITS = 64, MI_SAME_MAX_BYTES = 268, MI_SAME_RAW_BYTES = 272, MI_SAME_DEAF = 64, MI_SAME_STATE_ROW_BYTES = 1160 };
enum { MI_SAME_IDLE = 0, MI_SAME_BURST = 1 };
enum { MI_SAME_HEADER = 0, MI_SAME_EOM = 1 };
#define MI_SAME_SYNC_EXACT 0x80000000u /* sync_errors: no mismatch allowed */
#define MI_SAME_MAX_MESSAGES(nbatches) (2u * (2u + 66u * (nbatches) / 65u) + 1u)
typedef struct {
    uint32_t sync_errors;           /* 0 = 4; 1 .. 4; MI_SAME_SYNC_EXACT */
    uint32_t max_bad;               /* 0 = 4; 1 .. 16 */
    uint32_t gap_batches;           /* 0 = 20; 1 .. 1000 */
    float min_quality;              /* floor on Q[tau] of the batch that decides a sync hit */
    float space_gain;               /* 0 = 1 */
    uint32_t hold_timing;           /* 1: no timing moves */
} mi_same_cfg;                      /* 24 bytes */
typedef struct {
    uint32_t row;
    uint32_t kind;                  /* MI_SAME_HEADER / MI_SAME_EOM */
    uint32_t batch, unit;           /* where the first burst's 'Z' / 'N' begins */
    uint32_t end_batch;             /* call-relative */
    uint8_t nbursts, voted, truncated, fields_ok;
    uint16_t nbytes, agree;
    uint32_t zero;
    uint8_t bytes[272];             /* nbytes from 'Z' / 'N' on, then zeros */
} mi_same_message;                  /* 304 bytes */
typedef struct {                    /* a header's fields, NUL-terminated */
    char originator[4], event[4], purge[5], issue[8], station[9], pad[2];
    uint32_t nlocations;
    char locations[31][7];
    char pad2[3];
} mi_same_text;                     /* 256 bytes */
typedef struct mi_same mi_same;

/* cfg NULL = every default.  row_enabled, rows and max_batches as for mi_acars_create.  max_messages: capacity of the caller's
 * message buffer, 0 = rows * MI_SAME_MAX_MESSAGES(max_batches).  The handle owns the scratch for a call's bits, Q and messages; the
 * messages' part is sized by the bound whatever max_messages says, rows * MI_SAME_MAX_MESSAGES(max_batches) * 304 bytes -- 23 MB at
 * 2048 rows x 16 batches, 600 bytes per (row, batch) in the limit, so gigabytes near rows * max_batches = 2^24 -- though audio closes
 * a message every few seconds at most: size max_batches by the calls made, not by the longest imaginable. */
int mi_same_create(const mi_same_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_messages, int gpu, mi_same** out);
void mi_same_destroy(mi_same* s);
int mi_same_set_rows(mi_same* s, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the plane d_plane [rows][row_stride]: 16-byte aligned, the stride a multiple
 * of 4 floats and at least nbatches * 2000.  Outputs in device memory:
 *   d_bits               [rows][nbatches][16][4]  the packed bits and counts, or NULL (the handle's scratch); 4-byte aligned.
 *   d_q                  [rows][nbatches][16]     Q, or NULL (the handle's scratch).  A disabled row's are not written.
 *   d_messages           [max_messages]           rows ascending, time order within a row (8-byte aligned)
 *   d_row_first_message  [rows + 1]               exclusive prefix of the rows' message counts
 *   d_count              [2]                      number of messages, and min(that, max_messages) = the number stored
 * Nothing is written at or beyond max_messages.  Asynchronous on `hip_stream`, no host synchronisation; five kernels without atomics
 * -- bits (one workgroup per (row, batch)), walk (one wave per row, a lane per hypothesis), scan, store, tails -- so every byte is
 * the same on every run and equals mi_same_plan_host's. */
int mi_same_process_device(mi_same* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, float* d_q, mi_same_message* d_messages,
                           uint32_t* d_row_first_message, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_same_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] messages.  messages and row_first_message may each be NULL.  The one place that synchronises. */
int mi_same_download(mi_same* s, void* hip_stream, mi_same_message* messages, uint32_t* row_first_message, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_SAME_STATE_ROW_BYTES bytes in the layout above (mi_same_plan_host reads and writes the same bytes).
 * set_state refuses an impossible state: zero not 0; a grid that is no multiple of 16 below 768; an unknown phase; an idle row with a
 * burst field or a byte of the running burst set, or deaf beyond 64; inside a burst a kind other than MI_SAME_HEADER, u beyond 15,
 * nbits beyond 7, cur beyond its nbits bits, nbytes outside 4 .. 267, bytes that do not begin with "ZCZC", nbad / plus / dashes that
 * the bytes do not give or that would have ended the burst, deaf not 0, start_unit beyond 49 999, an assembler of the other kind;
 * an assembler with more than 2 bursts, an unknown kind, a length outside 4 .. 268 (an EOM's: not 4), a flag beyond 1, aidle at or
 * beyond gap_batches, astart_unit beyond 49 999, a field or byte set that its bursts do not use; a byte set behind a burst's length.
 * Both complete queued work first. */
size_t mi_same_state_size(const mi_same* s);
int mi_same_get_state(mi_same* s, void* buf, size_t len);
int mi_same_set_state(mi_same* s, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[5] = {bits, walk, scan, store, tails}.  tools/same_rate.py. */
int mi_same_set_timing(mi_same* s, int on);
int mi_same_last_launch_ms(mi_same* s, float* ms /* [5] */);
/* The host twin: no GPU and no HIP call; the same bits, Q, messages and state blob byte for byte.  plane [rows][row_stride] (no
 * alignment asked); state_inout rows * MI_SAME_STATE_ROW_BYTES bytes, read and updated; bits [rows][nbatches][16][4] and
 * q [rows][nbatches][16], each or NULL; messages holds max_messages entries (>= 1), of which min(count[0], max_messages) = count[1]
 * are written. */
int mi_same_plan_host(const mi_same_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                      void* state_inout, uint32_t* bits, float* q, mi_same_message* messages, size_t max_messages, uint32_t* row_first_message,
                      uint32_t* count /* [2] */);
/* The settings of cfg (NULL = all defaults) with every default filled in, or the refusal mi_same_create would give. */
int mi_same_settings(const mi_same_cfg* cfg, mi_same_cfg* out);
/* The four templates T0 .. T3.  Host only. */
int mi_same_templates(float* out /* [4][768] */);
/* A header record's fields.  Refuses a record that is no header with fields_ok. */
int mi_same_message_text(const mi_same_message* m, mi_same_text* out);

/* ---------------- ELT detector stage: swept-tone beacon alarms per row, on the device ----------------
 * The homing signal of a distress beacon (ELT / EPIRB / PLB) on 121.5 MHz is an AM carrier whose audio tone sweeps through at least
 * 700 Hz somewhere inside 300 .. 1600 Hz, normally downward, and repeats 2 to 4 times a second for minutes or hours.  The reference
 * leaves the wail in the recording; mi_tones_* and mi_selcal_* want steady tones and mi_aspec_* averages 125 ms, which smears a whole
 * sweep.  This stage answers "which row carries a beacon, and since when?": one ONSET record when a beacon starts, one END record
 * when it ends.  It reads a plane [rows][row_stride] of float32 audio as mi_selcal_* does and needs no flags.
 * NOT CHECKED: the signal description above is written from memory of the ELT specifications (TSO-C91a class); no document available
 * when this was written could confirm it, and no off-air beacon has been through the stage.  Everything is tried on synthetic
 * signals only (tests/elt_model.py, tools/elt_classes.py).
 *
 * Stream model.  As for the SELCAL stage: a row's audio is one running sequence x over all batches of all calls the row was enabled
 * in; samples before the handle's first call are 0.  A disabled row writes nothing and every byte of its state stays.  NaN and Inf
 * are unspecified, as everywhere behind the demodulator.
 * Frames are MI_ELT_FRAME = 256 samples at a hop of MI_ELT_HOP = 80: exactly 25 per (row, batch), numbered per row from creation /
 * set_state, modulo 2^32.  Frame g = 0 .. 24 of a batch covers the batch's samples 80 g - 176 .. 80 g + 79 (negative: the samples
 * before the batch).  The handle carries MI_ELT_HISTORY = 178 samples per row, of which the two oldest are never read: the lead in
 * front of a block (carry.hpp) is history + 2 = 180 floats and must be whole float4.  The history length is ABI.
 * Per frame, everything float32, every operation rounded on its own, no fused multiply-add:
 *   0. y[j] = x[j] * w[j], j = 0 .. 255.  w (mi_elt_window) is the 256-point Hann window 0.5 - 0.5 cos(2 pi j / 255), evaluated in
 *      float64 for j <= 127 and cast; w[255 - j] = w[j], so that w is symmetric bit for bit.
 *   1. E, the frame's energy: s_l = the sequential sum, j ascending over j = l (mod 64), of y[j] * y[j], starting from the first
 *      product, for l = 0 .. 63 (four terms each); then the butterfly s_l + s_{l+32} for l < 32, then + 16, 8, 4, 2, 1 in the same
 *      way; E is element 0.  If E == 0.0f the frame is SILENT: every power is +0.0f BY DEFINITION (so best = 2 and p3 = +0.0f) and
 *      the recurrence of item 2 is not part of its definition, for the reasons the SELCAL stage gives.
 *   2. A bank of 32 detectors on the exact bins k = 2 .. 33 of the 256-point transform (62.5 Hz apart, 125 .. 2062.5 Hz):
 *      coeff[k] = (float)(2 cos(2 pi k / 256)) (mi_elt_coeffs).  q1 = q2 = 0; for j = 0 .. 255 in order: q0 = coeff * q1 - q2 + y[j];
 *      q2 = q1; q1 = q0 (a product, a subtraction, an addition).  p[k] = ((q1 * q1) + (q2 * q2)) - ((q1 * q2) * coeff).
 *   3. best = the bin of the largest p, a tie going to the lowest bin.  p3 = (p[best - 1] + p[best]) + p[best + 1], a neighbour
 *      outside 2 .. 33 counting as +0.0f.
 *   4. The frame is TONAL with bin `best` iff all three hold, and has no bin (MI_ELT_NONE8) otherwise:
 *        E >= min_energy
 *        p3 >= tc * E                               tc = min_tonality * c, one float32 product made on the host
 *        band_lo <= best <= band_hi
 *      c = (float)((sum w)^2 / (2 sum w^2)), the sums in float64 over the float32 window: what one pure tone on a bin gives for
 *      p[best] / E, about 256 / 3 = 85.
 * Settings (mi_elt_cfg, 0 = the default; refused with MI_ERR_INVALID and "ELT stage: <setting> must be ..." outside the bounds):
 *   min_energy    1e-4   frame energy; finite and within 1e-12 .. 1e6
 *   min_tonality  0.5    fraction of c; within 0.01 .. 1.5
 *   band_lo       4      bins; within 2 .. 33
 *   band_hi       26     bins; within band_lo .. 33 (the default is band_lo where that is above 26)
 *   min_span      10     bins between a sweep's first and last bin; within 1 .. 31
 *   min_len       40     frames; within 2 .. 4096
 *   max_len       120    frames; within min_len .. 65536 (the default is min_len where that is above 120)
 *   max_step      3      bins between consecutive tonal frames; within 1 .. 31
 *   max_drop      2      frames without a bin inside a sweep; within 1 .. 64
 *   max_gap       10     frames between sweeps; within 1 .. 1024
 *   min_sweeps    6      sweeps before the alarm; within 1 .. 1024
 *   zero                 must be 0
 * They are a caller's settings, not tolerances, fixed from tools/elt_classes.py.
 *
 * Walker.  Per row, sequentially over the row's frames in order, its state carried in the handle.  A SEGMENT is a run of frames
 * that follows one sweep: start, first_bin, last_bin, last_frame (its last tonal frame), dir (0 until the first non-zero step, then
 * MI_ELT_UP or MI_ELT_DOWN) and drops.  A CHAIN is a run of valid sweeps: count, chain_dir, chain_first (the start of its first
 * sweep), last_end, alarmed, and bin_from / bin_to, the first and last bin of its last valid sweep.  At frame f with decision b, in
 * this order:
 *   1. b is a bin, no segment open: open one at f with first_bin = last_bin = b, last_frame = f, dir = 0, drops = 0.
 *   2. b is a bin, a segment open: step = b - last_bin.  The step is FOLLOWING iff |step| <= max_step * (1 + drops) and (step is 0, or
 *      dir is 0, or step has dir's sign).  A following step sets dir (if it was 0 and step != 0), last_bin = b, last_frame = f and
 *      drops = 0.  Any other step CLOSES the segment (4) and then opens a new one at f with b: what a beacon's retrace does.
 *   3. b is none, a segment open: drops++; if drops > max_drop, close it (4).  No segment is open afterwards.
 *   4. Closing.  The segment is a VALID SWEEP iff dir != 0, |first_bin - last_bin| >= min_span and min_len <= last_frame - start + 1
 *      <= max_len.  A valid sweep continues the chain (count++) iff count > 0, start - last_end <= max_gap and dir == chain_dir;
 *      otherwise it begins one: count = 1, chain_first = start, chain_dir = dir.  Either way last_end = last_frame, bin_from =
 *      first_bin, bin_to = last_bin.  When count reaches min_sweeps and the chain is not alarmed, alarmed = 1 and an ONSET record is
 *      emitted.  A segment that is not valid changes nothing in the chain.
 *   5. Expiry, judged last at every frame with count > 0.  The chain is ALIVE iff f - last_end <= max_gap, or a segment is open
 *      with start - last_end <= max_gap and f - start + 1 <= max_len.  Otherwise it expires: if alarmed, an END record is emitted;
 *      then the chain is cleared (count = 0, alarmed = 0, every chain field 0).
 * Decided where the rules above leave a choice, with tests/elt_model.py the tie-breaker:
 *   - A valid sweep that BEGINS a chain while an alarmed one stands (its direction differs: a beacon that flips) first emits the END
 *     record of the standing chain, with that chain's fields, and clears the alarm; the new chain raises its own ONSET when it has
 *     min_sweeps sweeps.  So alarmed == (count >= min_sweeps) always, and a row's records alternate ONSET, END, ONSET, ...
 *   - A chain that begins in the frame that expires another: the closing of item 4 comes first, so the close has already ended the
 *     old chain as above; item 5 then judges the new chain, which expires at once (silently: it is not alarmed unless min_sweeps is
 *     1) only where max_drop + 1 > max_gap.
 *   - Frame numbers, seq and every difference of frame numbers are uint32, modulo 2^32: a wrap inside a sweep or a chain changes
 *     nothing.  A segment that stays open for 2^31 frames or more (an unbroken tone for four months) has its length taken modulo
 *     2^32; set_state refuses such a state.
 *   - A consequence of item 5: a sweep of exactly max_len frames keeps its chain alive only where the retrace follows at once; one
 *     frame without a bin later f - start + 1 is over max_len while the segment is still open, and the chain expires.
 *   - Closed or cleared fields are 0 in the state, so one stream has one blob.  max_drop = 0 cannot be asked for (0 = the default).
 * An event record holds row, seq (the row's event number since creation / set_state), kind (MI_ELT_ONSET / MI_ELT_END), dir
 * (chain_dir), bin_from and bin_to (of the chain's last valid sweep), frame (the row's number of the frame that emitted it),
 * first_frame (chain_first), last_end, sweeps (count as it stood; for an ONSET min_sweeps) and batch, the call-relative batch of the
 * emitting frame.  A frame can emit up to three records (END, ONSET, END: only with min_sweeps = 1); they keep that order.
 * State: per row MI_ELT_STATE_ROW_BYTES = 776 bytes, little-endian: float32 x[178], the last 178 input samples of the last batch of
 * the last call the row was enabled in, oldest first, zeros at first; then uint32 frame (frames seen), seq (events emitted), open
 * (0 / 1), start, first_bin, last_bin, last_frame, dir, drops, count, chain_dir, chain_first, last_end, alarmed, bin_from, bin_to.  A
 * blob of zeros is a fresh state; there is no padding.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned buffers, nbatches
 * outside 1 .. max_batches. */
enum { MI_ELT_FRAME = 256, MI_ELT_HOP = 80, MI_ELT_HISTORY = 178, MI_ELT_FRAMES = 25, MI_ELT_BINS = 32, MI_ELT_BIN0 = 2, MI_ELT_STATE_ROW_BYTES = 776,
       MI_ELT_NONE8 = 0xFF };
enum { MI_ELT_ONSET = 1, MI_ELT_END = 2 };
enum { MI_ELT_UP = 1, MI_ELT_DOWN = 2 };
typedef struct {
    float min_energy, min_tonality;                 /* 0 = the default */
    uint32_t band_lo, band_hi, min_span;            /* bins; 0 = the default */
    uint32_t min_len, max_len;                      /* frames; 0 = the default */
    uint32_t max_step, max_drop, max_gap, min_sweeps; /* 0 = the default */
    uint32_t zero;
} mi_elt_cfg;                       /* 48 bytes */
typedef struct {
    uint8_t best;                   /* the bin of the largest power, 2 .. 33 */
    uint8_t bin;                    /* the decision: best, or MI_ELT_NONE8 */
    uint16_t zero;
    float energy;                   /* E */
    float p_best, p3;
} mi_elt_frame_record;              /* 16 bytes */
typedef struct {
    uint32_t row, seq;              /* seq: the row's event number since creation / set_state, 0-based */
    uint8_t kind, dir;              /* MI_ELT_ONSET / MI_ELT_END; MI_ELT_UP / MI_ELT_DOWN */
    uint8_t bin_from, bin_to;       /* first and last bin of the chain's last valid sweep */
    uint32_t frame;                 /* the row's number of the emitting frame */
    uint32_t first_frame, last_end; /* chain_first; last tonal frame of the chain's last valid sweep */
    uint32_t sweeps;                /* count as it stood */
    uint32_t batch;                 /* call-relative batch of the emitting frame */
} mi_elt_event;                     /* 32 bytes */
typedef struct mi_elt mi_elt;

/* cfg NULL = every default.  row_enabled [rows] as for mi_tones_create; rows and max_batches within the gate's limits (1 <= rows <
 * 2^20, rows * max_batches < 2^24).  max_events: capacity of the caller's event buffer, 0 = rows * the most events a row can emit in
 * max_batches batches, 2 * (1 + (25 * max_batches - 1) / (min_sweeps * min_len)) + 1.  Why: a row's records alternate ONSET and END;
 * an ONSET is emitted where a sweep closes, consecutive closes of valid sweeps lie at least min_len frames apart, and between two
 * ONSETs min_sweeps sweeps close, so the call's F = 25 * max_batches frames hold at most N = 1 + (F - 1) / (min_sweeps * min_len)
 * ONSETs (the first in the call's first frame, out of carried state) and at most N + 1 ENDs (the first out of an alarm carried in).
 * The handle owns the scratch for a call's frame decisions and events. */
int mi_elt_create(const mi_elt_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_events, int gpu, mi_elt** out);
void mi_elt_destroy(mi_elt* s);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_elt_set_rows(mi_elt* s, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the plane d_plane [rows][row_stride]: 16-byte aligned, the stride a multiple
 * of 4 floats and at least nbatches * 2000.  Outputs in device memory:
 *   d_frames           [rows][25 * nbatches]  frame records, or NULL (not wanted); 8-byte aligned.  A disabled row's are not written.
 *   d_events           [max_events]           rows ascending, seq ascending within a row (8-byte aligned)
 *   d_row_first_event  [rows + 1]             exclusive prefix of the rows' event counts
 *   d_count            [2]                    number of events, and min(that, max_events) = the number stored
 * Nothing is written at or beyond max_events.  Asynchronous on `hip_stream`, no host synchronisation; five kernels without atomics
 * -- bank (one wave per (row, batch): the 25 frames' records and decisions), walk (one lane per row: the walker over the call's
 * decisions, its events into the handle's scratch, the row's count and new walker state), scan, store (the events to their places),
 * tails (the enabled rows' last 178 samples into the carried state) -- so every byte is the same on every run and equals
 * mi_elt_plan_host's. */
int mi_elt_process_device(mi_elt* s, const float* d_plane, size_t row_stride, int nbatches, mi_elt_frame_record* d_frames, mi_elt_event* d_events,
                          uint32_t* d_row_first_event, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_elt_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and copies
 * exactly count[1] events (and the rows * 25 * nbatches frame records, if the call had a d_frames and frames is not NULL; with
 * frames not NULL after a call without d_frames it is refused).  events, frames and row_first_event may each be NULL.  The one place
 * that synchronises. */
int mi_elt_download(mi_elt* s, void* hip_stream, mi_elt_event* events, mi_elt_frame_record* frames, uint32_t* row_first_event, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_ELT_STATE_ROW_BYTES bytes in the layout above (mi_elt_plan_host reads and writes the same bytes).
 * set_state refuses a state the walker cannot be in: open or alarmed beyond 1; a closed segment or a cleared chain with a field
 * set; bins outside 2 .. 33; dir or chain_dir beyond MI_ELT_DOWN; bins that contradict dir; drops over max_drop or not the frames
 * since last_frame; a segment of 2^31 frames or more; a chain with chain_dir 0, a span under min_span, alarmed != (count >=
 * min_sweeps), or one that would have expired.  Both complete queued work first. */
size_t mi_elt_state_size(const mi_elt* s);
int mi_elt_get_state(mi_elt* s, void* buf, size_t len);
int mi_elt_set_state(mi_elt* s, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[5] = {bank, walk, scan, store, tails}.  tools/elt_rate.py. */
int mi_elt_set_timing(mi_elt* s, int on);
int mi_elt_last_launch_ms(mi_elt* s, float* ms /* [5] */);
/* The host twin: no GPU and no HIP call; the same frame records, events and state blob byte for byte.  plane [rows][row_stride] (no
 * alignment asked); state_inout rows * MI_ELT_STATE_ROW_BYTES bytes, read and updated; frames [rows][25 * nbatches] or NULL; events
 * holds max_events entries (max_events >= 1), of which min(count[0], max_events) = count[1] are written. */
int mi_elt_plan_host(const mi_elt_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride, void* state_inout,
                     mi_elt_frame_record* frames, mi_elt_event* events, size_t max_events, uint32_t* row_first_event, uint32_t* count /* [2] */);
/* The settings of cfg (NULL = all defaults) with every default filled in, or the refusal mi_elt_create would give; *c = the constant
 * of item 4 (may be NULL). */
int mi_elt_settings(const mi_elt_cfg* cfg, mi_elt_cfg* out, float* c);
/* The 256 window coefficients; the 32 recurrence coefficients of bins 2 .. 33.  Host only. */
int mi_elt_window(float* out /* [MI_ELT_FRAME] */);
int mi_elt_coeffs(float* out /* [MI_ELT_BINS] */);
/* One printable line from an event record, NUL-terminated, e.g. "ONSET down 1500.0 -> 500.0 Hz, 6 sweeps, 1.435 s": kind, direction,
 * the frequencies of bin_from and bin_to (62.5 Hz a bin), sweeps, and the seconds from first_frame to frame (0.005 s a frame, the
 * difference modulo 2^32).  Refuses a kind, a dir or a bin the stage cannot write. */
int mi_elt_event_text(const mi_elt_event* e, char* out /* [96] */);

/* ---------------- packet decoder stage: AX.25 / APRS frames per row, on the device ----------------
 * 1200 bit/s Bell 202 packet on NFM channels (AX.25 UI frames: APRS on 144.39 / 144.80 MHz, packet on marine and utility channels):
 * a 1200 Hz tone (MARK) or a 2200 Hz tone (SPACE) per bit, NRZI, HDLC framing.  The reference leaves it in the recording.  This stage
 * reads a plane [rows][row_stride] of float32 audio as mi_acars_* does, needs no flags, and writes one record per received frame
 * whose frame check sequence is right.  HDLC opens on an 8-bit flag, not on a long sync, so nothing chooses a hypothesis: a deframer
 * runs on every one of 30 LANES (three slicers times ten timing hypotheses) all the time, the frame check decides, and a rule on the
 * frames' positions keeps the copies of one frame down to one record.
 * NOT CHECKED: the air format is written from memory and pinned only to the modulator of tests/ax25_model.py; no off-air packet has
 * been through the stage.  No error correction and no bit-flip repair: one wrong bit loses the frame on that lane.
 *
 * Stream model.  As for the ACARS stage: a row's audio is one running sequence over all batches of all calls the row was enabled in;
 * samples before the handle's first call are 0.
 * Timing grid.  16000 / 1200 = 40 / 3 samples a bit; time is counted in THIRDS of a sample, sample n at third 3 n.  A bit is 40 thirds,
 * a batch 6000 thirds = exactly 150 bits, so the grid does not move from batch to batch.  Under hypothesis tau = 0 .. 9, bit k covers
 * the thirds [4 tau + 40 k, 4 tau + 40 k + 40), and sample n contributes to it when rho = 3 n - (4 tau + 40 k) lies in 0 .. 39:
 * fourteen samples where the first rho is 0, else thirteen.  The bits of a (row, batch) are those whose last sample lies in the batch,
 * exactly 150 per hypothesis, numbered by SLOT j = 0 .. 149: slot j of hypothesis tau is the bit that begins at third
 * 4 tau + 40 (j - [tau > 0]) of the batch.  The earliest sample a bit of a batch reads is the twelfth before it (tau = 1); the handle
 * carries MI_AX25_HISTORY = 14 samples per row, the smallest H >= 13 whose lead H + 2 (carry.hpp) is whole float4.  Positions are
 * ABSOLUTE THIRDS, 64 bits: 6000 * (the row's batches before the batch) + the third within it.  Slot j of hypothesis tau in the
 * row's batch B ends -- and slot j + 1 begins -- at 6000 B + 4 tau + 40 (j + 1 - [tau > 0]).
 * Bit bank, per (row, batch, tau, slot); float32, every operation rounded on its own, no fused multiply-add.  Four templates of 40
 * entries (mi_ax25_templates): T[0][rho] = cos(2 pi 1200 rho / 48000), T[1] the sine, T[2][rho] = cos(2 pi 2200 rho / 48000), T[3]
 * the sine, evaluated in double and rounded once.  s_i = sum x[n] * T[i][rho] over the bit's samples in ascending n, each sum
 * beginning with its first product; pm = s_0 * s_0 + s_1 * s_1, ps = s_2 * s_2 + s_3 * s_3.  THREE slicers share the sums: TONE bit
 * t_g = 1 (mark) if pm >= gain[g] * ps, g = 0, 1, 2.  Behind an NFM de-emphasis the 2200 Hz tone arrives weaker than the 1200 Hz one,
 * by an amount that depends on whether the transmitter pre-emphasised: gain[0] = 1 is flat audio, gain[2] the power tilt measured
 * behind this project's NFM path for a flat-deviation transmitter, gain[1] their geometric mean.  Packed: 5 words per
 * (row, batch, g, tau), slot j in bit j % 32 of word j / 32, the upper 10 bits of word 4 zero.  A block whose 2000 samples and 14
 * carried samples are all +-0 gives t = 1 everywhere (0 >= gain * 0); the device writes that without the sums.
 * Deframers.  Lane l = 10 g + tau, l = 0 .. 29; the lanes are independent.  Per slot a lane takes its tone bit t:
 *   d = 1 if t equals the lane's previous tone bit, else 0 (NRZI); the previous tone bit becomes t.  n = the lane's ONES count.
 *   d = 1: ones = min(n + 1, 7).  n <= 4: the 1 is COLLECTED.  n = 5: a sixth one is never data and is not collected.  n = 6: ABORT --
 *     the lane forgets its frame (every frame field 0) and WAITS for a flag.  n = 7: nothing.
 *   d = 0: ones = 0.  n <= 4: the 0 is collected.  n = 5: a stuffed bit, dropped.  n = 6: a FLAG (below).  n = 7: nothing.
 *   Collected (only IN A FRAME, i.e. behind a flag): the bit goes into the running byte, least significant first, and through the
 *   lane's CRC register (reflected polynomial 0x8408, the register starts a frame at 0xFFFF).  The eighth bit ends a byte: it is byte
 *   number nbytes of the frame, unless the frame already has MI_AX25_MAX_BYTES = 330 (10 addresses, control, PID, 256 of information,
 *   2 of the check): then the lane aborts as above.
 *   A flag's own 0 and first five ones are collected like any bits before the flag is known.  So at a flag a frame holds WHOLE BYTES
 *   when its running byte has exactly those 6 bits, and its register has taken them too: the frame check CRC-16/X.25 over the whole
 *   bytes (initial value 0xFFFF, the check sent low byte first and complemented) leaves the residue 0xF0B8, which those six bits
 *   advance to MI_AX25_FLAG_RESIDUE; the step is one to one, so the register equals it exactly when the residue was right.
 *   At a flag the lane CLOSES a candidate if it is in a frame that holds whole bytes, at least 17, whose frame check is right, and --
 *   under `strict` -- whose ADDRESS FIELD is well formed: the first byte with bit 0 set is byte 7 a - 1 for a number of addresses
 *   a = 2 .. 10, 7 a + 3 <= nbytes (a control byte and the check follow), and every byte i < 7 a with i % 7 != 6 shifted right by one
 *   is 'A'-'Z', '0'-'9' or a space.  naddr = a, or 0 where the field is not well formed (a record only without strict).
 *   A flag always opens the next frame, whether or not it closed one: the lane is in a frame with no bits, no bytes, the register
 *   0xFFFF, and START = the position where the next slot begins.  Frames may share one flag, and flags one 0.
 * One record per frame.  Slots are taken in order and within a slot the lanes in ascending l.  END of a candidate = the position
 * where the slot behind its closing flag's last bit begins.  A candidate is a record unless start + 40 < last_end, the end of the
 * row's last record (0 before the first): its first bit begins more than one bit before that record's closing flag ended.  A record
 * sets last_end to its end.  That is the duplicate filter -- the other lanes' copies of a frame start at least 17 bytes before its
 * end -- and the capacity bound: a frame takes 136 bits and its closing flag 8, so the ends of two records on one lane, or on lanes
 * that saw the flag in the same slot, lie 144 bits apart, and a lane that opened one bit before the last record's end can close 143
 * bits behind it; ends lie inside the call's 150 n bits, so a row has at most 1 + 150 n / 143 records in n batches.  Frames of 17
 * bytes sharing their flags on one lane give 1 + (150 n - 1) / 144, which is the same number for n <= 20 (tests reach it).
 * No timing moves: a lane's grid is fixed; the ten lanes four thirds apart are the tracker (DESIGN.md 5r has the clock offset the
 * longest frame survives).
 * Settings (mi_ax25_cfg, 0 = the default): gain[3], each finite and > 0, 0 = its default, MI_AX25_GAIN0 / 1 / 2; strict, 0 = on,
 * MI_AX25_STRICT_OFF = off (1 = on, said out loud).
 * Record: row; batch and third, where the first bit behind the opening flag begins (start / 6000 modulo 2^32 and start % 6000);
 * end_batch, the call's batch in which the closing flag ended; nbytes 17 .. 330, the check's two included; lane; naddr; the raw
 * bytes, zeros behind them.
 * State: per row MI_AX25_STATE_ROW_BYTES = 10544 bytes, little-endian, a blob of zeros being a fresh state: float32 x[14], the last
 * 14 input samples, oldest first; uint64 batch (batches seen, < 2^40); uint64 last_end; then per lane, 30 entries each: uint64 start;
 * uint16 nbytes; uint16 crc (the register over every collected bit, the running byte's included); uint8 prev (the previous tone
 * bit); uint8 ones (0 .. 7); uint8 phase (MI_AX25_WAIT / MI_AX25_FRAME); uint8 nbits and uint8 cur (the running byte's bits); then
 * uint8 zero[2]; then bytes[30][332], a lane's whole bytes so far with zeros behind them.  A waiting lane's start, nbytes, crc, nbits,
 * cur and bytes are all zero.  A disabled row writes nothing and every byte of its state stays.  NaN and Inf are unspecified.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned buffers, nbatches
 * outside 1 .. max_batches. */
enum { MI_AX25_HISTORY = 14, MI_AX25_HYPOTHESES = 10, MI_AX25_SLICERS = 3, MI_AX25_LANES = 30, MI_AX25_BITS = 150, MI_AX25_BIT_WORDS = 5,
       MI_AX25_MIN_BYTES = 17, MI_AX25_MAX_BYTES = 330, MI_AX25_RAW_BYTES = 332, MI_AX25_STATE_ROW_BYTES = 10544 };
enum { MI_AX25_WAIT = 0, MI_AX25_FRAME = 1 };
enum { MI_AX25_RESIDUE = 0xF0B8, MI_AX25_FLAG_RESIDUE = 0x9F0B }; /* the second: the first through the bits 0 1 1 1 1 1 */
#define MI_AX25_STRICT_OFF 0x80000000u /* strict: frames whose address field is not well formed are records too */
#define MI_AX25_GAIN0 1.0f
#define MI_AX25_GAIN1 1.6432f /* sqrt(2.7) */
#define MI_AX25_GAIN2 2.7f    /* tools/ax25_classes.py: 2.7002, +4.31 dB */
typedef struct {
    float gain[3];                  /* weight of the space power in slicer g's decision; 0 = the default */
    uint32_t strict;                /* 0 or 1 = on; MI_AX25_STRICT_OFF */
} mi_ax25_cfg;                      /* 16 bytes */
typedef struct {
    uint32_t row;
    uint32_t batch, third;          /* where the first bit behind the opening flag begins */
    uint32_t end_batch;             /* call-relative */
    uint16_t nbytes;                /* 17 .. 330, the two of the check included */
    uint8_t lane;                   /* 10 g + tau */
    uint8_t naddr;                  /* 2 .. 10; 0: the address field is not well formed */
    uint8_t bytes[332];             /* raw; zeros behind nbytes */
} mi_ax25_frame;                    /* 352 bytes */
typedef struct mi_ax25 mi_ax25;

/* cfg NULL = every default.  row_enabled, rows and max_batches as for mi_acars_create.  max_frames: capacity of the caller's frame
 * buffer, 0 = rows * the most records a row can have in max_batches batches, 1 + 150 * max_batches / 143.  The handle owns the
 * scratch for a call's tone bits and frames. */
int mi_ax25_create(const mi_ax25_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_frames, int gpu, mi_ax25** out);
void mi_ax25_destroy(mi_ax25* s);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_ax25_set_rows(mi_ax25* s, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the plane d_plane [rows][row_stride]: 16-byte aligned, the stride a multiple
 * of 4 floats and at least nbatches * 2000.  Outputs in device memory:
 *   d_bits             [rows][nbatches][3][10][5]  the packed tone bits, or NULL (the handle's scratch); 4-byte aligned.  A disabled
 *                                                  row's are not written.
 *   d_frames           [max_frames]                rows ascending, time order within a row (8-byte aligned)
 *   d_row_first_frame  [rows + 1]                  exclusive prefix of the rows' frame counts
 *   d_count            [2]                         number of frames, and min(that, max_frames) = the number stored
 * Nothing is written at or beyond max_frames.  Asynchronous on `hip_stream`, no host synchronisation; five kernels without atomics
 * -- bits (one workgroup per (row, batch)), walk (one wave per row, a lane per deframer), scan, store, tails -- so every byte is the
 * same on every run and equals mi_ax25_plan_host's. */
int mi_ax25_process_device(mi_ax25* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, mi_ax25_frame* d_frames,
                           uint32_t* d_row_first_frame, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_ax25_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] frames.  frames and row_first_frame may each be NULL.  The one place that synchronises. */
int mi_ax25_download(mi_ax25* s, void* hip_stream, mi_ax25_frame* frames, uint32_t* row_first_frame, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_AX25_STATE_ROW_BYTES bytes in the layout above (mi_ax25_plan_host reads and writes the same bytes).
 * set_state refuses an impossible state: batch at or beyond 2^40, a position beyond the row's next batch (last_end, or a start in a
 * frame), a start later than the lane's collected bits allow (start + 40 (8 nbytes + nbits) beyond where the lane's last slot ended:
 * the capacity bound rests on it), zero not 0, and per lane prev beyond 1, ones beyond 7, an unknown phase, nbits beyond 7, cur beyond its nbits bits, nbytes
 * beyond 330, a waiting lane with a frame field or a byte set, a crc that the bytes and the running bits do not give, a byte set
 * behind the ones taken.  Both complete queued work first. */
size_t mi_ax25_state_size(const mi_ax25* s);
int mi_ax25_get_state(mi_ax25* s, void* buf, size_t len);
int mi_ax25_set_state(mi_ax25* s, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[5] = {bits, walk, scan, store, tails}.  tools/ax25_rate.py. */
int mi_ax25_set_timing(mi_ax25* s, int on);
int mi_ax25_last_launch_ms(mi_ax25* s, float* ms /* [5] */);
/* The host twin: no GPU and no HIP call; the same bits, frames and state blob byte for byte.  plane [rows][row_stride] (no alignment
 * asked); state_inout rows * MI_AX25_STATE_ROW_BYTES bytes, read and updated; bits [rows][nbatches][3][10][5] or NULL; frames holds
 * max_frames entries (max_frames >= 1), of which min(count[0], max_frames) = count[1] are written. */
int mi_ax25_plan_host(const mi_ax25_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                      void* state_inout, uint32_t* bits, mi_ax25_frame* frames, size_t max_frames, uint32_t* row_first_frame,
                      uint32_t* count /* [2] */);
/* The settings of cfg (NULL = all defaults) with every default filled in (strict as 1 or MI_AX25_STRICT_OFF), or the refusal
 * mi_ax25_create would give. */
int mi_ax25_settings(const mi_ax25_cfg* cfg, mi_ax25_cfg* out);
/* The four templates, T[i][rho] at t[40 i + rho].  Host only. */
int mi_ax25_templates(float* t /* [160] */);
/* CRC-16/X.25 of n bytes, complemented as it is sent: 0x906E for "123456789" (NULL with n = 0 is fine; NULL otherwise gives
 * 0xFFFFFFFF, which no CRC is).  A frame's bytes with the check behind them, low byte first, give 0x0F47 = ~0xF0B8. */
uint32_t mi_ax25_crc(const uint8_t* bytes, size_t n);
/* The TNC2 line of a record, NUL-terminated, into text[cap]: SRC-S>DST-S,DIGI-S*,..:info -- the destination is the frame's first
 * address, the source its second; callsigns without their trailing spaces; a zero SSID (bits 1 .. 4 of an address's last byte) is
 * omitted; '*' behind the last digipeater whose H bit (bit 7 of its last byte) is set; info = the bytes behind control and PID (behind
 * control alone where the control byte is not 0x03 / 0x13, a UI frame's) up to the check, a byte outside 0x20 .. 0x7E written as '.'.
 * Refuses nbytes outside 17 .. 330, an address field that is not well formed (what strict refuses), and a cap the line does not fit
 * (MI_AX25_TEXT_BYTES always fits). */
enum { MI_AX25_TEXT_BYTES = 384 };
int mi_ax25_frame_text(const mi_ax25_frame* f, char* text, size_t cap);

/* ---------------- pager decoder stage: POCSAG messages per row, on the device ----------------
 * POCSAG is the 512 / 1200 / 2400 bit/s pager format: direct FSK of the carrier, +-4.5 kHz, which an NFM channel's discriminator
 * turns into NRZ audio.  The reference leaves it in the recording.  This stage reads a plane [rows][row_stride] of float32 audio as
 * mi_acars_* does, needs no flags, and writes one record per page (a MESSAGE).  It is the first decoder stage with forward error
 * correction: BCH(31,21) repair of up to two bits a codeword, by a table of the 497 syndromes of the error patterns of weight <= 2.
 * NOT CHECKED against off-air traffic: no recorded pager channel has been through the stage.  SYNC, IDLE, the generator and the
 * character codes are the published ones and were checked for consistency (both words have remainder 0 and even parity; the 497
 * patterns have 497 distinct syndromes), and the rest is pinned only to the modulator of tests/pocsag_model.py.  No reassembly of
 * pages sent in parts, no address filter, no FLEX.
 *
 * Air format.  A codeword is 32 bits, the first bit sent being bit 31.  Bit 31 is the kind, 0 address and 1 message; then 20 payload
 * bits; bits 10 .. 1 are the check bits of BCH(31,21), the remainder of bits 31 .. 11 times x^10 under the generator 0x769; bit 0
 * makes the parity of all 32 even.  SYNC is 0x7CD215D8, IDLE 0x7A89C197.  A transmission is a preamble of at least 576 alternating
 * bits, then GROUPS (the standard's "batch", a word that is taken here): SYNC and 16 codewords, index c = 0 .. 15.  An address word
 * carries 18 address bits (30 .. 13) and 2 function bits (12 .. 11); the full address is addr18 << 3 | c >> 1.  The lower radio
 * frequency is bit 1; receivers differ in the sign of their discriminator, so the stage takes both polarities and says which.
 * Stream model.  As for the ACARS stage: a row's audio is one running sequence over all batches of all calls the row was enabled
 * in; samples before the handle's first call are 0.
 * Timing grid.  Time is counted in TWELFTHS of a sample; sample n sits at twelfth 12 n; a batch is 24000 twelfths.  The baud is a
 * setting of the handle: a bit is L twelfths, there are H hypotheses a STEP = L / H twelfths apart, B = 24000 / L bits of a batch
 * and hypothesis in W = ceil(B / 32) words (mi_pocsag_geometry):
 *     baud 512: L 375, H 15, step 25, B 64, W 2;   1200: L 160, H 10, step 16, B 150, W 5;   2400: L 80, H 10, step 8, B 300, W 10.
 * Under hypothesis tau = 0 .. H - 1, bit k covers the twelfths [tau step + L k, tau step + L k + L), k counted from the row's first
 * sample, and sample n belongs to it when 12 n lies in that span (31 or 32 samples at 512 baud, 13 or 14 at 1200, 6 or 7 at 2400).
 * tau + H is tau one bit later, exactly.  The bits of a (row, batch) are those whose last sample lies in the batch, exactly B per
 * hypothesis, numbered by SLOT j = 0 .. B - 1: slot j of hypothesis tau is the bit that begins at twelfth tau step + L (j - [tau > 0])
 * of the batch, so slot 0 of tau >= 1 begins before the batch.  The earliest is tau = 1, at twelfth step - L: -350 at 512 baud, whose
 * first sample is the 29th before the batch (-348), -144 at 1200 (the 12th), -72 at 2400 (the 6th).  The handle carries
 * MI_POCSAG_HISTORY = 34 samples per row at every baud -- at least the 29, the lead 34 + 2 (carry.hpp) whole float4, and one size
 * of blob for every baud.  In one slot, hypothesis tau begins a step after tau - 1 for tau = 2 .. H - 1, and 0 a step after H - 1:
 * a walker steps between H - 1 and 0 as between any two neighbours.  Hypothesis 1 begins a step after hypothesis 0 OF THE SLOT BEFORE.
 * Bit bank, per (row, batch, lane, slot), lane = H g + tau for the slicer g = 0, 1; float32, every operation rounded on its own, no
 * fused multiply-add.  s = the sum of the bit's samples in ascending n, beginning with the first; k = their number.  Slicer 0:
 * v = s.  Slicer 1: v = s - (float)k * mu, mu = S / 2000.0f, S the sum of the batch's 2000 samples in the order of the ACARS
 * stage's Q: s_l = the sequential sum over the samples n = l (mod 64) in ascending n, l = 0 .. 63; then s_l + s_{l + 32} for l < 32,
 * then + 16, 8, 4, 2, 1 in the same way; S is element 0.  (Slicer 1 is for a discriminator with a tuning offset.)  The bit is 1 if
 * v < 0.  Q[lane] of the block is the sum of |v| over its slots in that same order, slot j in the place of sample n.  Packed: W
 * words per (row, batch, lane), slot j in bit j % 32 of word j / 32, the bits behind B zero: bits [rows][nbatches][2][H][W] and
 * q [rows][nbatches][2][H].  A block whose 2000 samples and 34 carried samples are all +-0 gives bits 0 and Q = +0.0f everywhere;
 * the device writes that without the sums.
 * Sync.  Every lane keeps its last 64 bits.  While a row is IDLE, at every slot in order, a lane HITS when its newest 32 bits
 * differ from SYNC in at most sync_errors places (polarity as sent) or from SYNC's complement in at most that many (INVERTED), and
 * the 32 bits before them differ from 0xAAAAAAAA or from 0x55555555 in at most preamble_errors places.  The first slot with a hit
 * opens a TRANSMISSION on the hitting lane with the fewest sync mismatches, then the largest Q of that batch, then the lowest
 * lane.  One transmission at a time per row; hits inside one are ignored.
 * Walker.  From the slot after the hit the chosen lane's bits, polarity undone, 32 to a word, the first in bit 31; a word's place
 * (batch, twelfth) is where its first bit begins.  ONE WORD (mi_pocsag_decode): the syndrome of bits 31 .. 1 under 0x769; e = the
 * weight of the one error pattern of weight <= 2 in those 31 bits with that syndrome (0 for syndrome 0), the word BAD if there is
 * none; the pattern is undone, and if the parity of the 32 bits is then odd, e + 1 and bit 0 is flipped.  GOOD if e <= correct,
 * stored corrected; else BAD, stored as received.  Words c = 0 .. 15 of a group: a good IDLE closes the open message; a good
 * address word closes it and opens one (address, function, the word's place, its e into corrected); a good message word is
 * appended to the open message with its e added to corrected -- dropped if none is open, and beyond MI_POCSAG_MAX_WORDS = 80
 * dropped with truncated set --; a bad word is appended with its bit in the mask `bad` and counted in nbad, under the same two
 * conditions.  Behind word 15 of a group whose 16 words were all bad the transmission ENDS: the open message closes and the row is
 * idle from the next slot.  Otherwise the next 32 bits must differ from SYNC in at most sync_errors places (no preamble is asked);
 * then the next group follows, else the transmission ends in the same way.  A closed message is a record; an address word alone
 * is a record with 0 words (a tone-only page).
 * Timing moves.  At the first slot of every batch that begins inside a transmission (unless hold_timing is 1), with Q of the new
 * batch and the lanes of the transmission's slicer g: v = tau; if Q[tau - 1] > Q[v] then v = tau - 1; if Q[tau + 1] > Q[v] then
 * v = tau + 1 (indices mod H; a tie keeps tau, a tie between the neighbours that beats tau goes to tau - 1); tau = v.  The walker
 * stays in step except between 0 and 1: moving 0 -> 1 it passes over slot 0 of the new batch, moving 1 -> 0 it first takes
 * hypothesis 0's last bit of the batch before, out of the lane's history, then slot 0.  The slicer never changes in a transmission.
 * Settings (mi_pocsag_cfg, 0 = the default): baud 512, 1200 (default) or 2400; sync_errors 1 .. 4, default 2,
 * MI_POCSAG_SYNC_EXACT for none; preamble_errors 1 .. 8, default 4, MI_POCSAG_PREAMBLE_EXACT for none, MI_POCSAG_PREAMBLE_OFF
 * drops the condition (a receiver that joins a transmission at a later group); correct 1 (default) or 2, MI_POCSAG_CORRECT_NONE:
 * at 1 a random word passes as good with probability 33 / 2048, at 2 with 1 / 4; hold_timing 0 / 1.
 * Record (mi_pocsag_message, 368 bytes): at 0 row; 4 batch and 8 twelfth, the address word's place (the row's batch number since
 * creation / set_state, wrapping at 2^32, and 0 .. 23999); 12 end_batch, the call's batch in which the message closed; 16 address
 * (21 bits); 20 function, 21 nwords, 22 nbad, 23 truncated; 24 corrected (the e of the address word and the good words); 26
 * inverted; 27 sync_errors, the hit's mismatches; 28 lane_sync and 29 lane_end, the lane at the hit and at the close; 30 zero; 32
 * bad[3], bit i % 32 of bad[i / 32] for word i; 44 zero2; 48 words[80], zeros behind nwords.
 * State: per row MI_POCSAG_STATE_ROW_BYTES = 800 bytes, little-endian, a blob of zeros being a fresh state: float32 x[34], the last
 * 34 input samples, oldest first; at 136 uint32 batch (batches seen), 140 phase (MI_POCSAG_IDLE / MI_POCSAG_TRANSMISSION); 144 uint64
 * hist[30], per lane the last 64 bits, the newest in bit 0 (lanes the baud does not have stay 0); at 384 uint32 lane, inverted, pos
 * (words of the group taken, 16 = SYNC is next), cur and nbits (the running word), gbad (bad words of the group), lane_sync,
 * mismatches, wbatch and wtwelfth (the running word's place), open, zero; at 432 the open message as the record has it so far
 * (row, end_batch and lane_end 0).  An idle row's fields from `lane` on are all zero.  A disabled row writes nothing and every byte
 * of its state stays.  The baud is not in the blob: one moved between handles of different baud is the caller's error, refused only
 * where a lane does not exist.  NaN and Inf are unspecified.
 * Capacity.  A message closes at the end of a 32-bit word, and no two closes share a word.  A call of n batches gives the walker n B
 * slots and at most n bits more (one 1 -> 0 move a batch), and the first word can end with the first of them, so a row closes at
 * most 1 + (n (B + 1) - 1) / 32 messages: mi_pocsag_max_messages.
 * MI_ERR_NO_DEVICE without a GPU (create only); MI_ERR_INVALID for bad arguments, refused settings, misaligned buffers, nbatches
 * outside 1 .. max_batches. */
enum { MI_POCSAG_HISTORY = 34, MI_POCSAG_MAX_HYPOTHESES = 15, MI_POCSAG_MAX_LANES = 30, MI_POCSAG_MAX_WORDS = 80, MI_POCSAG_STATE_ROW_BYTES = 800 };
enum { MI_POCSAG_IDLE = 0, MI_POCSAG_TRANSMISSION = 1 };
enum { MI_POCSAG_TEXT_AUTO = 0, MI_POCSAG_TEXT_NUMERIC = 1, MI_POCSAG_TEXT_ALPHA = 2 };
#define MI_POCSAG_SYNC 0x7CD215D8u
#define MI_POCSAG_IDLE_WORD 0x7A89C197u
#define MI_POCSAG_SYNC_EXACT 0x80000000u     /* sync_errors: no mismatch allowed */
#define MI_POCSAG_PREAMBLE_EXACT 0x80000000u /* preamble_errors: no mismatch allowed */
#define MI_POCSAG_PREAMBLE_OFF 0x80000001u   /* preamble_errors: the 32 bits before SYNC are not looked at */
#define MI_POCSAG_CORRECT_NONE 0x80000000u   /* correct: a word is good only as received */
typedef struct {
    uint32_t baud;                  /* 0 = 1200; 512, 1200, 2400 */
    uint32_t sync_errors;           /* 0 = 2; 1 .. 4; MI_POCSAG_SYNC_EXACT */
    uint32_t preamble_errors;       /* 0 = 4; 1 .. 8; MI_POCSAG_PREAMBLE_EXACT; MI_POCSAG_PREAMBLE_OFF */
    uint32_t correct;               /* 0 = 1; 1, 2; MI_POCSAG_CORRECT_NONE */
    uint32_t hold_timing;           /* 1: no timing moves */
} mi_pocsag_cfg;                    /* 20 bytes */
typedef struct {
    uint32_t row;
    uint32_t batch, twelfth;        /* where the address word's first bit begins */
    uint32_t end_batch;             /* call-relative */
    uint32_t address;               /* 21 bits */
    uint8_t function, nwords, nbad, truncated;
    uint16_t corrected;             /* bits repaired in the address word and the good words */
    uint8_t inverted, sync_errors;
    uint8_t lane_sync, lane_end;
    uint16_t zero;
    uint32_t bad[3];
    uint32_t zero2;
    uint32_t words[80];             /* message words, corrected where good; zeros behind nwords */
} mi_pocsag_message;                /* 368 bytes */
typedef struct mi_pocsag mi_pocsag;

/* cfg NULL = every default.  row_enabled, rows and max_batches as for mi_acars_create.  max_messages: capacity of the caller's
 * message buffer, 0 = rows * mi_pocsag_max_messages(baud, max_batches).  The handle owns the scratch for a call's bits, Q and
 * messages, and the syndrome table. */
int mi_pocsag_create(const mi_pocsag_cfg* cfg, const uint8_t* row_enabled, int rows, int max_batches, size_t max_messages, int gpu, mi_pocsag** out);
void mi_pocsag_destroy(mi_pocsag* s);
/* Other rows from the next call on; all state stays.  Completes the work queued on the device first. */
int mi_pocsag_set_rows(mi_pocsag* s, const uint8_t* row_enabled /* [rows] */);
/* One call over nbatches (1 .. max_batches) batches of the plane d_plane [rows][row_stride]: 16-byte aligned, the stride a multiple
 * of 4 floats and at least nbatches * 2000.  Outputs in device memory:
 *   d_bits               [rows][nbatches][2][H][W]  the packed bits, or NULL (the handle's scratch); 4-byte aligned.
 *   d_q                  [rows][nbatches][2][H]     Q, or NULL (the handle's scratch).  A disabled row's are not written.
 *   d_messages           [max_messages]             rows ascending, in the order they closed within a row (8-byte aligned)
 *   d_row_first_message  [rows + 1]                 exclusive prefix of the rows' message counts
 *   d_count              [2]                        number of messages, and min(that, max_messages) = the number stored
 * Nothing is written at or beyond max_messages.  Asynchronous on `hip_stream`, no host synchronisation; five kernels without
 * atomics -- bits (one workgroup per (row, batch)), walk (one wave per row, a lane per lane of the bank), scan, store, tails -- so
 * every byte is the same on every run and equals mi_pocsag_plan_host's. */
int mi_pocsag_process_device(mi_pocsag* s, const float* d_plane, size_t row_stride, int nbatches, uint32_t* d_bits, float* d_q,
                             mi_pocsag_message* d_messages, uint32_t* d_row_first_message, uint32_t* d_count, void* hip_stream);
/* Results of the last mi_pocsag_process_device, which must have been enqueued on `hip_stream`: waits for it, reads the counts and
 * copies exactly count[1] messages.  messages and row_first_message may each be NULL.  The one place that synchronises. */
int mi_pocsag_download(mi_pocsag* s, void* hip_stream, mi_pocsag_message* messages, uint32_t* row_first_message, uint32_t* count /* [2] */);
/* Checkpoint / resume, rows * MI_POCSAG_STATE_ROW_BYTES bytes in the layout above (mi_pocsag_plan_host reads and writes the same
 * bytes).  set_state refuses an impossible state: zero not 0; an unknown phase; history bits in a lane the baud does not have; an
 * idle row with a walker field or a byte of the message set; inside a transmission a lane or lane_sync the baud does not have or
 * the two on different slicers, inverted or open beyond 1, pos beyond 16, nbits beyond 31, cur beyond its nbits bits, gbad beyond
 * pos or 16 of 16, mismatches beyond 4, wtwelfth beyond 23999; a message set though none is open; and of an open message a row,
 * end_batch, lane_end or zero field set, an address beyond 21 bits, a function beyond 3, nwords beyond 80, truncated beyond 1 or
 * set below 80 words, a twelfth beyond 23999, inverted, lane_sync or sync_errors that are not the transmission's, bad bits or
 * words behind nwords, an nbad that is not the mask's count, a corrected beyond 2 (nwords - nbad + 1).  Both complete queued work
 * first. */
size_t mi_pocsag_state_size(const mi_pocsag* s);
int mi_pocsag_get_state(mi_pocsag* s, void* buf, size_t len);
int mi_pocsag_set_state(mi_pocsag* s, const void* buf, size_t len);
/* (diagnostic) as mi_outgate_set_timing; ms[5] = {bits, walk, scan, store, tails}.  tools/pocsag_rate.py. */
int mi_pocsag_set_timing(mi_pocsag* s, int on);
int mi_pocsag_last_launch_ms(mi_pocsag* s, float* ms /* [5] */);
/* The host twin: no GPU and no HIP call; the same bits, Q, messages and state blob byte for byte.  plane [rows][row_stride] (no
 * alignment asked); state_inout rows * MI_POCSAG_STATE_ROW_BYTES bytes, read and updated; bits [rows][nbatches][2][H][W] and
 * q [rows][nbatches][2][H], each or NULL; messages holds max_messages entries (max_messages >= 1), of which
 * min(count[0], max_messages) = count[1] are written. */
int mi_pocsag_plan_host(const mi_pocsag_cfg* cfg, const uint8_t* row_enabled, int rows, int nbatches, const float* plane, size_t row_stride,
                        void* state_inout, uint32_t* bits, float* q, mi_pocsag_message* messages, size_t max_messages,
                        uint32_t* row_first_message, uint32_t* count /* [2] */);
/* The settings of cfg (NULL = all defaults) with every default filled in, or the refusal mi_pocsag_create would give. */
int mi_pocsag_settings(const mi_pocsag_cfg* cfg, mi_pocsag_cfg* out);
/* H, B and W of a baud (0 = 1200); each pointer may be NULL.  Refuses any other baud.  Host only, as the four below. */
int mi_pocsag_geometry(uint32_t baud, int* hypotheses, int* bits, int* words);
/* The most messages one row can close in nbatches batches at a baud; 0 for a refused baud. */
uint32_t mi_pocsag_max_messages(uint32_t baud, uint64_t nbatches);
/* The codeword of 21 data bits (bit 20 the kind): check bits and parity appended.  mi_pocsag_encode(MI_POCSAG_SYNC >> 11) is SYNC. */
uint32_t mi_pocsag_encode(uint32_t data21);
/* The walker's rule for one word: 1 GOOD, 0 BAD, MI_ERR_INVALID for a refused `correct` (a setting, 0 = the default).  *fixed = the
 * word as stored, *errors = e (for a bad word whose syndrome has a pattern, what the repair would have taken; where it has
 * none, 3).  fixed and errors may be NULL. */
int mi_pocsag_decode(uint32_t word, uint32_t correct, uint32_t* fixed, uint32_t* errors);
/* A record's text, NUL-terminated, into text[cap].  MI_POCSAG_TEXT_NUMERIC: every word's 20 payload bits (30 .. 11) as five 4-bit
 * BCD digits, each least significant bit first, "0123456789*U -)(" ; MI_POCSAG_TEXT_ALPHA: the payloads as one bit string, 7-bit
 * characters least significant bit first, a character outside 0x20 .. 0x7E written '.', trailing bits short of a character and
 * trailing NUL / ETX / EOT characters left out; a character (or digit) with a bit out of a bad word is '?'.  MI_POCSAG_TEXT_AUTO:
 * function 0 numeric, any other alpha.  Refuses nwords beyond 80, an unknown mode and a cap the text does not fit
 * (MI_POCSAG_TEXT_BYTES always fits). */
enum { MI_POCSAG_TEXT_BYTES = 408 };
int mi_pocsag_message_text(const mi_pocsag_message* m, int mode, char* text, size_t cap);

/* ---------------- multi-GPU: gather of audio + flags to rank 0 ----------------
 * One process per GPU; device streams are independent (one demod thread per device in the reference,
 * rtl_airband.cpp:1044-1078) and are partitioned stream-major over the ranks; nothing crosses GPUs except this gather, which
 * brings every rank's decimated audio and axcindicate flags to rank 0, where the reference's output / mixer threads run
 * (output.cpp:899-961).  RCCL point-to-point on the gather's own stream (librccl.so.1 is loaded on first use).
 *   mi_gather_unique_id   rank 0 makes the 128-byte id; the host program hands it to every rank (its launcher's channel)
 *   mi_gather_create      streams_per_rank[world]; max_batches bounds nbatches of a step
 *   mi_gather_audio       one step, every rank: d_waveout [streams_local][nch][nbatches*WAVE_BATCH], d_axc [streams_local][nch][nbatches]
 *                         as mi_demod_process_device wrote them on `hip_stream`; on rank 0 the job-wide arrays
 *                         d_all_waveout [streams_total][nch][nbatches*WAVE_BATCH], d_all_axc [streams_total][nch][nbatches] (ignored elsewhere).
 *                         Asynchronous: it starts when `hip_stream` reaches this point and runs on the gather's stream beside
 *                         whatever the caller enqueues next; do not overwrite its inputs / read its outputs before
 *                         mi_gather_stream_wait (makes a stream wait for it) or mi_gather_sync (the host waits).
 *                         open_only != 0: only the (row, batch) blocks whose flag is not MI_NO_SIGNAL travel -- what the reference's
 *                         non-continuous outputs consume (output.cpp:518,568) -- and rank 0 gets zeros for the others; this mode
 *                         synchronises the gather's stream with the host once per step (it needs the block counts). */
typedef struct { char internal[128]; } mi_gather_id;
typedef struct mi_gather mi_gather;
int mi_gather_unique_id(mi_gather_id* id);
/* TEST TRANSPORT: an id that makes mi_gather_create connect the ranks of job number `job` through an in-process loopback (one host
 * thread per rank, any GPU -- all on the same one is fine) instead of RCCL: device-to-device copies ordered by events, same
 * send / recv / group call sequence.  It lets a single-GPU machine execute every world > 1 branch of mi_gather_audio. */
int mi_gather_loopback_id(mi_gather_id* id, uint64_t job);
int mi_gather_create(const mi_gather_id* id, int rank, int world, int gpu, const int* streams_per_rank, int nch, int max_batches, mi_gather** out);
void mi_gather_destroy(mi_gather* g);
int mi_gather_audio(mi_gather* g, const float* d_waveout, const char* d_axc, int nbatches, int open_only, float* d_all_waveout, char* d_all_axc,
                    void* hip_stream);
int mi_gather_stream_wait(mi_gather* g, void* hip_stream);
int mi_gather_sync(mi_gather* g);

#ifdef __cplusplus
}
#endif
#endif /* MI_AIRBAND_H */
