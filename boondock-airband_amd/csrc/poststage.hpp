// poststage.hpp -- what the post-stages (outgate.hip, txsplit.hip, tones.hip, pcm.hip, aspec.hip, vband.hip, limit.hip, denoise.hip, selcal.hip, acars.hip, same.hip, elt.hip, ax25.hip, pocsag.hip, mixer.hip, gather.hip, survey.hip, occupancy.hip, probe.hip) and the host twins (poststage_host.cpp)
// share on the host side: the error helper, argument checks, launch timing, the handle bases (Stage, BatchStage, RowStage, IqFront)
// with the bodies of the entry points every handle repeats (geometry, set_rows, set_timing, last_launch_ms, destroy, the state blob in
// and out, the checks of a plane-in / plane-out call, the create checks, table upload, I/Q checks and kernel arguments of an I/Q front
// stage), the row scan's launcher and the blob layouts.  The device side of a stage that carries samples from call to call -- the
// lead's load and the tails kernel -- is in carry.hpp; that of a stage that reads raw I/Q is in iq_front.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "hip_own.hpp"
#include "plan.hpp"

namespace mi {

std::string& last_error_ref();  // mi_airband.cpp

inline int fail(int code, const std::string& msg) {
    last_error_ref() = msg;
    return code;
}

inline bool aligned(const void* p, uintptr_t a) {
    return reinterpret_cast<uintptr_t>(p) % a == 0;
}

// truth values as 0 / 1 bytes
inline std::vector<uint8_t> as_flags(const void* v, size_t n) {
    std::vector<uint8_t> f(n);
    for (size_t i = 0; i < n; ++i)
        f[i] = static_cast<const uint8_t*>(v)[i] ? 1 : 0;
    return f;
}

// MI_OK, or the refusal of a create call on a machine without a device (in the stage's own words) or with fewer than gpu + 1
inline int check_gpu(int gpu, const char* no_device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MI_ERR_NO_DEVICE, no_device);
    if (gpu < 0 || gpu >= ndev)
        return fail(MI_ERR_INVALID, "gpu index out of range");
    return MI_OK;
}

// Events around each launch of a call: event i before launch i, the last one after the last launch.
struct LaunchTiming {
    const char* stage;  // leads the error texts
    int launches;
    bool on = false;
    Event ev[6];
    LaunchTiming(const char* stage_, int launches_) : stage(stage_), launches(launches_) {}
    void stamp(int i, hipStream_t q) {
        if (on)
            (void)hipEventRecord(ev[i], q);
    }
    int enable(int gpu, bool want) {
        if (want && !ev[0]) {
            if (hipSetDevice(gpu) != hipSuccess)
                return fail(MI_ERR_HIP, "hipSetDevice failed");
            for (int i = 0; i <= launches; ++i)
                if (hipEventCreate(ev[i].put()) != hipSuccess)
                    return fail(MI_ERR_HIP, std::string(stage) + ": hipEventCreate failed");
        }
        on = want;
        return MI_OK;
    }
    int elapsed(int gpu, float* ms) {  // ms[launches] of the last stamped call
        if (hipSetDevice(gpu) != hipSuccess || hipEventSynchronize(ev[launches]) != hipSuccess)
            return fail(MI_ERR_HIP, std::string(stage) + ": waiting for the timing events failed");
        for (int i = 0; i < launches; ++i)
            if (hipEventElapsedTime(ms + i, ev[i], ev[i + 1]) != hipSuccess)
                return fail(MI_ERR_HIP, std::string(stage) + ": hipEventElapsedTime failed");
        return MI_OK;
    }
};

// The two counts of the last call, landed through pinned memory on the caller's stream: what a download starts with.
inline bool land_counts(int gpu, hipStream_t q, uint32_t* h_count, const uint32_t* d_count, uint32_t* count) {
    if (hipSetDevice(gpu) != hipSuccess || hipMemcpyAsync(h_count, d_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, q) != hipSuccess ||
        hipStreamSynchronize(q) != hipSuccess)
        return false;
    count[0] = h_count[0];
    count[1] = h_count[1];
    return true;
}

// State and settings in or out between calls: whatever is queued on the device finishes first.
inline bool sync_copy(int gpu, void* dst, const void* src, size_t len, hipMemcpyKind kind) {
    return hipSetDevice(gpu) == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipMemcpy(dst, src, len, kind) == hipSuccess;
}

// What every post-stage handle holds.  `called`: a process_device call has been made (the survey, the finder and the probe: a
// stamped one), the precondition of last_launch_ms.
struct Stage {
    int gpu = 0;
    LaunchTiming timing;
    bool called = false;
    Stage(const char* stage, int launches) : timing(stage, launches) {}
};
// ... a stage over [rows][max_batches] blocks of audio
struct BatchStage : Stage {
    using Stage::Stage;
    int rows = 0;
    int max_batches = 0;
};
// ... whose rows the caller switches on and off
struct RowStage : BatchStage {
    using BatchStage::BatchStage;
    DevBuf<uint8_t> d_enabled;  // [rows]
};

// The bodies of the extern "C" entry points that differ between stages in nothing but the handle's type and the stage's name:
// `stage` is the string the handle gives its LaunchTiming (a NULL handle has none to ask).  Each returns MI_OK or the refusal with
// its message set.
inline int batch_geometry_ok(const char* stage, int rows, int max_batches) {
    if (rows < 1 || rows >= (1 << 20) || max_batches < 1 || static_cast<uint64_t>(rows) * static_cast<uint64_t>(max_batches) >= (1ull << 24))
        return fail(MI_ERR_INVALID, std::string(stage) + " needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24");
    return MI_OK;
}

inline int set_enabled(const char* stage, RowStage* s, const uint8_t* row_enabled) {
    if (!s || !row_enabled)
        return fail(MI_ERR_INVALID, "NULL argument");
    const std::vector<uint8_t> flags = as_flags(row_enabled, static_cast<size_t>(s->rows));
    // (a call still queued reads the rows it was made with)
    if (!sync_copy(s->gpu, s->d_enabled, flags.data(), flags.size(), hipMemcpyHostToDevice))
        return fail(MI_ERR_HIP, std::string(stage) + ": uploading the rows failed");
    return MI_OK;
}

inline int set_timing(Stage* s, int on) {
    if (!s)
        return fail(MI_ERR_INVALID, "NULL argument");
    return s->timing.enable(s->gpu, on != 0);
}

// `process_device`: the entry point's own name, e.g. "mi_pcm_process_device"
inline int last_launch_ms(Stage* s, float* ms, const char* process_device) {
    if (!s || !ms)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (!s->timing.on || !s->called)
        return fail(MI_ERR_INVALID, std::string("no timed ") + process_device + " call");
    return s->timing.elapsed(s->gpu, ms);
}

template <class H>
void destroy(H* h) {
    if (!h)
        return;
    (void)hipSetDevice(h->gpu);
    delete h;
}

// The checkpoint blob, rows x RowState, as the device array `state` of the handle holds it.
template <class H, class RowState>
size_t state_size(const H* h, DevBuf<RowState> H::*) {
    return h ? static_cast<size_t>(h->rows) * sizeof(RowState) : 0;
}

template <class H, class RowState>
int get_state(const char* stage, H* h, DevBuf<RowState> H::*state, void* buf, size_t len) {
    if (!h || !buf || len != state_size(h, state))
        return fail(MI_ERR_INVALID, std::string(stage) + " state: NULL argument or wrong length");
    if (!sync_copy(h->gpu, buf, h->*state, len, hipMemcpyDeviceToHost))
        return fail(MI_ERR_HIP, std::string(stage) + ": reading the state failed");
    return MI_OK;
}

// `malformed(rows, n)`: for a stage that checks a blob before it takes it -- NULL, or what is wrong with it in the stage's words
template <class H, class RowState, class Check = std::nullptr_t>
int set_state(const char* stage, H* h, DevBuf<RowState> H::*state, const void* buf, size_t len, Check malformed = nullptr) {
    if (!h || !buf || len != state_size(h, state))
        return fail(MI_ERR_INVALID, std::string(stage) + " state: NULL argument or wrong length");
    std::vector<RowState> rows;  // (a checked blob is looked at, and uploaded, as an aligned copy)
    if constexpr (!std::is_same<Check, std::nullptr_t>::value) {
        rows.resize(static_cast<size_t>(h->rows));
        std::memcpy(rows.data(), buf, len);
        if (const char* const why = malformed(rows.data(), rows.size()))
            return fail(MI_ERR_INVALID, std::string(stage) + " state: " + why);
        buf = rows.data();
    }
    if (!sync_copy(h->gpu, h->*state, buf, len, hipMemcpyHostToDevice))
        return fail(MI_ERR_HIP, std::string(stage) + ": writing the state failed");
    return MI_OK;
}

// whether the planes [rows][stride] share a byte over a call of nbatches batches (poststage_host.cpp)
bool planes_overlap(const float* in, size_t in_stride, const float* out, size_t out_stride, size_t rows, size_t nbatches);

// The checks of a call that reads a plane [rows][in_stride] and writes one [rows][out_stride] (voice band, limiter).  `in_noun`:
// what the stage's texts call the plane it reads.
inline int plane_call_ok(const BatchStage* s, const float* in, size_t in_stride, int nbatches, const float* out, size_t out_stride, const char* in_noun) {
    if (!s || !in || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    if (nbatches < 1 || nbatches > s->max_batches)
        return fail(MI_ERR_INVALID, "nbatches outside 1 .. max_batches");
    if (in_stride < static_cast<size_t>(nbatches) * kWaveBatch || out_stride < static_cast<size_t>(nbatches) * kWaveBatch)
        return fail(MI_ERR_INVALID, "a row stride is shorter than the call");
    if (in_stride % 4 != 0 || out_stride % 4 != 0 || !aligned(in, 16) || !aligned(out, 16))
        return fail(MI_ERR_INVALID, std::string("the ") + in_noun + " and the output must be 16-byte aligned with row strides that are multiples of 4 floats");
    if (planes_overlap(in, in_stride, out, out_stride, static_cast<size_t>(s->rows), static_cast<size_t>(nbatches)))
        return fail(MI_ERR_INVALID, std::string("the output overlaps the ") + in_noun);
    return MI_OK;
}

constexpr int kRowsPerGroup = 4;  // one wave per row, four rows per 256-thread workgroup
constexpr int kScanTile = 256;

// k_row_scan (poststage.hip), one workgroup: row_first[0 .. rows] = exclusive scan of row_count[0 .. rows - 1], count[0] = the total,
// count[1] = min(total, cap)
void launch_row_scan(hipStream_t stream, const uint32_t* row_count, int rows, uint32_t cap, uint32_t* row_first, uint32_t* count);

// One row of the transmission splitter's state (include/mi_airband.h "transmission splitter"): the checkpoint blob is an array of
// these, and txsplit.hip keeps the same array in device memory.
struct TxRowState {
    uint64_t clock;       // batches this row has handled
    uint64_t opened;      // value of clock when the open file was opened
    uint64_t last_write;  // value of clock at the last write
    uint32_t seq;         // running file number, 0 before the first file
    uint8_t open;         // fdata->f != NULL
    uint8_t active;       // output_t::active
    uint16_t zero;
};
static_assert(sizeof(TxRowState) == MI_TX_STATE_ROW_BYTES && sizeof(mi_tx_record) == 40, "the splitter's blob and record layouts are ABI");

mi_tx_cfg tx_cfg_or_default(const mi_tx_cfg* cfg);  // poststage_host.cpp

// One row of the tone finder's state (include/mi_airband.h "CTCSS tone finder"): the checkpoint blob is an array of these, and
// tones.hip keeps the same array in device memory.
struct TonesRowState {
    uint32_t count;  // samples in the running window, < window
    uint32_t seq;    // windows completed since creation / set_state
    float q1[MI_TONES_LANES], q2[MI_TONES_LANES];
};
static_assert(sizeof(TonesRowState) == MI_TONES_STATE_ROW_BYTES && sizeof(mi_tone_record) == 40 && sizeof(mi_tones_vote) == 32,
              "the tone finder's blob and record layouts are ABI");

// What both halves of the tone finder share (poststage_host.cpp).  tones_window: the window with the default filled in, or 0 with
// the refusal's message set.  tones_max_windows: the most windows one row completes in a call.  tones_coeffs: coeff[64], lanes 51 ..
// 63 zero.  tones_state_ok: every row's count < window and padding lanes all-zero bits.
uint32_t tones_window(const mi_tones_cfg* cfg);
inline uint64_t tones_max_windows(uint32_t window, uint64_t nbatches) {
    return (window - 1 + static_cast<uint64_t>(kWaveBatch) * nbatches) / window;
}
void tones_coeffs(uint32_t window, float* coeff);
bool tones_state_ok(const TonesRowState* state, size_t rows, uint32_t window);

// The PCM stage (include/mi_airband.h "PCM stage").  One row of its state: the checkpoint blob is an array of these, and pcm.hip
// keeps the same array in device memory.
struct PcmRowState {
    float x[MI_PCM_HISTORY];  // the last 62 samples of the row's last batch, oldest first
};
// The settings with the defaults filled in and what follows from them.
struct PcmGeometry {
    uint32_t rate, format;
    uint32_t samples;      // S, samples per block
    uint32_t block_bytes;  // 2 S, or 16 S / 25
};
// Taps whose value is not exactly zero, in the order the sum takes them: h[0], h[2], .. h[30], h[31], h[32], .. h[62].  pcm.hip sums
// only these: a zero tap's product is +-0, and adding it changes no finite sum that started from +0.0f.
constexpr int kPcmLiveTaps = 33;
struct PcmLiveTaps {
    float h[kPcmLiveTaps];
};
static_assert(sizeof(PcmRowState) == MI_PCM_STATE_ROW_BYTES && MI_PCM_HISTORY == MI_PCM_TAPS - 1 && sizeof(mi_pcm_cfg) == 8 &&
                  sizeof(mi_gate_block) == 8 && kWaveBatch % (2 * MI_PCM_IMA_SAMPLES) == 0 && kWaveBatch % 8 == 0,
              "the PCM stage's blob and block layouts are ABI");
constexpr int kImaSteps = 89;
extern const int kImaStepTable[kImaSteps];  // poststage_host.cpp

// pcm_geometry: MI_OK, or the refusal with its message set.  pcm_taps: h[63].  (poststage_host.cpp)
int pcm_geometry(const mi_pcm_cfg* cfg, PcmGeometry* out);
void pcm_taps(float* h);
PcmLiveTaps pcm_live_taps();

// The audio spectrum stage (include/mi_airband.h "audio spectrum stage"), what aspec.hip and its twin share (poststage_host.cpp).
// aspec_band: MI_OK with the two bins, or the refusal with its message set.  aspec_window: w[2000].  aspec_twiddles: the plan's table
// at fft_size_log 11, 1024 x {re, im}.
static_assert(sizeof(mi_aspec_record) == 32 && sizeof(mi_aspec_cfg) == 8 && sizeof(mi_aspec_notch) == 40 && MI_ASPEC_FFT == 1 << MI_ASPEC_FFT_LOG &&
                  MI_ASPEC_BINS == MI_ASPEC_FFT / 2 && kWaveBatch <= MI_ASPEC_FFT,
              "the audio spectrum stage's record layouts are ABI");
struct AspecBand {
    uint32_t lo, hi;
};
int aspec_band(const mi_aspec_cfg* cfg, AspecBand* out);
void aspec_window(float* w);
int aspec_twiddles(std::vector<float>& tw);

// The voice band stage (include/mi_airband.h "voice band stage").  One row of its state: the checkpoint blob is an array of these,
// and vband.hip keeps the same array in device memory.
struct VbandRowState {
    float x[MI_VBAND_HISTORY];  // the last 510 input samples of the row's last batch, oldest first
};
static_assert(sizeof(VbandRowState) == MI_VBAND_STATE_ROW_BYTES && MI_VBAND_HISTORY == MI_VBAND_TAPS - 1 && MI_VBAND_TAPS % 2 == 1 &&
                  sizeof(mi_vband_row) == 8 && MI_VBAND_STATE_ROW_BYTES % 8 == 0 && MI_VBAND_HISTORY <= kWaveBatch,
              "the voice band stage's blob and settings layouts are ABI");
constexpr int kVbandTapRow = 512;  // floats of one class of the device's tap table: the 511 taps and a zero that is never read

// What both halves of the voice band stage share (poststage_host.cpp).  vband_row_ok: MI_OK, or the settings' refusal with its
// message set.  vband_taps: h[511] of valid settings.  vband_classes: the rows' settings (NULL = the default row everywhere)
// checked and deduplicated in order of first appearance -- class_of[rows] and the distinct settings --, or the first refusal.
int vband_row_ok(const mi_vband_row& r);
void vband_taps(const mi_vband_row& r, float* h);
int vband_classes(const mi_vband_row* row_cfg, size_t rows, std::vector<uint32_t>& class_of, std::vector<mi_vband_row>& classes);

// The peak limiter stage (include/mi_airband.h "peak limiter stage").  One row of its state: the checkpoint blob is an array of
// these, and limit.hip keeps the same array in device memory.
struct LimitRowState {
    float x[MI_LIMIT_HISTORY];  // the last 1086 input samples of the row's last batch, oldest first
};
static_assert(sizeof(LimitRowState) == MI_LIMIT_STATE_ROW_BYTES && MI_LIMIT_HISTORY == MI_LIMIT_LOOKAHEAD + MI_LIMIT_WINDOW - 1 &&
                  (MI_LIMIT_WINDOW & (MI_LIMIT_WINDOW - 1)) == 0 && MI_LIMIT_LOOKAHEAD + 1 == 64 && sizeof(mi_limit_row) == 8 &&
                  MI_LIMIT_STATE_ROW_BYTES % 8 == 0 && MI_LIMIT_HISTORY <= kWaveBatch,
              "the limiter stage's blob and settings layouts are ABI");
// limit_row_ok: MI_OK, or the settings' refusal with its message set.  limit_rows: the rows' settings (NULL = the default row
// everywhere) checked, or the first refusal.  (poststage_host.cpp)
int limit_row_ok(const mi_limit_row& r);
int limit_rows(const mi_limit_row* row_cfg, size_t rows, std::vector<mi_limit_row>& out);

// The noise reduction stage (include/mi_airband.h "noise reduction stage").  One row of its state: the checkpoint blob is an array of
// these, and denoise.hip keeps the same array in device memory.
struct DenoiseRowState {
    float x[MI_DENOISE_FRAME];                           // the last 500 input samples of the row's last batch, oldest first
    float m[MI_DENOISE_DEPTH - 1][MI_DENOISE_BINS];      // M of the row's last seven batches, oldest first; +Inf at first
};
static_assert(sizeof(DenoiseRowState) == MI_DENOISE_STATE_ROW_BYTES && sizeof(mi_denoise_row) == 8 && MI_DENOISE_FRAME == 2 * MI_DENOISE_HOP &&
                  kWaveBatch % MI_DENOISE_HOP == 0 && MI_DENOISE_FRAME <= MI_DENOISE_FFT && MI_DENOISE_FFT == 1 << MI_DENOISE_FFT_LOG &&
                  MI_DENOISE_BINS == MI_DENOISE_FFT / 2 + 1 && MI_DENOISE_FRAME % 4 == 0,
              "the noise reduction stage's blob and settings layouts are ABI");
// A row's settings as the kernels take them.
struct DenoiseGains {
    float g_min;  // (float)10^(-reduction_db / 20)
    float over;
};
// What both halves of the noise reduction stage share (poststage_host.cpp).  denoise_rows: the rows' settings (NULL = the default row
// everywhere) checked and converted, or the first refusal with its message set.  denoise_window: w[500].  spec_twiddles: the plan's
// twiddle table at fft_size_log log2n, 2^(log2n - 1) x {re, im}.  denoise_fresh: a blob's first bytes, zeros and +Inf.
int denoise_rows(const mi_denoise_row* row_cfg, size_t rows, std::vector<DenoiseGains>& out);
void denoise_window(float* w);
int spec_twiddles(int log2n, std::vector<float>& tw);
void denoise_fresh(DenoiseRowState* state, size_t rows);

// The SELCAL decoder stage (include/mi_airband.h "SELCAL decoder stage").  One row of its state: the checkpoint blob is an array of
// these, and selcal.hip keeps the same array in device memory.
struct SelcalRowState {
    float x[MI_SELCAL_HISTORY];  // the last 1002 input samples of the row's last batch, oldest first (the two oldest are never read)
    uint32_t window;             // windows seen since creation / set_state
    uint32_t seq;                // codes emitted
    uint32_t phase;              // MI_SELCAL_IDLE .. MI_SELCAL_DONE
    uint32_t pair1, pair2;       // lo | hi << 8, MI_SELCAL_NONE where the phase has none
    uint32_t run1, run2, gap;
    uint32_t first_window;
    uint32_t zero;
};
static_assert(sizeof(SelcalRowState) == MI_SELCAL_STATE_ROW_BYTES && offsetof(SelcalRowState, window) == MI_SELCAL_HISTORY * 4 &&
                  sizeof(mi_selcal_window_record) == 24 && sizeof(mi_selcal_code) == 32 && sizeof(mi_selcal_cfg) == 168 &&
                  (MI_SELCAL_HISTORY + 2) % 4 == 0 && MI_SELCAL_HISTORY >= MI_SELCAL_HOP && MI_SELCAL_WINDOW == kWaveBatch &&
                  MI_SELCAL_WINDOW == 2 * MI_SELCAL_HOP && MI_SELCAL_STATE_ROW_BYTES % 8 == 0,
              "the SELCAL stage's blob, record and settings layouts are ABI");
// The settings with every default filled in and what follows from them, as both halves take them.
struct SelcalPlan {
    uint32_t ntones;
    float freq[MI_SELCAL_MAX_TONES], coeff[MI_SELCAL_MAX_TONES];
    char letter[MI_SELCAL_MAX_TONES];
    float min_energy, tc, max_twist, min_separation;  // tc = min_tonality * c
    uint32_t min_run, max_run, max_gap;
    mi_selcal_cfg filled;  // the settings as the caller would have written them
    float c;
};
// The decoder's part of a row's state, as the walk carries it in registers.
struct SelcalDecoder {
    uint32_t phase, pair1, pair2, run1, run2, gap, first_window;
};
// One window through the decoder table of the header: `pair` is what the window named (MI_SELCAL_NONE: none), n its number.
// True when the window emits a code (d then holds what the record takes).  Host and device run this text.
__host__ __device__ inline bool selcal_step(SelcalDecoder& d, const uint32_t pair, const uint32_t n, const uint32_t min_run, const uint32_t max_run,
                                            const uint32_t max_gap) {
    const bool some = pair != MI_SELCAL_NONE;
    bool from_idle = false;
    switch (d.phase) {
    case MI_SELCAL_FIRST:
        if (some && pair == d.pair1) {
            if (++d.run1 > max_run) {
                d.phase = MI_SELCAL_OVER;
                d.run1 = max_run + 1;
            }
        } else if (d.run1 >= min_run) {
            if (some) {
                d.phase = MI_SELCAL_SECOND;
                d.pair2 = pair;
                d.run2 = 1;
            } else {
                d.phase = MI_SELCAL_GAP;
                d.gap = 1;
            }
        } else {
            from_idle = true;  // (a pair Q restarts FIRST, no pair ends in IDLE)
        }
        break;
    case MI_SELCAL_OVER:
        from_idle = !(some && pair == d.pair1);
        break;
    case MI_SELCAL_GAP:
        if (!some) {
            from_idle = ++d.gap > max_gap;
        } else if (pair == d.pair1) {
            d.run1 += d.gap + 1;
            d.gap = 0;
            d.phase = MI_SELCAL_FIRST;
            if (d.run1 > max_run) {
                d.phase = MI_SELCAL_OVER;
                d.run1 = max_run + 1;
            }
        } else {
            d.phase = MI_SELCAL_SECOND;
            d.pair2 = pair;
            d.run2 = 1;
        }
        break;
    case MI_SELCAL_SECOND:
        if (some && pair == d.pair2) {
            if (++d.run2 == min_run) {
                d.phase = MI_SELCAL_DONE;
                return true;
            }
        } else {
            from_idle = true;
        }
        break;
    case MI_SELCAL_DONE:
        from_idle = !(some && pair == d.pair2);
        break;
    default:
        from_idle = true;
        break;
    }
    if (from_idle) {
        d = SelcalDecoder{MI_SELCAL_IDLE, MI_SELCAL_NONE, MI_SELCAL_NONE, 0u, 0u, 0u, 0u};
        if (some) {
            d.phase = MI_SELCAL_FIRST;
            d.pair1 = pair;
            d.run1 = 1;
            d.first_window = n;
        }
    }
    return false;
}
// the most codes one row can emit in a call: the first needs one window of the call, each further one 2 * min_run
inline uint32_t selcal_max_codes(uint32_t min_run, uint64_t nbatches) {
    return static_cast<uint32_t>(1 + (2 * nbatches - 1) / (2ull * min_run));
}
// What both halves of the SELCAL stage share (poststage_host.cpp).  selcal_plan: MI_OK with the plan, or the settings' refusal with
// its message set.  selcal_window: w[2000].  selcal_state_ok: NULL, or what is impossible about a blob's decoder state.
int selcal_plan(const mi_selcal_cfg* cfg, SelcalPlan* out);
void selcal_window(float* w);
const char* selcal_state_ok(const SelcalRowState* state, size_t rows, const SelcalPlan& plan);

// The ACARS decoder stage (include/mi_airband.h "ACARS decoder stage").  One row of its state: the checkpoint blob is an array of
// these, and acars.hip keeps the same array in device memory.
struct AcarsRowState {
    float x[MI_ACARS_HISTORY];              // the last 6 input samples of the row's last batch, oldest first
    uint32_t batch;                         // batches seen since creation / set_state
    uint32_t phase;                         // MI_ACARS_IDLE / MI_ACARS_FRAME
    uint64_t hist[MI_ACARS_HYPOTHESES];     // per hypothesis the last 38 change bits, the newest in bit 0
    uint32_t u, prev, nbits, cur, nbytes, tail, crc, parity_errors, start_batch, start_third, tau_sync, mismatches, end, zero;
    uint8_t bytes[MI_ACARS_RAW_BYTES];
};
static_assert(sizeof(AcarsRowState) == MI_ACARS_STATE_ROW_BYTES && offsetof(AcarsRowState, hist) == 32 && offsetof(AcarsRowState, u) == 192 &&
                  offsetof(AcarsRowState, bytes) == 248 && sizeof(mi_acars_frame) == 272 && offsetof(mi_acars_frame, bytes) == 24 &&
                  sizeof(mi_acars_cfg) == 16 && sizeof(mi_acars_text) == 248 && (MI_ACARS_HISTORY + 2) % 4 == 0 &&
                  MI_ACARS_MAX_BYTES + 2 <= MI_ACARS_RAW_BYTES && MI_ACARS_RAW_BYTES % 8 == 0 && 20 * MI_ACARS_BITS == 3 * kWaveBatch &&
                  MI_ACARS_BIT_WORDS * 32 >= MI_ACARS_BITS,
              "the ACARS stage's blob, record and settings layouts are ABI");
// The settings with every default filled in, as both halves take them.
struct AcarsPlan {
    uint32_t sync_errors;  // the number itself, 0 .. 4
    uint32_t keep_bad, hold_timing;
    float min_quality;
    mi_acars_cfg filled;   // the settings as the caller would have written them
};
// The walker's part of a row's state, as the walk carries it in registers; the bytes so far stay in memory beside it.
struct AcarsWalker {
    uint32_t phase, u, prev, nbits, cur, nbytes, tail, crc, parity_errors, start_batch, start_third, tau_sync, mismatches, end;
};
constexpr uint64_t kAcarsMask39 = (1ull << MI_ACARS_SYNC_BITS) - 1, kAcarsMask38 = kAcarsMask39 >> 1;
// the 39 change bits inside '+' '*' SYN SYN SOH, sent least significant bit first, the newest in bit 0
constexpr uint64_t acars_sync_pattern() {
    const uint8_t s[5] = {0xAB, 0x2A, 0x16, 0x16, 0x01};
    uint64_t p = 0;
    int prev = s[0] & 1;
    for (int i = 1; i < 40; ++i) {
        const int b = (s[i / 8] >> (i % 8)) & 1;
        p = p << 1 | static_cast<uint64_t>(b ^ prev);
        prev = b;
    }
    return p;
}
constexpr uint64_t kAcarsSync = acars_sync_pattern();
// the most frames one row can end in a call: the first may end in the call's first slot, each further one takes 39 slots of sync
// and at least 119 of its 120 bits (a timing move can take two in one slot)
inline uint32_t acars_max_frames(uint64_t nbatches) {
    return static_cast<uint32_t>(1 + MI_ACARS_BITS * nbatches / 119);
}
__host__ __device__ inline uint32_t acars_crc_byte(uint32_t crc, const uint32_t byte) {
    crc ^= byte;
    for (int i = 0; i < 8; ++i)
        crc = crc & 1u ? crc >> 1 ^ 0x8408u : crc >> 1;
    return crc;
}
// Slot j of hypothesis tau over what is staged for a block -- s[kLead + n] is the block's sample n, kLead = MI_ACARS_HISTORY + 2 --:
// the change bit, and the quality into *q.  Host and device run this text.
__host__ __device__ inline uint32_t acars_bit(const float* s, const float* h1, const float* h2, const int tau, const int j, float* q) {
    const int t0 = tau + 20 * (j - (tau > 0));           // -19 .. 5980
    const int n0 = (t0 + 23) / 3 - 7;                    // ceil(t0 / 3)
    const int rho0 = 3 * n0 - t0;                        // 0 .. 2
    const float* const x = s + (MI_ACARS_HISTORY + 2) + n0;
    float r1 = x[0] * h1[rho0], r2 = x[0] * h2[rho0];
#pragma unroll
    for (int i = 1; i < 6; ++i) {
        r1 = r1 + x[i] * h1[rho0 + 3 * i];
        r2 = r2 + x[i] * h2[rho0 + 3 * i];
    }
    if (rho0 <= 1) {
        r1 = r1 + x[6] * h1[rho0 + 18];
        r2 = r2 + x[6] * h2[rho0 + 18];
    }
    const float a1 = r1 * r1, a2 = r2 * r2;
    *q = a1 > a2 ? a1 : a2;
    return fabsf(r1) >= fabsf(r2) ? 1u : 0u;
}
// What one change bit on the walker's hypothesis does to a frame.
enum { kAcarsNone = 0, kAcarsDone = 1, kAcarsDropped = 2 };
// One change bit c through the walker of the header, the frame's bytes so far at `bytes` (MI_ACARS_RAW_BYTES of them).  kAcarsDone:
// the frame is whole -- w and bytes hold what the record takes, w.crc == 0 being crc_ok -- and the caller calls acars_idle behind the
// record.  kAcarsDropped: no ETX / ETB in 240 bytes; the row is idle.  Host and device run this text.
__host__ __device__ inline void acars_idle(AcarsWalker& w, uint8_t* bytes) {
    for (uint32_t i = 0; i < w.nbytes + w.tail && i < MI_ACARS_RAW_BYTES; ++i)
        bytes[i] = 0;
    w = AcarsWalker{};
}
__host__ __device__ inline int acars_step(AcarsWalker& w, uint8_t* bytes, const uint32_t c) {
    w.prev ^= c;
    w.cur |= w.prev << w.nbits;
    if (++w.nbits < 8)
        return kAcarsNone;
    const uint32_t byte = w.cur;
    w.cur = 0;
    w.nbits = 0;
    w.crc = acars_crc_byte(w.crc, byte);
    if (w.tail) {
        bytes[w.nbytes + w.tail - 1] = static_cast<uint8_t>(byte);
        return ++w.tail == 3 ? kAcarsDone : kAcarsNone;
    }
    bytes[w.nbytes++] = static_cast<uint8_t>(byte);
    uint32_t ones = byte;
    ones ^= ones >> 4;
    ones ^= ones >> 2;
    ones ^= ones >> 1;
    w.parity_errors += (ones & 1u) ^ 1u;
    const uint32_t ch = byte & 0x7Fu;
    if (w.nbytes > MI_ACARS_HEAD_BYTES && (ch == 0x03u || ch == 0x17u)) {
        w.end = ch;
        w.tail = 1;
    } else if (w.nbytes == MI_ACARS_MAX_BYTES) {
        acars_idle(w, bytes);
        return kAcarsDropped;
    }
    return kAcarsNone;
}
// The hypothesis a sync opens the frame on: mism[tau] = the mismatches of tau's 39 bits, q[tau] = Q of the slot's batch; -1: no hit.
__host__ __device__ inline int acars_pick(const uint32_t* mism, const float* q, const uint32_t sync_errors, const float min_quality) {
    int best = -1;
    for (int t = 0; t < MI_ACARS_HYPOTHESES; ++t) {
        if (mism[t] > sync_errors || !(q[t] >= min_quality))
            continue;
        if (best < 0 || mism[t] < mism[best] || (mism[t] == mism[best] && q[t] > q[best]))
            best = t;
    }
    return best;
}
// A frame opens on hypothesis u at a hit in slot j of the row's batch number `batch`.
__host__ __device__ inline void acars_open(AcarsWalker& w, const int u, const uint32_t mismatches, const uint32_t batch, const int j) {
    w = AcarsWalker{};
    w.phase = MI_ACARS_FRAME;
    w.u = w.tau_sync = static_cast<uint32_t>(u);
    w.mismatches = mismatches;
    const int t = u + 20 * (j + 1 - (u > 0));  // where slot j + 1 begins
    w.start_batch = t >= 3 * kWaveBatch ? batch + 1 : batch;
    w.start_third = static_cast<uint32_t>(t >= 3 * kWaveBatch ? t - 3 * kWaveBatch : t);
}
// The timing move at a batch's first slot inside a frame, from the new batch's Q.
enum { kAcarsInStep = 0, kAcarsSkip = 1, kAcarsReplay = 2 };
__host__ __device__ inline int acars_retime(AcarsWalker& w, const float* q) {
    const uint32_t u = w.u, um = (u + 19) % 20, up = (u + 1) % 20;
    uint32_t v = u;
    if (q[um] > q[v])
        v = um;
    if (q[up] > q[v])
        v = up;
    w.u = v;
    return u == 0 && v == 1 ? kAcarsSkip : u == 1 && v == 0 ? kAcarsReplay : kAcarsInStep;
}
// What both halves of the ACARS stage share (poststage_host.cpp).  acars_plan: MI_OK with the plan, or the settings' refusal with its
// message set.  acars_templates: h1[20], h2[20].  acars_state_ok: NULL, or what is impossible about a blob.
int acars_plan(const mi_acars_cfg* cfg, AcarsPlan* out);
void acars_templates(float* h1, float* h2);
const char* acars_state_ok(const AcarsRowState* state, size_t rows);

// The SAME decoder stage (include/mi_airband.h "SAME decoder stage").  The walker's and the assembler's part of a row's state, as the
// walk carries it in registers; the running burst's bytes and the two stored bursts stay in memory beside it.
struct SameWalker {
    uint32_t phase, u, kind, nbits, cur, nbytes, nbad, plus, dashes, deaf, start_batch, start_unit;  // the burst's
    uint32_t an, akind, alen0, alen1, atrunc0, atrunc1, aidle, astart_batch, astart_unit;            // the assembler's
};
constexpr int kSameWalkerWords = sizeof(SameWalker) / 4;
// One row of the state: the checkpoint blob is an array of these, and same.hip keeps the same array in device memory.
struct SameRowState {
    float x[MI_SAME_HISTORY];              // the last 30 input samples of the row's last batch, oldest first
    uint32_t batch;                        // batches seen since creation / set_state
    uint32_t grid;                         // (50 000 * batches seen) mod 768
    uint64_t hist[MI_SAME_HYPOTHESES];     // per hypothesis the last 64 bits, the newest in bit 0
    SameWalker w;
    uint32_t zero;
    uint8_t bytes[3][MI_SAME_RAW_BYTES];   // the running burst, then the assembler's two
};
static_assert(sizeof(SameRowState) == MI_SAME_STATE_ROW_BYTES && offsetof(SameRowState, hist) == 128 && offsetof(SameRowState, w) == 256 &&
                  offsetof(SameRowState, bytes) == 344 && kSameWalkerWords == 21 && sizeof(mi_same_message) == 304 &&
                  offsetof(mi_same_message, bytes) == 32 && sizeof(mi_same_cfg) == 24 && sizeof(mi_same_text) == 256 &&
                  (MI_SAME_HISTORY + 2) % 4 == 0 && MI_SAME_MAX_BYTES <= MI_SAME_RAW_BYTES && MI_SAME_RAW_BYTES % 8 == 0 &&
                  25 * kWaveBatch == MI_SAME_BATCH_UNITS && MI_SAME_BIT_WORDS * 32 >= MI_SAME_MAX_BITS + 32,
              "the SAME stage's blob, record and settings layouts are ABI");
// The settings with every default filled in, as both halves take them.
struct SamePlan {
    uint32_t sync_errors;  // the number itself, 0 .. 4
    uint32_t max_bad, gap_batches, hold_timing;
    float min_quality, space_gain;
    mi_same_cfg filled;    // the settings as the caller would have written them
};
constexpr int kSameTemplate = MI_SAME_BIT_UNITS;  // entries of one template
constexpr uint64_t same_pattern(const char c0, const char c1, const char c2, const char c3) {
    const uint8_t s[8] = {0xAB, 0xAB, 0xAB, 0xAB, static_cast<uint8_t>(c0), static_cast<uint8_t>(c1), static_cast<uint8_t>(c2), static_cast<uint8_t>(c3)};
    uint64_t p = 0;
    for (int i = 0; i < 64; ++i)
        p = p << 1 | static_cast<uint64_t>((s[i / 8] >> (i % 8)) & 1);
    return p;
}
constexpr uint64_t kSameHeaderSync = same_pattern('Z', 'C', 'Z', 'C'), kSameEomSync = same_pattern('N', 'N', 'N', 'N');
inline uint32_t same_max_messages(uint64_t nbatches) {
    return static_cast<uint32_t>(2 * (2 + 66 * nbatches / 65) + 1);
}
// The grid of a batch whose state field is `grid`: the hypotheses below same_ahead had their bit of the batch's first index in the
// batch before; same_first is where hypothesis tau's first bit of the batch begins, -767 .. 0; same_count how many it has.
__host__ __device__ inline int same_ahead(const uint32_t grid) {
    const int a = static_cast<int>(grid) / 48 + 1;
    return a == MI_SAME_HYPOTHESES ? 0 : a;
}
__host__ __device__ inline int same_first(const uint32_t grid, const int tau) {
    const int c = (48 * tau + MI_SAME_BIT_UNITS - static_cast<int>(grid)) % MI_SAME_BIT_UNITS;
    return c ? c - MI_SAME_BIT_UNITS : 0;
}
__host__ __device__ inline int same_count(const int r0) {
    return (MI_SAME_BATCH_UNITS - MI_SAME_BIT_UNITS - r0) / MI_SAME_BIT_UNITS + 1;
}
// The bit that begins at unit r (-767 .. 49 232) of the block staged at s -- s[32 + n] is the block's sample n --, T the four
// templates: the bit, and its quality into *q.  Host and device run this text.
__host__ __device__ inline uint32_t same_bit(const float* s, const float* T, const int r, const float space_gain, float* q) {
    const int n0 = (r + 824) / 25 - 32;  // ceil(r / 25)
    int rho = 25 * n0 - r;               // 0 .. 24
    const bool more = rho + 750 < MI_SAME_BIT_UNITS;
    const float* const x = s + (MI_SAME_HISTORY + 2) + n0;
    float s0 = x[0] * T[rho], s1 = x[0] * T[kSameTemplate + rho], s2 = x[0] * T[2 * kSameTemplate + rho], s3 = x[0] * T[3 * kSameTemplate + rho];
    for (int i = 1; i < 30; ++i) {
        rho += 25;
        s0 = s0 + x[i] * T[rho];
        s1 = s1 + x[i] * T[kSameTemplate + rho];
        s2 = s2 + x[i] * T[2 * kSameTemplate + rho];
        s3 = s3 + x[i] * T[3 * kSameTemplate + rho];
    }
    if (more) {
        rho += 25;
        s0 = s0 + x[30] * T[rho];
        s1 = s1 + x[30] * T[kSameTemplate + rho];
        s2 = s2 + x[30] * T[2 * kSameTemplate + rho];
        s3 = s3 + x[30] * T[3 * kSameTemplate + rho];
    }
    const float pm = s0 * s0 + s1 * s1, ps = s2 * s2 + s3 * s3;
    *q = pm > ps ? pm : ps;
    return pm >= space_gain * ps ? 1u : 0u;
}
// mk[tau] = mismatches | kind << 8 of tau's 64 bits against the nearer pattern
__host__ __device__ inline uint32_t same_mismatch(const uint64_t hist) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t mh = static_cast<uint32_t>(__popcll(hist ^ kSameHeaderSync)), me = static_cast<uint32_t>(__popcll(hist ^ kSameEomSync));
#else
    const uint32_t mh = static_cast<uint32_t>(__builtin_popcountll(hist ^ kSameHeaderSync)), me = static_cast<uint32_t>(__builtin_popcountll(hist ^ kSameEomSync));
#endif
    return me < mh ? me | MI_SAME_EOM << 8 : mh;
}
// The hypothesis a sync opens the burst on; -1: no hit.
__host__ __device__ inline int same_pick(const uint32_t* mk, const float* q, const uint32_t sync_errors, const float min_quality) {
    int best = -1;
    for (int t = 0; t < MI_SAME_HYPOTHESES; ++t) {
        const uint32_t m = mk[t] & 0xFFu;
        if (m > sync_errors || !(q[t] >= min_quality))
            continue;
        if (best < 0 || m < (mk[best] & 0xFFu) || (m == (mk[best] & 0xFFu) && q[t] > q[best]))
            best = t;
    }
    return best;
}
// Whether n bytes of a message of `kind` match the grammar of the header.
__host__ __device__ inline uint32_t same_fields_ok(const uint8_t* b, const uint32_t n, const uint32_t kind) {
    const auto cap = [](uint8_t c) { return c >= 'A' && c <= 'Z'; };
    const auto dig = [](uint8_t c) { return c >= '0' && c <= '9'; };
    if (kind == MI_SAME_EOM)
        return n == 4 && b[0] == 'N' && b[1] == 'N' && b[2] == 'N' && b[3] == 'N';
    // "ZCZC-ORG-EEE" 12, a location 7, "+TTTT-JJJHHMM-LLLLLLLL-" 23
    if (n < 12 + 7 + 23 || (n - 12 - 23) % 7 != 0 || (n - 12 - 23) / 7 > 31)
        return 0;
    if (b[0] != 'Z' || b[1] != 'C' || b[2] != 'Z' || b[3] != 'C' || b[4] != '-' || b[8] != '-')
        return 0;
    for (int i = 0; i < 3; ++i)
        if (!cap(b[5 + i]) || !cap(b[9 + i]))
            return 0;
    uint32_t i = 12;
    for (; i < n - 23; i += 7) {
        if (b[i] != '-')
            return 0;
        for (int d = 1; d < 7; ++d)
            if (!dig(b[i + d]))
                return 0;
    }
    if (b[i] != '+' || b[i + 5] != '-' || b[i + 13] != '-' || b[i + 22] != '-')
        return 0;
    for (int d = 0; d < 4; ++d)
        if (!dig(b[i + 1 + d]))
            return 0;
    for (int d = 0; d < 7; ++d)
        if (!dig(b[i + 6 + d]))
            return 0;
    for (int d = 0; d < 8; ++d)
        if (b[i + 14 + d] < 0x20 || b[i + 14 + d] > 0x7E || b[i + 14 + d] == '-')
            return 0;
    return 1;
}
// The assembler's n bursts become the record *m, closed in the call's batch b; the third burst, where n = 3, is the running one
// (len2 bytes, flag trunc2).  The assembler is empty behind it.  bytes: the row's [3][272].
__host__ __device__ inline void same_close(SameWalker& w, uint8_t* bytes, const uint32_t row, const uint32_t b, const uint32_t n, const uint32_t len2,
                                           const uint32_t trunc2, mi_same_message* m) {
    uint8_t *const b0 = bytes + MI_SAME_RAW_BYTES, *const b1 = bytes + 2 * MI_SAME_RAW_BYTES;
    const uint8_t* const b2 = bytes;
    uint32_t len = w.alen0, trunc = w.atrunc0, agree = 0;
    if (n == 3) {
        const uint32_t lo = w.alen0 < w.alen1 ? w.alen0 : w.alen1, hi = w.alen0 < w.alen1 ? w.alen1 : w.alen0;
        len = len2 < lo ? lo : len2 > hi ? hi : len2;  // the median
        trunc = w.atrunc0 + w.atrunc1 + trunc2 >= 2;
    }
    for (uint32_t i = 0; i < MI_SAME_RAW_BYTES; ++i) {
        uint8_t v = 0;
        if (i < len) {
            const uint8_t a = b0[i], c = b1[i], d = b2[i];
            v = n == 3 ? static_cast<uint8_t>((a & c) | (a & d) | (c & d)) : a;
            agree += n == 1 || (a == c && (n == 2 || c == d));
        }
        m->bytes[i] = v;
    }
    m->row = row;
    m->kind = w.akind;
    m->batch = w.astart_batch;
    m->unit = w.astart_unit;
    m->end_batch = b;
    m->nbursts = static_cast<uint8_t>(n);
    m->voted = n == 3;
    m->truncated = static_cast<uint8_t>(trunc);
    m->nbytes = static_cast<uint16_t>(len);
    m->agree = static_cast<uint16_t>(agree);
    m->zero = 0;
    m->fields_ok = static_cast<uint8_t>(same_fields_ok(m->bytes, len, w.akind));
    for (uint32_t i = 0; i < w.alen0; ++i)
        b0[i] = 0;
    for (uint32_t i = 0; i < w.alen1; ++i)
        b1[i] = 0;
    w.an = w.akind = w.alen0 = w.alen1 = w.atrunc0 = w.atrunc1 = w.aidle = w.astart_batch = w.astart_unit = 0;
}
// The running burst ends (trunc: as truncated) in the call's batch b: it goes to the assembler, the row is idle and deaf.  True when
// that closed a message into *m.
__host__ __device__ inline bool same_burst_end(SameWalker& w, uint8_t* bytes, const uint32_t trunc, const uint32_t row, const uint32_t b, mi_same_message* m) {
    bool closed = false;
    if (w.an == 0) {
        w.akind = w.kind;
        w.astart_batch = w.start_batch;
        w.astart_unit = w.start_unit;
    }
    if (w.an == 2) {
        same_close(w, bytes, row, b, 3, w.nbytes, trunc, m);
        closed = true;
    } else {
        uint8_t* const dst = bytes + (1 + w.an) * MI_SAME_RAW_BYTES;
        for (uint32_t i = 0; i < w.nbytes; ++i)
            dst[i] = bytes[i];
        (w.an ? w.alen1 : w.alen0) = w.nbytes;
        (w.an ? w.atrunc1 : w.atrunc0) = trunc;
        ++w.an;
        w.aidle = 0;
    }
    for (uint32_t i = 0; i < w.nbytes; ++i)
        bytes[i] = 0;
    w.phase = MI_SAME_IDLE;
    w.u = w.kind = w.nbits = w.cur = w.nbytes = w.nbad = w.plus = w.dashes = w.start_batch = w.start_unit = 0;
    w.deaf = MI_SAME_DEAF;
    return closed;
}
// A burst of `kind` opens on hypothesis u at a hit on the bit that begins at unit r of the row's batch number `batch`, the call's b.
// True when that closed a message of the other kind into *m.  (The caller ends an EOM burst at once.)
__host__ __device__ inline bool same_open(SameWalker& w, uint8_t* bytes, const int u, const uint32_t kind, const uint32_t batch, const int r, const uint32_t row,
                                          const uint32_t b, mi_same_message* m) {
    bool closed = false;
    if (w.an && w.akind != kind) {
        same_close(w, bytes, row, b, w.an, 0, 0, m);
        closed = true;
    }
    w.phase = MI_SAME_BURST;
    w.u = static_cast<uint32_t>(u);
    w.kind = kind;
    w.nbits = w.cur = w.nbad = w.plus = w.dashes = w.deaf = 0;
    w.nbytes = 4;
    bytes[0] = bytes[2] = kind == MI_SAME_EOM ? 'N' : 'Z';
    bytes[1] = bytes[3] = kind == MI_SAME_EOM ? 'N' : 'C';
    const int zs = r - 31 * MI_SAME_BIT_UNITS;  // the hit's bit is the pattern's last: 'Z' / 'N' began 31 bits before it
    w.start_batch = zs < 0 ? batch - 1u : batch;
    w.start_unit = static_cast<uint32_t>(zs < 0 ? zs + MI_SAME_BATCH_UNITS : zs);
    return closed;
}
// One bit c of the chosen hypothesis through a ZCZC burst.  True when the burst ends, *trunc saying how.
__host__ __device__ inline bool same_step(SameWalker& w, uint8_t* bytes, const uint32_t c, const uint32_t max_bad, uint32_t* trunc) {
    w.cur |= c << w.nbits;
    if (++w.nbits < 8)
        return false;
    const uint32_t byte = w.cur;
    w.cur = 0;
    w.nbits = 0;
    bytes[w.nbytes++] = static_cast<uint8_t>(byte);
    if ((byte & 0x80u) || byte < 0x20u) {
        if (++w.nbad == max_bad) {
            for (uint32_t i = 0; i < max_bad; ++i)
                bytes[--w.nbytes] = 0;
            *trunc = 1;
            return true;
        }
    } else {
        w.nbad = 0;
        if (!w.plus) {
            w.plus = byte == '+';
        } else if (byte == '-' && ++w.dashes == 3) {
            *trunc = 0;
            return true;
        }
    }
    if (w.nbytes == MI_SAME_MAX_BYTES) {
        *trunc = 1;
        return true;
    }
    return false;
}
// The gap rule at a batch's first index.  True when it closed a message into *m.
__host__ __device__ inline bool same_gap(SameWalker& w, uint8_t* bytes, const uint32_t gap_batches, const uint32_t row, const uint32_t b, mi_same_message* m) {
    if (w.phase != MI_SAME_IDLE || !w.an || ++w.aidle < gap_batches)
        return false;
    same_close(w, bytes, row, b, w.an, 0, 0, m);
    return true;
}
// The timing move at a batch's first index inside a burst, from the new batch's Q.
enum { kSameInStep = 0, kSameSkip = 1, kSameReplay = 2 };
__host__ __device__ inline int same_retime(SameWalker& w, const float* q) {
    const uint32_t u = w.u, um = (u + 15) % 16, up = (u + 1) % 16;
    uint32_t v = u;
    if (q[um] > q[v])
        v = um;
    if (q[up] > q[v])
        v = up;
    w.u = v;
    return u == 15 && v == 0 ? kSameSkip : u == 0 && v == 15 ? kSameReplay : kSameInStep;
}
// What both halves of the SAME stage share (poststage_host.cpp).  same_plan: MI_OK with the plan, or the settings' refusal with its
// message set.  same_templates: T[4][768].  same_state_ok: NULL, or what is impossible about a blob.
int same_plan(const mi_same_cfg* cfg, SamePlan* out);
void same_templates(float* T);
const char* same_state_ok(const SameRowState* state, size_t rows, const SamePlan& plan);

// The ELT detector stage (include/mi_airband.h "ELT detector stage").  One row of its state: the checkpoint blob is an array of these,
// and elt.hip keeps the same array in device memory.
struct EltRowState {
    float x[MI_ELT_HISTORY];  // the last 178 input samples of the row's last batch, oldest first (the two oldest are never read)
    uint32_t frame;           // frames seen since creation / set_state
    uint32_t seq;             // events emitted
    uint32_t open, start, first_bin, last_bin, last_frame, dir, drops;       // the segment
    uint32_t count, chain_dir, chain_first, last_end, alarmed, bin_from, bin_to;  // the chain
};
static_assert(sizeof(EltRowState) == MI_ELT_STATE_ROW_BYTES && offsetof(EltRowState, frame) == MI_ELT_HISTORY * 4 && sizeof(mi_elt_frame_record) == 16 &&
                  sizeof(mi_elt_event) == 32 && sizeof(mi_elt_cfg) == 48 && (MI_ELT_HISTORY + 2) % 4 == 0 &&
                  MI_ELT_HISTORY >= MI_ELT_FRAME - MI_ELT_HOP && MI_ELT_FRAMES * MI_ELT_HOP == kWaveBatch && MI_ELT_STATE_ROW_BYTES % 8 == 0 &&
                  MI_ELT_BIN0 + MI_ELT_BINS - 1 < MI_ELT_FRAME / 2,
              "the ELT stage's blob, record and settings layouts are ABI");
// The settings with every default filled in and what follows from them, as both halves take them.
struct EltPlan {
    float min_energy, tc;  // tc = min_tonality * c
    uint32_t band_lo, band_hi, min_span, min_len, max_len, max_step, max_drop, max_gap, min_sweeps;
    float coeff[MI_ELT_BINS];
    mi_elt_cfg filled;  // the settings as the caller would have written them
    float c;
};
// What the walker is told of the settings.
struct EltRules {
    uint32_t min_span, min_len, max_len, max_step, max_drop, max_gap, min_sweeps;
};
// The walker's part of a row's state, as the walk carries it in registers.
struct EltWalker {
    uint32_t open, start, first_bin, last_bin, last_frame, dir, drops, count, chain_dir, chain_first, last_end, alarmed, bin_from, bin_to;
};
// One frame through the walker of the header: b is the frame's decision (MI_ELT_NONE8: none), f its number.  emit(kind) is called for
// every record the frame emits, in order, while w holds what the record takes.  Host and device run this text.
template <class Emit>
__host__ __device__ inline void elt_step(EltWalker& w, const EltRules& r, const uint32_t b, const uint32_t f, Emit&& emit) {
    bool close = false, reopen = false;
    if (b != MI_ELT_NONE8) {
        if (!w.open) {
            reopen = true;
        } else {
            const uint32_t up = b > w.last_bin ? b - w.last_bin : 0u, down = w.last_bin > b ? w.last_bin - b : 0u;
            const uint32_t sd = up ? MI_ELT_UP : down ? MI_ELT_DOWN : 0u;
            if (up + down <= r.max_step * (1u + w.drops) && (sd == 0u || w.dir == 0u || sd == w.dir)) {
                if (w.dir == 0u)
                    w.dir = sd;
                w.last_bin = b;
                w.last_frame = f;
                w.drops = 0u;
            } else {
                close = reopen = true;
            }
        }
    } else if (w.open) {
        close = ++w.drops > r.max_drop;
    }
    if (close) {
        const uint32_t len = w.last_frame - w.start + 1u;
        const uint32_t span = w.first_bin > w.last_bin ? w.first_bin - w.last_bin : w.last_bin - w.first_bin;
        if (w.dir != 0u && span >= r.min_span && len >= r.min_len && len <= r.max_len) {
            if (w.count > 0u && w.start - w.last_end <= r.max_gap && w.dir == w.chain_dir) {
                ++w.count;
            } else {
                if (w.alarmed) {  // a chain begins while an alarmed one stands: that one ends here
                    emit(MI_ELT_END);
                    w.alarmed = 0u;
                }
                w.count = 1u;
                w.chain_first = w.start;
                w.chain_dir = w.dir;
            }
            w.last_end = w.last_frame;
            w.bin_from = w.first_bin;
            w.bin_to = w.last_bin;
            if (!w.alarmed && w.count >= r.min_sweeps) {
                w.alarmed = 1u;
                emit(MI_ELT_ONSET);
            }
        }
        w.open = w.start = w.first_bin = w.last_bin = w.last_frame = w.dir = w.drops = 0u;
    }
    if (reopen) {
        w.open = 1u;
        w.start = w.last_frame = f;
        w.first_bin = w.last_bin = b;
        w.dir = w.drops = 0u;
    }
    if (w.count > 0u) {
        const bool alive = f - w.last_end <= r.max_gap || (w.open && w.start - w.last_end <= r.max_gap && f - w.start + 1u <= r.max_len);
        if (!alive) {
            if (w.alarmed)
                emit(MI_ELT_END);
            w.count = w.chain_dir = w.chain_first = w.last_end = w.alarmed = w.bin_from = w.bin_to = 0u;
        }
    }
}
// an event record's words as both halves write them: {row, seq, kind | dir << 8 | bin_from << 16 | bin_to << 24, frame}, {first_frame,
// last_end, sweeps, batch}
__host__ __device__ inline uint32_t elt_event_word2(const EltWalker& w, const uint32_t kind) {
    return kind | w.chain_dir << 8 | w.bin_from << 16 | w.bin_to << 24;
}
// the most events one row can emit in a call (the header has the argument)
inline uint32_t elt_max_events(uint32_t min_sweeps, uint32_t min_len, uint64_t nbatches) {
    return static_cast<uint32_t>(2 * (1 + (MI_ELT_FRAMES * nbatches - 1) / (static_cast<uint64_t>(min_sweeps) * min_len)) + 1);
}
// What both halves of the ELT stage share (poststage_host.cpp).  elt_plan: MI_OK with the plan, or the settings' refusal with its
// message set.  elt_window: w[256].  elt_state_ok: NULL, or what is impossible about a blob's walker state.
int elt_plan(const mi_elt_cfg* cfg, EltPlan* out);
void elt_window(float* w);
const char* elt_state_ok(const EltRowState* state, size_t rows, const EltPlan& plan);
inline EltRules elt_rules(const EltPlan& p) {
    return EltRules{p.min_span, p.min_len, p.max_len, p.max_step, p.max_drop, p.max_gap, p.min_sweeps};
}

// The device configuration as the plan sees it (poststage_host.cpp): window, twiddles, level table, hop.  The band survey, the channel
// finder and the channel probe have no channels; the plan is built for one at the centre frequency and only its device-wide part is
// used.  MI_OK, or the plan's refusal with its message set.
int device_plan(const mi_device_cfg& dev, Plan& p);

// An I/Q front stage: a stage in front of the demodulator that reads raw I/Q as stage 1 does, cells of wpc windows of it (the band
// survey, the channel probe).  What its handle keeps of the plan, and the bodies its entry points share; `stage` as above.
struct IqFront : Stage {
    using Stage::Stage;
    int nstreams = 0;
    int max_cells = 0;
    uint32_t wpc = 0;  // windows per cell
    int log2n = 0, fft_size = 0, sfmt = 0, sample_bytes = 0;  // sample_bytes: one complex sample
    bool conv_arith = false;
    float conv_scale = 0.0f;
    size_t hop_bytes = 0;
    DevBuf<float> d_window, d_tw, d_levels;
};

// The head of a create call, up to the refusal of a geometry whose workgroup would need more than lds_limit bytes by lds_bytes(log2n,
// sfmt, hop_bytes), the function the stage's launcher sizes its launch with.  MI_OK with the plan, or the refusal.
template <class H>
int iq_front_plan(const char* stage, const mi_device_cfg* dev, H** out, int nstreams, int max_cells, int windows_per_cell,
                  size_t (*lds_bytes)(int, int, unsigned), size_t lds_limit, Plan& plan) {
    if (!dev || !out)
        return fail(MI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (nstreams < 1 || nstreams > 65535 || max_cells < 1 || max_cells >= (1 << 24) || windows_per_cell < 0 || windows_per_cell > (1 << 20))
        return fail(MI_ERR_INVALID, std::string(stage) + " needs 1 <= nstreams < 2^16, 1 <= max_cells < 2^24 and 0 <= windows_per_cell <= 2^20");
    if (const int rc = device_plan(*dev, plan))
        return rc;
    if (plan.hop_bytes == 0 || plan.hop_bytes > (1u << 20))
        return fail(MI_ERR_INVALID, std::string(stage) + ": the hop (sample_rate / 16000 samples) is out of range");
    if (const size_t lds = lds_bytes(plan.log2n, plan.dev.sfmt, static_cast<unsigned>(plan.hop_bytes)); lds > lds_limit)
        return fail(MI_ERR_INVALID, std::string(stage) + ": a workgroup would need " + std::to_string(lds) + " bytes of LDS at this fft_size, sample format and hop (" +
                                        std::to_string(plan.hop_bytes) + " bytes), over the limit of " + std::to_string(lds_limit) +
                                        " (160 KiB): lower the sample rate");
    return MI_OK;
}

// ... and behind the stage's own checks: the device, then the handle with what it keeps of the plan.  MI_OK with *h, or the refusal.
template <class H>
int iq_front_new(const char* stage, const Plan& plan, int nstreams, int max_cells, int windows_per_cell, int gpu, H** h) {
    if (const int rc = check_gpu(gpu, ("no HIP device: the " + std::string(stage) + " runs on the GPU only").c_str()))
        return rc;
    H* s = new (std::nothrow) H();
    if (!s)
        return fail(MI_ERR_NOMEM, "host allocation failed");
    s->gpu = gpu;
    s->nstreams = nstreams;
    s->max_cells = max_cells;
    s->wpc = static_cast<uint32_t>(windows_per_cell ? windows_per_cell : MI_WAVE_BATCH);
    s->log2n = plan.log2n;
    s->fft_size = plan.fft_size;
    s->sfmt = plan.dev.sfmt;
    s->sample_bytes = 2 * plan.bytes_per_sample;
    s->conv_arith = plan.conv_arith;
    s->conv_scale = plan.conv_scale;
    s->hop_bytes = plan.hop_bytes;
    *h = s;
    return MI_OK;
}

// the plan's window, twiddles and level table into the handle's device arrays
inline hipError_t iq_front_upload(IqFront* s, const Plan& plan) {
    if (const hipError_t e = dalloc_copy(s->d_window, plan.window); e != hipSuccess)
        return e;
    if (const hipError_t e = dalloc_copy(s->d_tw, plan.tw); e != hipSuccess)
        return e;
    return dalloc_copy(s->d_levels, plan.levels);
}

// bytes of I/Q a call over ncells cells reads per stream
inline size_t iq_bytes_needed(const IqFront* s, int ncells) {
    if (!s || ncells < 1)
        return 0;
    return (static_cast<size_t>(ncells) * s->wpc - 1) * s->hop_bytes + static_cast<size_t>(s->sample_bytes) * static_cast<size_t>(s->fft_size);
}

// The checks of a call's ncells and I/Q, with the stage's check of its output's alignment where it stands between them.
inline int iq_call_ok(const IqFront* s, const void* d_iq, size_t stream_stride_bytes, int ncells, bool out_aligned, const char* out_text) {
    if (ncells < 1 || ncells > s->max_cells)
        return fail(MI_ERR_INVALID, "ncells outside 1 .. max_cells");
    if (!out_aligned)
        return fail(MI_ERR_INVALID, std::string(s->timing.stage) + ": " + out_text);
    if (!aligned(d_iq, static_cast<uintptr_t>(s->sample_bytes)) || stream_stride_bytes % static_cast<size_t>(s->sample_bytes) != 0)
        return fail(MI_ERR_INVALID, std::string(s->timing.stage) + ": d_iq and the stream stride must be aligned to one complex sample");
    return MI_OK;
}

// What every kernel of an I/Q front stage is told about the call's I/Q and the plan's tables; a stage's own arguments extend it.
struct IqArgs {
    const unsigned char* iq;  // stream s at iq + s*stream_stride
    size_t stream_stride;
    size_t valid_bytes;       // readable bytes per stream starting at its base
    uint32_t hop_bytes;
    const float* window;
    const float* tw;
    const float* levels;
    float conv_scale;
};

inline void iq_args(IqArgs& a, const IqFront* s, const void* d_iq, size_t stream_stride_bytes, int ncells) {
    a.iq = static_cast<const unsigned char*>(d_iq);
    a.stream_stride = stream_stride_bytes;
    a.valid_bytes = iq_bytes_needed(s, ncells);
    a.hop_bytes = static_cast<uint32_t>(s->hop_bytes);
    a.conv_scale = s->conv_scale;
    a.window = s->d_window;
    a.tw = s->d_tw;
    a.levels = s->d_levels;
}

static_assert(sizeof(mi_occ_bin) == 32 && sizeof(mi_occ_candidate) == 40, "the channel finder's record layouts are ABI");
static_assert(sizeof(mi_probe_target) == 8 && sizeof(mi_probe_cell) == 40, "the channel probe's record layouts are ABI");

// The channel finder's settings with the defaults filled in and its view of the device configuration (poststage_host.cpp): MI_OK, or
// the refusal with its message set.  *log2n: the one field the arithmetic uses.
int occ_settings(const mi_device_cfg* dev, const mi_occ_cfg* cfg, mi_occ_cfg* out, int* log2n);

// The packet decoder stage (include/mi_airband.h "packet decoder stage").  One row of its state: the checkpoint blob is an array of
// these, and ax25.hip keeps the same array in device memory.  The lanes' fields lie lane by lane, so a wave's lane l reads field[l].
struct Ax25RowState {
    float x[MI_AX25_HISTORY];               // the last 14 input samples of the row's last batch, oldest first
    uint64_t batch;                         // batches seen since creation / set_state
    uint64_t last_end;                      // where the closing flag of the row's last record ended, in absolute thirds
    uint64_t start[MI_AX25_LANES];          // where the lane's frame began
    uint16_t nbytes[MI_AX25_LANES], crc[MI_AX25_LANES];
    uint8_t prev[MI_AX25_LANES], ones[MI_AX25_LANES], phase[MI_AX25_LANES], nbits[MI_AX25_LANES], cur[MI_AX25_LANES], zero[2];
    uint8_t bytes[MI_AX25_LANES][MI_AX25_RAW_BYTES];
};
constexpr int kAx25LaneWords = MI_AX25_RAW_BYTES / 4;  // 83 words of frame bytes a lane
constexpr uint32_t ax25_crc_bit(const uint32_t crc, const uint32_t d) {
    return (crc ^ d) & 1u ? crc >> 1 ^ 0x8408u : crc >> 1;
}
constexpr uint32_t ax25_flag_residue() {
    uint32_t crc = MI_AX25_RESIDUE;
    for (int i = 0; i < 6; ++i)
        crc = ax25_crc_bit(crc, i ? 1u : 0u);
    return crc;
}
static_assert(sizeof(Ax25RowState) == MI_AX25_STATE_ROW_BYTES && offsetof(Ax25RowState, batch) == 56 && offsetof(Ax25RowState, start) == 72 &&
                  offsetof(Ax25RowState, nbytes) == 312 && offsetof(Ax25RowState, prev) == 432 && offsetof(Ax25RowState, zero) == 582 &&
                  offsetof(Ax25RowState, bytes) == 584 && sizeof(mi_ax25_frame) == 352 && offsetof(mi_ax25_frame, nbytes) == 16 &&
                  offsetof(mi_ax25_frame, bytes) == 20 && sizeof(mi_ax25_cfg) == 16 && (MI_AX25_HISTORY + 2) % 4 == 0 &&
                  MI_AX25_MAX_BYTES <= MI_AX25_RAW_BYTES && MI_AX25_RAW_BYTES % 4 == 0 && MI_AX25_LANES == MI_AX25_SLICERS * MI_AX25_HYPOTHESES &&
                  40 * MI_AX25_BITS == 3 * kWaveBatch && MI_AX25_BIT_WORDS * 32 >= MI_AX25_BITS && ax25_flag_residue() == MI_AX25_FLAG_RESIDUE,
              "the packet stage's blob, record and settings layouts are ABI");
// The settings with every default filled in, as both halves take them.
struct Ax25Plan {
    float gain[MI_AX25_SLICERS];
    uint32_t strict;     // 0 / 1
    mi_ax25_cfg filled;  // the settings as the caller would have written them
};
struct Ax25Gains {
    float g[MI_AX25_SLICERS];
};
// A lane's deframer, as the walk carries it in registers; its bytes so far stay in memory beside it.
struct Ax25Lane {
    uint32_t prev, ones, phase, nbits, cur, nbytes, crc;
    uint64_t start;
};
// the most records one row can have in a call (the header argues it)
inline uint32_t ax25_max_frames(uint64_t nbatches) {
    return static_cast<uint32_t>(1 + MI_AX25_BITS * nbatches / 143);
}
// Where slot j of hypothesis tau ends, in thirds from the batch's first.
__host__ __device__ inline int ax25_slot_end(const int tau, const int j) {
    return 4 * tau + 40 * (j + 1 - (tau > 0));
}
// Slot j of hypothesis tau over what is staged for a block -- s[kLead + n] is the block's sample n, kLead = MI_AX25_HISTORY + 2 --, T
// the four templates: the three slicers' tone bits, slicer g's in bit g.  Host and device run this text.
__host__ __device__ inline uint32_t ax25_bit(const float* s, const float* T, const Ax25Gains& gain, const int tau, const int j) {
    const int t0 = 4 * tau + 40 * (j - (tau > 0));  // -36 .. 5960
    const int n0 = (t0 + 41) / 3 - 13;              // ceil(t0 / 3)
    int rho = 3 * n0 - t0;                          // 0 .. 2
    const bool more = rho == 0;
    const float* const x = s + (MI_AX25_HISTORY + 2) + n0;
    float s0 = x[0] * T[rho], s1 = x[0] * T[40 + rho], s2 = x[0] * T[80 + rho], s3 = x[0] * T[120 + rho];
#pragma unroll
    for (int i = 1; i < 13; ++i) {
        rho += 3;
        s0 = s0 + x[i] * T[rho];
        s1 = s1 + x[i] * T[40 + rho];
        s2 = s2 + x[i] * T[80 + rho];
        s3 = s3 + x[i] * T[120 + rho];
    }
    if (more) {
        rho += 3;
        s0 = s0 + x[13] * T[rho];
        s1 = s1 + x[13] * T[40 + rho];
        s2 = s2 + x[13] * T[80 + rho];
        s3 = s3 + x[13] * T[120 + rho];
    }
    const float pm = s0 * s0 + s1 * s1, ps = s2 * s2 + s3 * s3;
    return (pm >= gain.g[0] * ps ? 1u : 0u) | (pm >= gain.g[1] * ps ? 2u : 0u) | (pm >= gain.g[2] * ps ? 4u : 0u);
}
// What a slot did to a lane: kAx25Flag -- the slot is a flag's last bit, the caller opens the next frame with ax25_open behind
// whatever it does about the old one --, with kAx25Cand where the lane's frame is a candidate (whole bytes, at least 17, the check
// right; the address field and the ordering are the caller's to judge).
enum { kAx25Flag = 1, kAx25Cand = 2 };
__host__ __device__ inline void ax25_wait(Ax25Lane& L) {
    L.phase = MI_AX25_WAIT;
    L.nbits = L.cur = L.nbytes = L.crc = 0;
    L.start = 0;
}
__host__ __device__ inline void ax25_open(Ax25Lane& L, const uint64_t next) {
    L.phase = MI_AX25_FRAME;
    L.nbits = L.cur = L.nbytes = 0;
    L.crc = 0xFFFFu;
    L.start = next;
}
// One tone bit t through a lane's deframer; store(i, byte) takes byte number i of the frame.  Bytes behind nbytes are whatever an
// earlier frame left: whoever reads a lane's bytes takes nbytes of them.  Host and device run this text.
template <class Store>
__host__ __device__ inline uint32_t ax25_step(Ax25Lane& L, const uint32_t t, Store&& store) {
    const uint32_t d = t == L.prev ? 1u : 0u, n = L.ones;
    L.prev = t;
    L.ones = d ? (n < 7u ? n + 1u : 7u) : 0u;
    if (n >= 5u) {
        if (n != 6u)
            return 0;
        if (d) {
            ax25_wait(L);
            return 0;
        }
        return L.phase == MI_AX25_FRAME && L.nbits == 6u && L.nbytes >= MI_AX25_MIN_BYTES && L.crc == MI_AX25_FLAG_RESIDUE ? kAx25Flag | kAx25Cand : kAx25Flag;
    }
    if (L.phase != MI_AX25_FRAME)
        return 0;
    L.cur |= d << L.nbits;
    L.crc = ax25_crc_bit(L.crc, d);
    if (++L.nbits == 8u) {
        if (L.nbytes == MI_AX25_MAX_BYTES) {
            ax25_wait(L);
        } else {
            store(L.nbytes, L.cur);
            ++L.nbytes;
            L.nbits = L.cur = 0;
        }
    }
    return 0;
}
// Whether a callsign byte, shifted right by one, is 'A'-'Z', '0'-'9' or a space.
__host__ __device__ inline bool ax25_call_char(const uint32_t byte) {
    const uint32_t c = byte >> 1;
    return (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == ' ';
}
// The number of addresses of a frame of nbytes bytes whose address field is well formed, else 0.
inline uint32_t ax25_naddr(const uint8_t* b, const uint32_t nbytes) {
    uint32_t i = 0;
    while (i < 70 && i + 3 < nbytes && !(b[i] & 1u))
        ++i;
    if (i >= 70 || i + 3 >= nbytes || i % 7 != 6 || i < 13)
        return 0;
    for (uint32_t k = 0; k < i; ++k)
        if (k % 7 != 6 && !ax25_call_char(b[k]))
            return 0;
    return (i + 1) / 7;
}
// What both halves of the packet stage share (poststage_host.cpp).  ax25_plan: MI_OK with the plan, or the settings' refusal with its
// message set.  ax25_templates: t[160].  ax25_state_ok: NULL, or what is impossible about a blob.
int ax25_plan(const mi_ax25_cfg* cfg, Ax25Plan* out);
void ax25_templates(float* t);
const char* ax25_state_ok(const Ax25RowState* state, size_t rows);

// The pager decoder stage (include/mi_airband.h "pager decoder stage").  One row of its state: the checkpoint blob is an array of
// these, and pocsag.hip keeps the same array in device memory.
struct PocsagRowState {
    float x[MI_POCSAG_HISTORY];             // the last 34 input samples of the row's last batch, oldest first
    uint32_t batch;                         // batches seen since creation / set_state
    uint32_t phase;                         // MI_POCSAG_IDLE / MI_POCSAG_TRANSMISSION
    uint64_t hist[MI_POCSAG_MAX_LANES];     // per lane the last 64 bits, the newest in bit 0
    uint32_t lane, inverted, pos, cur, nbits, gbad, lane_sync, mismatches, wbatch, wtwelfth, open, zero;
    mi_pocsag_message msg;                  // the open message as the record has it so far
};
static_assert(sizeof(PocsagRowState) == MI_POCSAG_STATE_ROW_BYTES && offsetof(PocsagRowState, batch) == 136 && offsetof(PocsagRowState, hist) == 144 &&
                  offsetof(PocsagRowState, lane) == 384 && offsetof(PocsagRowState, msg) == 432 && sizeof(mi_pocsag_message) == 368 &&
                  offsetof(mi_pocsag_message, corrected) == 24 && offsetof(mi_pocsag_message, lane_end) == 29 && offsetof(mi_pocsag_message, bad) == 32 &&
                  offsetof(mi_pocsag_message, words) == 48 && sizeof(mi_pocsag_cfg) == 20 && (MI_POCSAG_HISTORY + 2) % 4 == 0 &&
                  MI_POCSAG_MAX_LANES == 2 * MI_POCSAG_MAX_HYPOTHESES && MI_POCSAG_MAX_WORDS <= 96,
              "the pager stage's blob, record and settings layouts are ABI");
// The grid of a baud: a bit's twelfths, the hypotheses' distance, their number, the bits and the words of a batch and hypothesis.
struct PocsagGeom {
    int L, step, H, B, W;
};
__host__ __device__ inline PocsagGeom pocsag_geom(const uint32_t baud) {  // (baud: 512, 1200 or 2400)
    return baud == 512 ? PocsagGeom{375, 25, 15, 64, 2} : baud == 2400 ? PocsagGeom{80, 8, 10, 300, 10} : PocsagGeom{160, 16, 10, 150, 5};
}
constexpr int kPocsagTwelfths = 12 * kWaveBatch;
constexpr uint32_t kPocsagNoHit = 99, kPocsagNoPattern = 1;
// The settings with every default filled in, as both halves take them.
struct PocsagPlan {
    PocsagGeom g;
    uint32_t sync_errors;      // the number itself, 0 .. 4
    uint32_t preamble_errors;  // the number itself, 0 .. 8; 32 where the condition is off (no 32 bits are further than 16 from both phases)
    uint32_t correct;          // the number itself, 0 .. 2
    uint32_t hold_timing;
    mi_pocsag_cfg filled;      // the settings as the caller would have written them
};
// The walker's part of a row's state, as the walk carries it in registers; the open message stays in memory beside it.
struct PocsagWalker {
    uint32_t phase, lane, inverted, pos, cur, nbits, gbad, lane_sync, mismatches, wbatch, wtwelfth, open;
};
// the most messages one row can close in a call: the first word can end with the call's first bit, each further one takes 32 of
// the n B slots and the at most n bits that the moves 1 -> 0 add
inline uint32_t pocsag_max_messages(const PocsagGeom& g, uint64_t nbatches) {
    return static_cast<uint32_t>(1 + (nbatches * static_cast<uint64_t>(g.B + 1) - 1) / 32);
}
// Where slot j of hypothesis tau begins, in twelfths from the batch's first sample (negative: in the batch before).
__host__ __device__ inline int pocsag_slot_begin(const PocsagGeom& g, const int tau, const int j) {
    return tau * g.step + g.L * (j - (tau > 0));
}
// Slot j of hypothesis tau over what is staged for a block -- s[kLead + n] is the block's sample n, kLead = MI_POCSAG_HISTORY + 2 --:
// the sum of the bit's samples, and their number into *k.  Host and device run this text.
__host__ __device__ inline float pocsag_sum(const float* s, const PocsagGeom& g, const int tau, const int j, int* k) {
    const int t0 = pocsag_slot_begin(g, tau, j);  // -350 .. 24000 - L
    const int n0 = (t0 + 371) / 12 - 30;          // ceil(t0 / 12), -29 ..
    const int n1 = (t0 + g.L + 371) / 12 - 30;    // .. 2000
    const float* const x = s + (MI_POCSAG_HISTORY + 2) + n0;
    float a = x[0];
    for (int i = 1; i < n1 - n0; ++i)
        a = a + x[i];
    *k = n1 - n0;
    return a;
}
// The remainder of a word's bits 31 .. 1 under the generator 0x769.
__host__ __device__ inline uint32_t pocsag_syndrome(const uint32_t word) {
    uint32_t r = word >> 1;
    for (int i = 30; i >= 10; --i)
        if (r >> i & 1u)
            r ^= 0x769u << (i - 10);
    return r;
}
// One word by the header's rule, table[syndrome] = the error pattern of weight <= 2 in bits 31 .. 1 (kPocsagNoPattern: none): e, the
// word being good where e <= correct; *fixed = the word repaired (as received where there is no pattern, e = 3).
__host__ __device__ inline uint32_t pocsag_repair(const uint32_t* table, const uint32_t word, uint32_t* fixed) {
    const uint32_t pat = table[pocsag_syndrome(word)];
    if (pat == kPocsagNoPattern) {
        *fixed = word;
        return 3u;
    }
    uint32_t f = word ^ pat, e = static_cast<uint32_t>(__builtin_popcount(pat));
    if (__builtin_popcount(f) & 1) {
        f ^= 1u;
        ++e;
    }
    *fixed = f;
    return e;
}
// A lane's last 64 bits against SYNC, its complement and the preamble: the sync mismatches of a hit, else kPocsagNoHit.
__host__ __device__ inline uint32_t pocsag_hit(const uint64_t h, const uint32_t sync_errors, const uint32_t preamble_errors, uint32_t* inverted) {
    uint32_t m = static_cast<uint32_t>(__builtin_popcount(static_cast<uint32_t>(h) ^ MI_POCSAG_SYNC));
    *inverted = m > 16u;
    if (m > 16u)
        m = 32u - m;
    uint32_t p = static_cast<uint32_t>(__builtin_popcount(static_cast<uint32_t>(h >> 32) ^ 0xAAAAAAAAu));
    if (p > 16u)
        p = 32u - p;
    return m <= sync_errors && p <= preamble_errors ? m : kPocsagNoHit;
}
// The lane a sync opens the transmission on: mism[lane] = pocsag_hit's answer, q[lane] = Q of the slot's batch; -1: no hit.
__host__ __device__ inline int pocsag_pick(const uint32_t* mism, const float* q, const int lanes) {
    int best = -1;
    for (int t = 0; t < lanes; ++t) {
        if (mism[t] == kPocsagNoHit)
            continue;
        if (best < 0 || mism[t] < mism[best] || (mism[t] == mism[best] && q[t] > q[best]))
            best = t;
    }
    return best;
}
__host__ __device__ inline void pocsag_open(PocsagWalker& w, const int lane, const uint32_t inverted, const uint32_t mismatches) {
    w = PocsagWalker{};
    w.phase = MI_POCSAG_TRANSMISSION;
    w.lane = w.lane_sync = static_cast<uint32_t>(lane);
    w.inverted = inverted;
    w.mismatches = mismatches;
}
// The timing move at a batch's first slot inside a transmission, from the new batch's Q.
enum { kPocsagInStep = 0, kPocsagSkip = 1, kPocsagReplay = 2 };
__host__ __device__ inline int pocsag_retime(PocsagWalker& w, const float* q, const int H) {
    const uint32_t h = static_cast<uint32_t>(H), base = w.lane / h * h, u = w.lane - base, um = (u + h - 1) % h, up = (u + 1) % h;
    uint32_t v = u;
    if (q[base + um] > q[base + v])
        v = um;
    if (q[base + up] > q[base + v])
        v = up;
    w.lane = base + v;
    return u == 0 && v == 1 ? kPocsagSkip : u == 1 && v == 0 ? kPocsagReplay : kPocsagInStep;
}
// The open message closes: emit() takes the record out of *msg (the caller adds row, end_batch and lane_end), then it is cleared.
template <class Emit>
__host__ __device__ inline void pocsag_close(PocsagWalker& w, mi_pocsag_message* msg, Emit& emit) {
    if (!w.open)
        return;
    emit();
    const uint32_t n = offsetof(mi_pocsag_message, words) / 4 + msg->nwords;
    for (uint32_t i = 0; i < n; ++i)
        reinterpret_cast<uint32_t*>(msg)[i] = 0;
    w.open = 0;
}
// The walker's running word is whole: what it does to the group, the open message and the transmission.  Host and device run this
// text, the device with wave-uniform values and every lane writing the same bytes of *msg.
template <class Emit>
__host__ __device__ inline void pocsag_word(PocsagWalker& w, mi_pocsag_message* msg, const uint32_t* table, const uint32_t sync_errors, const uint32_t correct,
                                            Emit& emit) {
    const uint32_t word = w.cur;
    w.cur = w.nbits = 0;
    if (w.pos == 16) {  // the SYNC behind word 15
        if (static_cast<uint32_t>(__builtin_popcount(word ^ MI_POCSAG_SYNC)) <= sync_errors) {
            w.pos = w.gbad = 0;
        } else {
            pocsag_close(w, msg, emit);
            w = PocsagWalker{};
        }
        return;
    }
    uint32_t fixed;
    const uint32_t e = pocsag_repair(table, word, &fixed);
    const bool good = e <= correct;
    if (good && fixed == MI_POCSAG_IDLE_WORD) {
        pocsag_close(w, msg, emit);
    } else if (good && !(fixed >> 31)) {
        pocsag_close(w, msg, emit);
        msg->batch = w.wbatch;
        msg->twelfth = w.wtwelfth;
        msg->address = (fixed >> 13 & 0x3FFFFu) << 3 | w.pos >> 1;
        msg->function = static_cast<uint8_t>(fixed >> 11 & 3u);
        msg->corrected = static_cast<uint16_t>(e);
        msg->inverted = static_cast<uint8_t>(w.inverted);
        msg->sync_errors = static_cast<uint8_t>(w.mismatches);
        msg->lane_sync = static_cast<uint8_t>(w.lane_sync);
        w.open = 1;
    } else if (w.open) {
        const uint32_t i = msg->nwords;
        if (i == MI_POCSAG_MAX_WORDS) {
            msg->truncated = 1;
        } else {
            msg->words[i] = good ? fixed : word;
            if (good) {
                msg->corrected = static_cast<uint16_t>(msg->corrected + e);
            } else {
                msg->bad[i / 32] |= 1u << (i % 32);
                msg->nbad = static_cast<uint8_t>(msg->nbad + 1);
            }
            msg->nwords = static_cast<uint8_t>(i + 1);
        }
    }
    w.gbad += good ? 0u : 1u;
    if (++w.pos == 16 && w.gbad == 16) {
        pocsag_close(w, msg, emit);
        w = PocsagWalker{};
    }
}
// One bit, polarity undone, that begins t twelfths from the first sample of the row's batch number `batch`, into the running word.
template <class Emit>
__host__ __device__ inline void pocsag_take(PocsagWalker& w, mi_pocsag_message* msg, const uint32_t* table, const uint32_t sync_errors, const uint32_t correct,
                                            const uint32_t bit, const uint32_t batch, const int t, Emit& emit) {
    if (w.nbits == 0) {
        w.wbatch = t < 0 ? batch - 1u : batch;
        w.wtwelfth = static_cast<uint32_t>(t < 0 ? t + kPocsagTwelfths : t);
    }
    w.cur = w.cur << 1 | bit;
    if (++w.nbits == 32)
        pocsag_word(w, msg, table, sync_errors, correct, emit);
}
// What both halves of the pager stage share (poststage_host.cpp).  pocsag_plan: MI_OK with the plan, or the settings' refusal with
// its message set.  pocsag_table: t[1024].  pocsag_state_ok: NULL, or what is impossible about a blob on a handle of the plan's baud.
int pocsag_plan(const mi_pocsag_cfg* cfg, PocsagPlan* out);
void pocsag_table(uint32_t* t);
const char* pocsag_state_ok(const PocsagRowState* state, size_t rows, const PocsagPlan& plan);

}  // namespace mi
