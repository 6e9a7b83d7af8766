// tuning.hpp -- the tuning switches of a handle: one record, one table (tuning.cpp) that says how each is set from the
// MI_AIRBAND_* environment and through mi_demod_set_option.  Plain C++: nothing here needs a device.
#pragma once

namespace mi {

// (defaults from the environment at mi_demod_create, then mi_demod_set_option: per handle, the library keeps no process-wide state)
struct Tuning {
    bool early_input = false;   // MI_OPT_EARLY_INPUT: the IQ of a call is valid when the call is made
    bool steady_blocks = true;  // MI_OPT_STEADY_BLOCKS
    int tp = -1;          // MI_OPT_TIME_PARALLEL: -1 auto, 0 serial kernel, 1 time-parallel whenever eligible
    int conv = -1;        // MI_OPT_U8_CONVERSION: -1 auto, 0 level table, 1 arithmetic
    bool prune = true;    // MI_OPT_PRUNE_FFT
    int uni_rows = 4096;  // MI_OPT_UNI_ROWS: up to this many rows keep one channel per wave in k_demod
    int tp_chunks = 0;    // MI_OPT_TP_CHUNKS: 0 = measured default
    double tp_ratio = 0;  // MI_OPT_TP_RATIO_PCT / 100: 0 = measured default
    int tp_lpw = 0;       // MI_OPT_TP_SEG_LANES: lanes per wave of the segment pass, 0 = auto
    int tp_L = 0;         // MI_AIRBAND_TP_SEGMENT at create: 0 = by row count
    int pre_wave = -1;       // MI_OPT_PRE_WAVE: serial kernel, one channel per wave: further waves per channel walk the squelch pre-filter ahead and the audio behind (k_demod_pw); -1 = up to 256 rows
    bool audio_wave = true;  // MI_OPT_AUDIO_WAVE: ... and NFM channels a third wave for everything behind the filtered I/Q (audio, CTCSS, gate, stores)
    bool spec_head = true;   // MI_OPT_SPEC_HEAD: overlapped calls start their first segments from a guessed state (see TpArgs)
    bool mixed = true;       // MI_OPT_MIXED_PLAN: the plain AM rows of a mixed plan take the time-parallel path, the others the serial kernel beside it
    int tp_eager = 0;        // (diagnostic, MI_AIRBAND_TP_EAGER)
    int core_lead = 0;       // (diagnostic, MI_AIRBAND_CORE_LEAD) blocks the noise-floor wave may run ahead, 0 = default
    int agc_hint = 1;        // (diagnostic, MI_AIRBAND_AGC_HINT=0) segment lanes start from agcavgfast = 0.5 instead of the channel's last value
    int core_decay = 1;      // (diagnostic, MI_AIRBAND_CORE_DECAY=0) no decay waves: the walking wave steps every decay itself
    int core_guess = 1;      // (diagnostic, MI_AIRBAND_CORE_GUESS) 0: the noise-floor wave walks systolic passes only; 2: the first guess-and-verify rounds (groups of 64)
    int core_lean = 1;       // (diagnostic, MI_AIRBAND_CORE_LEAN=0) k_tp_core2 without the round-4 run paths and restarts
    bool core_split = true;  // MI_OPT_CORE_SPLIT: noise-floor passes of the core chain on their own wave (k_tp_core2)
    bool l64 = true;      // MI_OPT_LANE_FFT: the lane-resident stage 1 (N = 512, 1024, 2048) where the plan allows it
    int l64_wgs = 0;      // (diagnostic, MI_AIRBAND_L64_WGS) workgroups per CU of the persistent stage-1 launch, 0 = default
    bool l64_jit = true;  // MI_OPT_LANE_FFT_JIT: compile the plan's own instance with hipRTC (else the full-graph instance)
    int reserve_cus = -1;  // MI_OPT_RESERVE_CUS: -1 auto: 32 for handles of up to 64 rows, none beyond; 0 none
    int split_cus = -1;    // MI_OPT_SPLIT_CUS: -1 auto (see enqueue_serial_pipelined)
};

// MI_AIRBAND_DEBUG is set to a non-zero number: the library explains itself on stderr
bool debug_enabled();
// Defaults of a new handle's switches from the caller's environment
void tuning_from_env(Tuning& t);
// mi_demod_set_option without the handle: MI_OK, or MI_ERR_INVALID with *why set and `t` as it was
int tuning_set(Tuning& t, int option, int value, const char** why);

}  // namespace mi
