// tuning.cpp -- the table of a handle's tuning switches (tuning.hpp) and the two routes into it.
#include "tuning.hpp"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>

#include "../../include/mi_airband.h"

namespace mi {
namespace {

// One switch: the names it goes by, and how a value is normalised and stored
struct Switch {
    int id;           // MI_OPT_*, or 0: no mi_demod_set_option twin
    const char* env;  // MI_AIRBAND_*, or null: not read from the environment
    const char* (*store)(Tuning&, int value);  // returns null, or why the value is refused (the field is left alone then)
    void (*from_text)(Tuning&, const char* text);  // the environment's route where it is not store(atoi(text)), else null
};

template <auto Field>
const char* flag(Tuning& t, int v) {
    t.*Field = v != 0;
    return nullptr;
}
template <int Tuning::*Field, int Lo, int Hi = INT_MAX>
const char* clamped(Tuning& t, int v) {
    t.*Field = std::max(Lo, std::min(Hi, v));
    return nullptr;
}
template <int Tuning::*Field, int Lo, int Hi>
const char* in_range_or_0(Tuning& t, int v) {
    t.*Field = (v >= Lo && v <= Hi) ? v : 0;
    return nullptr;
}
const char* uni_rows(Tuning& t, int v) {
    if (v < 1)
        return "MI_OPT_UNI_ROWS must be >= 1";
    t.uni_rows = v;
    return nullptr;
}
const char* tp_ratio_pct(Tuning& t, int v) {
    t.tp_ratio = v <= 0 ? 0.0 : std::max(0.25, v / 100.0);
    return nullptr;
}
const char* tp_segment(Tuning& t, int v) {
    t.tp_L = (v == 512 || v == 1024 || v == 2048 || v == 4096) ? v : 0;
    return nullptr;
}

// The environment has no "auto" (-1) and no "default" (0) to give: it is left unset for those
void env_tp(Tuning& t, const char* e) {
    t.tp = std::atoi(e) != 0;
}
void env_conv(Tuning& t, const char* e) {  // lut | arith
    t.conv = e[0] == 'a' || e[0] == 'A';
}
template <int Tuning::*Field>
void env_at_least_1(Tuning& t, const char* e) {
    t.*Field = std::max(1, std::atoi(e));
}
void env_tp_ratio(Tuning& t, const char* e) {  // a factor, not a percentage
    t.tp_ratio = std::max(0.25, std::atof(e));
}

// Defaults of a new handle's tuning switches come from the caller's environment (A/B measurements, tests):
//   MI_AIRBAND_TP=0|1        serial kernel / time-parallel path whenever eligible
//   MI_AIRBAND_PRUNE=0       full FFT graph at N = 512 (the pruned one is bit-exact and faster where it applies)
//   MI_AIRBAND_CONV=lut|arith  u8 conversion through the level table / the arithmetic form the plan has checked against it
//   MI_AIRBAND_STEADY=0      serial stage 2 takes every step in the sample loop
//   MI_AIRBAND_TP_SEGMENT=512|1024|2048|4096  steps per segment of the time-parallel path (default: by row count; sizes the scratch,
//                            so it is read when the handle is created and has no mi_demod_set_option twin)
//   MI_AIRBAND_L64=0         no lane-resident stage 1 at N = 512, 1024, 2048 (the pruned / full exchange kernels instead)
//   MI_AIRBAND_UNI_ROWS=n, MI_AIRBAND_TP_CHUNKS=n, MI_AIRBAND_TP_RATIO=x, MI_AIRBAND_TP_LPW=n
// (MI_AIRBAND_DEBUG=1 names every one found on stderr: a variable exported for a test changes a production handle just as silently)
const Switch kSwitches[] = {
    {MI_OPT_EARLY_INPUT, nullptr, flag<&Tuning::early_input>, nullptr},
    {MI_OPT_STEADY_BLOCKS, "MI_AIRBAND_STEADY", flag<&Tuning::steady_blocks>, nullptr},
    {MI_OPT_TIME_PARALLEL, "MI_AIRBAND_TP", clamped<&Tuning::tp, -1, 1>, env_tp},
    {MI_OPT_PRUNE_FFT, "MI_AIRBAND_PRUNE", flag<&Tuning::prune>, nullptr},
    {MI_OPT_U8_CONVERSION, "MI_AIRBAND_CONV", clamped<&Tuning::conv, -1, 1>, env_conv},
    {MI_OPT_UNI_ROWS, "MI_AIRBAND_UNI_ROWS", uni_rows, env_at_least_1<&Tuning::uni_rows>},
    {MI_OPT_TP_CHUNKS, "MI_AIRBAND_TP_CHUNKS", clamped<&Tuning::tp_chunks, 0>, env_at_least_1<&Tuning::tp_chunks>},
    {MI_OPT_TP_RATIO_PCT, "MI_AIRBAND_TP_RATIO", tp_ratio_pct, env_tp_ratio},
    {MI_OPT_TP_SEG_LANES, "MI_AIRBAND_TP_LPW", in_range_or_0<&Tuning::tp_lpw, 1, 64>, nullptr},
    {MI_OPT_LANE_FFT, "MI_AIRBAND_L64", flag<&Tuning::l64>, nullptr},
    {MI_OPT_LANE_FFT_JIT, "MI_AIRBAND_L64_JIT", flag<&Tuning::l64_jit>, nullptr},
    {MI_OPT_CORE_SPLIT, "MI_AIRBAND_CORE_SPLIT", flag<&Tuning::core_split>, nullptr},
    {MI_OPT_SPEC_HEAD, "MI_AIRBAND_SPEC_HEAD", flag<&Tuning::spec_head>, nullptr},
    {MI_OPT_PRE_WAVE, "MI_AIRBAND_PRE_WAVE", clamped<&Tuning::pre_wave, -1, 2>, nullptr},
    {MI_OPT_RESERVE_CUS, "MI_AIRBAND_RESERVE_CUS", clamped<&Tuning::reserve_cus, -1>, nullptr},
    {MI_OPT_AUDIO_WAVE, "MI_AIRBAND_AUDIO_WAVE", flag<&Tuning::audio_wave>, nullptr},
    {MI_OPT_MIXED_PLAN, "MI_AIRBAND_MIXED", flag<&Tuning::mixed>, nullptr},
    {MI_OPT_SPLIT_CUS, "MI_AIRBAND_SPLIT_CUS", clamped<&Tuning::split_cus, -1>, nullptr},
    {0, "MI_AIRBAND_TP_SEGMENT", tp_segment, nullptr},
    {0, "MI_AIRBAND_TP_EAGER", flag<&Tuning::tp_eager>, nullptr},
    {0, "MI_AIRBAND_CORE_LEAD", clamped<&Tuning::core_lead, 0>, nullptr},
    {0, "MI_AIRBAND_AGC_HINT", flag<&Tuning::agc_hint>, nullptr},
    {0, "MI_AIRBAND_CORE_DECAY", flag<&Tuning::core_decay>, nullptr},
    {0, "MI_AIRBAND_CORE_GUESS", clamped<&Tuning::core_guess, 0, 2>, nullptr},
    {0, "MI_AIRBAND_CORE_LEAN", flag<&Tuning::core_lean>, nullptr},
    {0, "MI_AIRBAND_L64_WGS", clamped<&Tuning::l64_wgs, 0>, nullptr},
};

}  // namespace

bool debug_enabled() {
    const char* e = std::getenv("MI_AIRBAND_DEBUG");
    return e && std::atoi(e) != 0;
}

void tuning_from_env(Tuning& t) {
    const bool debug = debug_enabled();
    for (const Switch& sw : kSwitches) {
        const char* e = sw.env ? std::getenv(sw.env) : nullptr;
        if (!e || !*e)  // (set but empty counts as unset)
            continue;
        if (debug)
            std::fprintf(stderr, "mi_airband: %s=%s (from the environment)\n", sw.env, e);
        if (sw.from_text)
            sw.from_text(t, e);
        else
            sw.store(t, std::atoi(e));
    }
}

int tuning_set(Tuning& t, int option, int value, const char** why) {
    *why = "unknown option";
    for (const Switch& sw : kSwitches)
        if (sw.id == option && option != 0)
            *why = sw.store(t, value);
    return *why ? MI_ERR_INVALID : MI_OK;
}

}  // namespace mi
