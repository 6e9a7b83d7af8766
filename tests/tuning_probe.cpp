// tuning_probe -- csrc/tuning.cpp on its own, for tests/test_tuning.py.
//   tuning_probe [NAME=text ...] [ID:VALUE ...]
// sets the environment variables, reads the defaults from them (tuning_from_env), makes the tuning_set calls in order and prints
// every field and every return code as one JSON object.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../boondock-airband_amd/csrc/tuning.hpp"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (const char* eq = std::strchr(argv[i], '='))
            setenv(std::string(argv[i], static_cast<size_t>(eq - argv[i])).c_str(), eq + 1, 1);
    mi::Tuning t;
    mi::tuning_from_env(t);
    std::printf("{\"set\": [");
    const char* sep = "";
    for (int i = 1; i < argc; ++i) {
        const char* colon = std::strchr(argv[i], ':');
        if (!colon || std::strchr(argv[i], '='))
            continue;
        const char* why = nullptr;
        const int rc = mi::tuning_set(t, std::atoi(argv[i]), std::atoi(colon + 1), &why);
        std::printf("%s[%d, \"%s\"]", sep, rc, why ? why : "");
        sep = ", ";
    }
    std::printf("], \"fields\": {");
    sep = "";
#define FIELD(name) std::printf("%s\"" #name "\": %.17g", sep, static_cast<double>(t.name)), sep = ", "
    FIELD(early_input);
    FIELD(steady_blocks);
    FIELD(tp);
    FIELD(conv);
    FIELD(prune);
    FIELD(uni_rows);
    FIELD(tp_chunks);
    FIELD(tp_ratio);
    FIELD(tp_lpw);
    FIELD(tp_L);
    FIELD(pre_wave);
    FIELD(audio_wave);
    FIELD(spec_head);
    FIELD(mixed);
    FIELD(tp_eager);
    FIELD(core_lead);
    FIELD(agc_hint);
    FIELD(core_decay);
    FIELD(core_guess);
    FIELD(core_lean);
    FIELD(core_split);
    FIELD(l64);
    FIELD(l64_wgs);
    FIELD(l64_jit);
    FIELD(reserve_cus);
    FIELD(split_cus);
#undef FIELD
    std::printf("}}\n");
    return 0;
}
