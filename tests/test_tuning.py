"""The tuning switches of a handle (csrc/tuning.cpp) without a GPU: how each MI_AIRBAND_* variable and each mi_demod_set_option value
is normalised, route by route.  The GPU tests steer the library almost entirely through these variables, so a wrong clamp here would
silently change what a parity test covers.  tests/tuning_probe.cpp links tuning.cpp alone; the expectations below are written from the
rules (include/mi_airband.h, README "tuning switches"), not read back from the code."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boondock-airband_amd", "csrc")

INVALID = -1  # MI_ERR_INVALID

DEFAULTS = dict(early_input=0, steady_blocks=1, tp=-1, conv=-1, prune=1, uni_rows=4096, tp_chunks=0, tp_ratio=0.0, tp_lpw=0, tp_L=0,
                pre_wave=-1, audio_wave=1, spec_head=1, mixed=1, tp_eager=0, core_lead=0, agc_hint=1, core_decay=1, core_guess=1,
                core_lean=1, core_split=1, l64=1, l64_wgs=0, l64_jit=1, reserve_cus=-1, split_cus=-1)


def _makefile_var(name, text):
    return re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/tuning_probe.cpp + csrc/tuning.cpp, built with the compiler and flags of csrc/Makefile's %.cpp rule, as host code only."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC", _makefile_var("HIPCC", mk))
    flags = _makefile_var("CXXFLAGS", mk).replace("$(EXTRA)", "").split()
    exe = str(tmp_path_factory.mktemp("tuning") / "tuning_probe")
    cmd = [hipcc, "-x", "c++"] + flags + [os.path.join(ROOT, "tests", "tuning_probe.cpp"), os.path.join(CSRC, "tuning.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(env=None, sets=()):
        # the probe calls setenv itself; whatever MI_AIRBAND_* the caller of pytest has exported is kept away from it
        clean = {k: v for k, v in os.environ.items() if not k.startswith("MI_AIRBAND_")}
        args = ["%s=%s" % kv for kv in (env or {}).items()] + ["%d:%d" % s for s in sets]
        out = subprocess.run([exe] + args, env=clean, capture_output=True, text=True, check=True).stdout
        got = json.loads(out)
        return got["fields"], [tuple(x) for x in got["set"]]

    return run


def _env(**kw):
    return {"MI_AIRBAND_" + k: str(v) for k, v in kw.items()}


# mi_demod_set_option ids (include/mi_airband.h)
EARLY_INPUT, STEADY_BLOCKS, TIME_PARALLEL, PRUNE_FFT, U8_CONVERSION, UNI_ROWS, TP_CHUNKS, TP_RATIO_PCT, TP_SEG_LANES = range(1, 10)
LANE_FFT, LANE_FFT_JIT, CORE_SPLIT, SPEC_HEAD, PRE_WAVE, RESERVE_CUS, AUDIO_WAVE, MIXED_PLAN, SPLIT_CUS = range(10, 19)

OK = (0, "")
# (name, environment, set_option calls, fields that differ from the defaults, return codes of the calls)
CASES = [
    ("nothing set", {}, [], {}, []),
    ("every variable at an ordinary value",
     _env(TP=1, CONV="arith", STEADY=0, PRUNE=0, UNI_ROWS=8, TP_CHUNKS=3, TP_RATIO=1.5, TP_SEGMENT=2048, CORE_SPLIT=0, TP_EAGER=1,
          CORE_LEAD=4, RESERVE_CUS=16, SPLIT_CUS=64, AGC_HINT=0, CORE_DECAY=0, CORE_GUESS=2, CORE_LEAN=0, PRE_WAVE=1, MIXED=0,
          AUDIO_WAVE=0, SPEC_HEAD=0, L64=0, L64_JIT=0, L64_WGS=2, TP_LPW=16), [],
     dict(tp=1, conv=1, steady_blocks=0, prune=0, uni_rows=8, tp_chunks=3, tp_ratio=1.5, tp_L=2048, core_split=0, tp_eager=1,
          core_lead=4, reserve_cus=16, split_cus=64, agc_hint=0, core_decay=0, core_guess=2, core_lean=0, pre_wave=1, mixed=0,
          audio_wave=0, spec_head=0, l64=0, l64_jit=0, l64_wgs=2, tp_lpw=16), []),
    ("every option at an ordinary value", {},
     [(EARLY_INPUT, 1), (STEADY_BLOCKS, 0), (TIME_PARALLEL, 1), (PRUNE_FFT, 0), (U8_CONVERSION, 1), (UNI_ROWS, 8), (TP_CHUNKS, 3),
      (TP_RATIO_PCT, 150), (TP_SEG_LANES, 16), (LANE_FFT, 0), (LANE_FFT_JIT, 0), (CORE_SPLIT, 0), (SPEC_HEAD, 0), (PRE_WAVE, 1),
      (RESERVE_CUS, 16), (AUDIO_WAVE, 0), (MIXED_PLAN, 0), (SPLIT_CUS, 64)],
     dict(early_input=1, steady_blocks=0, tp=1, prune=0, conv=1, uni_rows=8, tp_chunks=3, tp_ratio=1.5, tp_lpw=16, l64=0, l64_jit=0,
          core_split=0, spec_head=0, pre_wave=1, reserve_cus=16, audio_wave=0, mixed=0, split_cus=64), [OK] * 18),
    # TP: the environment knows 0 and 1 only (non-zero is 1), the option has -1 for "auto" as well
    ("TP env 0", _env(TP=0), [], dict(tp=0), []),
    ("TP env 7", _env(TP=7), [], dict(tp=1), []),
    ("TP env -1", _env(TP=-1), [], dict(tp=1), []),
    ("TP option 0", {}, [(TIME_PARALLEL, 0)], dict(tp=0), [OK]),
    ("TP option 7", {}, [(TIME_PARALLEL, 7)], dict(tp=1), [OK]),
    ("TP option -5 after env 1", _env(TP=1), [(TIME_PARALLEL, -5)], dict(tp=-1), [OK]),
    # CONV: first letter a or A is the arithmetic form, anything else the table
    ("CONV lut", _env(CONV="lut"), [], dict(conv=0), []),
    ("CONV arith", _env(CONV="arith"), [], dict(conv=1), []),
    ("CONV Arith", _env(CONV="Arith"), [], dict(conv=1), []),
    ("CONV x", _env(CONV="x"), [], dict(conv=0), []),
    ("CONV option -2 after env arith", _env(CONV="arith"), [(U8_CONVERSION, -2)], dict(conv=-1), [OK]),
    ("CONV option 0", {}, [(U8_CONVERSION, 0)], dict(conv=0), [OK]),
    ("CONV option 3", {}, [(U8_CONVERSION, 3)], dict(conv=1), [OK]),
    # booleans: atoi != 0 / value != 0
    ("booleans read by atoi", _env(L64=2, STEADY="no"), [], dict(steady_blocks=0), []),
    ("PRUNE option -1", {}, [(PRUNE_FFT, 0), (PRUNE_FFT, -1)], {}, [OK, OK]),
    # UNI_ROWS: the environment clamps to 1, the option refuses and leaves the field alone
    ("UNI_ROWS env 0", _env(UNI_ROWS=0), [], dict(uni_rows=1), []),
    ("UNI_ROWS env -7", _env(UNI_ROWS=-7), [], dict(uni_rows=1), []),
    ("UNI_ROWS option 0", {}, [(UNI_ROWS, 0)], {}, [(INVALID, "MI_OPT_UNI_ROWS must be >= 1")]),
    ("UNI_ROWS option 0 after 8", {}, [(UNI_ROWS, 8), (UNI_ROWS, 0), (UNI_ROWS, -1)], dict(uni_rows=8),
     [OK, (INVALID, "MI_OPT_UNI_ROWS must be >= 1"), (INVALID, "MI_OPT_UNI_ROWS must be >= 1")]),
    ("UNI_ROWS option 1", {}, [(UNI_ROWS, 1)], dict(uni_rows=1), [OK]),
    # TP_CHUNKS: the environment's 0 becomes 1, the option's 0 means "default"
    ("TP_CHUNKS env 0", _env(TP_CHUNKS=0), [], dict(tp_chunks=1), []),
    ("TP_CHUNKS env -3", _env(TP_CHUNKS=-3), [], dict(tp_chunks=1), []),
    ("TP_CHUNKS option 0 after env 4", _env(TP_CHUNKS=4), [(TP_CHUNKS, 0)], {}, [OK]),
    ("TP_CHUNKS option -3", _env(TP_CHUNKS=4), [(TP_CHUNKS, -3)], {}, [OK]),
    # TP_RATIO: a factor of at least 0.25 in the environment; a percentage with 0 for "default" as the option
    ("TP_RATIO env 0.1", _env(TP_RATIO=0.1), [], dict(tp_ratio=0.25), []),
    ("TP_RATIO env 0", _env(TP_RATIO=0), [], dict(tp_ratio=0.25), []),
    ("TP_RATIO env 1.375", _env(TP_RATIO=1.375), [], dict(tp_ratio=1.375), []),
    ("TP_RATIO_PCT option 0", _env(TP_RATIO=2), [(TP_RATIO_PCT, 0)], {}, [OK]),
    ("TP_RATIO_PCT option -20", _env(TP_RATIO=2), [(TP_RATIO_PCT, -20)], {}, [OK]),
    ("TP_RATIO_PCT option 10", {}, [(TP_RATIO_PCT, 10)], dict(tp_ratio=0.25), [OK]),
    ("TP_RATIO_PCT option 150", {}, [(TP_RATIO_PCT, 150)], dict(tp_ratio=1.5), [OK]),
    # TP_SEGMENT: one of four lengths, else "by row count"
    ("TP_SEGMENT 300", _env(TP_SEGMENT=300), [], {}, []),
    ("TP_SEGMENT 8192", _env(TP_SEGMENT=8192), [], {}, []),
    ("TP_SEGMENT 512", _env(TP_SEGMENT=512), [], dict(tp_L=512), []),
    ("TP_SEGMENT 1024", _env(TP_SEGMENT=1024), [], dict(tp_L=1024), []),
    ("TP_SEGMENT 4096", _env(TP_SEGMENT=4096), [], dict(tp_L=4096), []),
    # TP_LPW / TP_SEG_LANES: 1 .. 64, else "auto"
    ("TP_LPW env 0", _env(TP_LPW=0), [], {}, []),
    ("TP_LPW env 65", _env(TP_LPW=65), [], {}, []),
    ("TP_LPW env 1", _env(TP_LPW=1), [], dict(tp_lpw=1), []),
    ("TP_LPW env 64", _env(TP_LPW=64), [], dict(tp_lpw=64), []),
    ("TP_SEG_LANES option 65", _env(TP_LPW=8), [(TP_SEG_LANES, 65)], {}, [OK]),
    ("TP_SEG_LANES option 0", _env(TP_LPW=8), [(TP_SEG_LANES, 0)], {}, [OK]),
    ("TP_SEG_LANES option 64", {}, [(TP_SEG_LANES, 64)], dict(tp_lpw=64), [OK]),
    # CORE_LEAD, L64_WGS: not below 0
    ("CORE_LEAD -2", _env(CORE_LEAD=-2, L64_WGS=-2), [], {}, []),
    # CORE_GUESS: 0 .. 2
    ("CORE_GUESS -1", _env(CORE_GUESS=-1), [], dict(core_guess=0), []),
    ("CORE_GUESS 5", _env(CORE_GUESS=5), [], dict(core_guess=2), []),
    # PRE_WAVE: negative is "auto", at most 2, on both routes
    ("PRE_WAVE env -4", _env(PRE_WAVE=-4), [], {}, []),
    ("PRE_WAVE env 7", _env(PRE_WAVE=7), [], dict(pre_wave=2), []),
    ("PRE_WAVE env 0", _env(PRE_WAVE=0), [], dict(pre_wave=0), []),
    ("PRE_WAVE option -4", _env(PRE_WAVE=1), [(PRE_WAVE, -4)], {}, [OK]),
    ("PRE_WAVE option 7", {}, [(PRE_WAVE, 7)], dict(pre_wave=2), [OK]),
    # RESERVE_CUS, SPLIT_CUS: negative is "auto" on both routes
    ("RESERVE_CUS env -9", _env(RESERVE_CUS=-9, SPLIT_CUS=-9), [], {}, []),
    ("RESERVE_CUS env 0", _env(RESERVE_CUS=0, SPLIT_CUS=0), [], dict(reserve_cus=0, split_cus=0), []),
    ("RESERVE_CUS option -9", _env(RESERVE_CUS=8, SPLIT_CUS=8), [(RESERVE_CUS, -9), (SPLIT_CUS, -9)], {}, [OK, OK]),
    ("RESERVE_CUS option 300", {}, [(RESERVE_CUS, 300), (SPLIT_CUS, 300)], dict(reserve_cus=300, split_cus=300), [OK, OK]),
    # a variable that is set but empty counts as unset
    ("empty strings", _env(TP="", CONV="", UNI_ROWS="", TP_RATIO="", L64="", PRE_WAVE=""), [], {}, []),
    # ids that name no option: 0 is the table's mark for an environment-only switch and must not reach one
    ("option ids 0, 19, 99, -1", {}, [(0, 1), (19, 1), (99, 1), (-1, 1)], {}, [(INVALID, "unknown option")] * 4),
    # MI_OPT_EARLY_INPUT has no variable
    ("EARLY_INPUT is not read from the environment", _env(EARLY_INPUT=1, EARLY=1), [], {}, []),
]


@pytest.mark.parametrize("name,env,sets,changed,codes", CASES, ids=[c[0] for c in CASES])
def test_switch_values(probe, name, env, sets, changed, codes):
    fields, got_codes = probe(env, sets)
    assert set(fields) == set(DEFAULTS), "the probe prints every field of mi::Tuning"
    assert got_codes == codes
    assert fields == dict(DEFAULTS, **changed)


def _header_options():
    text = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bMI_OPT_(\w+)\s*=\s*(-?\d+)", text)}


def test_option_ids_agree_between_header_python_and_table(probe, pkg):
    header = _header_options()
    assert len(header) == 18 and len(set(header.values())) == len(header), header
    python = {k[4:]: v for k, v in vars(pkg).items() if k.startswith("OPT_") and isinstance(v, int)}
    assert python == header
    in_source = [k for k in re.findall(r"^OPT_(\w+)\s*=", open(pkg.__file__).read(), re.M)]
    assert in_source == sorted(in_source, key=lambda k: python[k]), "OPT_* are listed in numeric order"
    ids = list(range(-2, 2 * max(header.values()) + 1))
    _, codes = probe({}, [(i, 1) for i in ids])
    accepted = {i for i, (rc, _) in zip(ids, codes) if rc == 0}
    assert accepted == set(header.values())
