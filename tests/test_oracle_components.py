"""Pins the oracle's Squelch / CTCSS / NotchFilter / LowpassFilter restatements:
  - against the committed fixtures generated from the REFERENCE's own compiled sources
    (tests/golden/components_ref.npz, made by tests/golden/gen_golden.py), everywhere;
  - over longer random sweeps and every standard tone, against the reference's answers recorded in
    tests/golden/ref_sweeps.npz (same generator), everywhere.
Bit-exact: flags, squelch level, noise floor, signal level, counters, filter outputs."""
import os

import numpy as np
import pytest

import libs
from golden_inputs import (CTCSS_CASES, FILTER_CASES, SQUELCH_CASES, SQUELCH_SWEEP_SEEDS, digest, make_audio, make_filtered, make_raw,
                           squelch_sweep, tone_bank_inputs)

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "components_ref.npz"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_squelch_case(api, case):
    raw = make_raw(case)
    filt = make_filtered(case, raw) if case.get("filt") else None
    audio = make_audio(case) if case.get("audio") else None
    return api.squelch_run(raw, filt=filt, audio=audio, manual_level=case.get("manual_level", 0.0), snr_db=case.get("snr_db"),
                           ctcss_freq=case.get("ctcss_freq", 0.0), ctcss_rate=case.get("ctcss_rate", 16000))


@pytest.mark.parametrize("name", sorted(SQUELCH_CASES))
def test_squelch_matches_reference_fixture(name):
    res = run_squelch_case(libs.oracle(), SQUELCH_CASES[name])
    for key in ("flags", "level", "noise", "signal"):
        assert np.array_equal(bits(res[key]), bits(GOLD[f"sq_{name}_{key}"])), f"{name}: {key} differs from the reference"
    f = res["final"]
    assert [f.open_count, f.flappy_count, f.ctcss_count, f.no_ctcss_count] == list(GOLD[f"sq_{name}_final_counts"])
    assert np.array_equal(bits(np.array([f.noise_level, f.signal_level, f.squelch_level], np.float32)), bits(GOLD[f"sq_{name}_final_levels"]))


def test_fixture_exercises_the_state_machine():
    """The fixtures must actually reach the interesting corners, otherwise equality proves little."""
    assert GOLD["sq_flap_final_counts"][1] > 0          # flappy_count: flap detection engaged
    assert GOLD["sq_ctcss_good_final_counts"][2] > 0    # ctcss found
    assert GOLD["sq_ctcss_wrong_final_counts"][3] > 0   # ctcss rejected
    assert (GOLD["sq_bursts_filt_flags"] & 32).any()    # signal_outside_filter seen
    states_open = (GOLD["sq_dropout_flags"] & 1).astype(bool)
    assert states_open.any() and not states_open.all()
    assert (GOLD["sq_dropout_flags"] & 16).sum() >= 2   # last_open_sample fired (incl. a low-signal abort)


@pytest.mark.parametrize("name", sorted(CTCSS_CASES))
def test_ctcss_matches_reference_fixture(name):
    case = CTCSS_CASES[name]
    flags, found, nfound = libs.oracle().ctcss_run(case["freq"], case["rate"], case["window"], make_audio(case))
    assert np.array_equal(flags, GOLD[f"ct_{name}_flags"])
    assert [found, nfound] == list(GOLD[f"ct_{name}_counts"])


@pytest.mark.parametrize("name", sorted(FILTER_CASES))
def test_filters_match_reference_fixture(name):
    case = FILTER_CASES[name]
    rng = np.random.default_rng(case["seed"])
    x = rng.normal(size=case["n"]).astype(np.float32)
    y = rng.normal(size=case["n"]).astype(np.float32)
    o = libs.oracle()
    if case["kind"] == "notch":
        assert np.array_equal(bits(o.notch_run(case["freq"], 16000.0, case["q"], x)), bits(GOLD[f"fl_{name}_y"]))
    else:
        a, b = o.lowpass_run(case["freq"], 16000.0, x, y)
        assert np.array_equal(bits(a), bits(GOLD[f"fl_{name}_re"]))
        assert np.array_equal(bits(b), bits(GOLD[f"fl_{name}_im"]))


def test_tone_generator_matches_reference_fixture():
    assert np.array_equal(bits(libs.oracle().tone_run(8000, 79.7, 0.2, 4000)), bits(GOLD["tone_79_7"]))


# ---------- the longer sweeps, against the reference's recorded answers (tests/golden/ref_sweeps.npz) ----------

SWEEPS = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_sweeps.npz"))


@pytest.mark.parametrize("seed", SQUELCH_SWEEP_SEEDS)
def test_squelch_random_vs_live_reference(seed):
    """Random bursts under every squelch mode; the compiled reference's outputs were recorded as digests by gen_golden.py."""
    raw, kws = squelch_sweep(seed)
    o = libs.oracle()
    for i, kw in enumerate(kws):
        a = o.squelch_run(raw, **kw)
        for key in ("flags", "level", "noise", "signal"):
            assert np.array_equal(digest(bits(a[key])), SWEEPS[f"sw{seed}_{i}_{key}"]), (seed, list(kw), key)
        f = a["final"]
        assert [f.open_count, f.flappy_count, f.ctcss_count, f.no_ctcss_count] == list(SWEEPS[f"sw{seed}_{i}_final_counts"]), (seed, list(kw))
        assert np.array_equal(bits(np.array([f.noise_level, f.signal_level, f.squelch_level], np.float32)),
                              bits(SWEEPS[f"sw{seed}_{i}_final_levels"])), (seed, list(kw))


def test_every_standard_tone_bank_vs_live_reference():
    """Detector-bank construction (dedupe by coefficient, +-5 Hz exclusion) for every standard tone."""
    tones = SWEEPS["standard_tones"]
    assert tones.size == 51
    o = libs.oracle()
    n = 0
    for (t, rate, win, x), want_flags, want_counts in zip(tone_bank_inputs(tones), SWEEPS["tone_bank_flags"], SWEEPS["tone_bank_counts"]):
        flags, found, nfound = o.ctcss_run(t, rate, win, x)
        assert np.array_equal(digest(flags), want_flags) and [found, nfound] == list(want_counts), (t, rate, win)
        n += 1
    assert n == len(SWEEPS["tone_bank_counts"]) == tones.size * 2


def test_default_filters_disabled_in_reference():
    assert int(SWEEPS["filters_default_disabled"]) == 1  # src/test_filters.cpp:33-41, as the compiled reference answered
    # the oracle's counterpart: a filter set up without a frequency passes its input through untouched
    rng = np.random.default_rng(3)
    x, y = rng.normal(size=(2, 1000)).astype(np.float32)
    o = libs.oracle()
    assert np.array_equal(bits(o.notch_run(0.0, 16000.0, 10.0, x)), bits(x))
    a, b = o.lowpass_run(0.0, 16000.0, x, y)
    assert np.array_equal(bits(a), bits(x)) and np.array_equal(bits(b), bits(y))
