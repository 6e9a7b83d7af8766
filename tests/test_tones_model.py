"""The CTCSS tone finder's definition, pinned without a GPU: the model of tones_model.py against the CPU oracle's (and, where it is
built, the reference's own) CTCSS decision for every one of the 51 targets; mi_tones_table against the plan and the model; then
mi_tones_plan_host (csrc/poststage_host.cpp) against the model -- records, powers and the state blob as bytes --, the vote, the
exported symbols and the refusals; and a generated NFM capture with and without a 100 Hz tone through the oracle, the twin and the vote."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import libs
from common import bytes_for_batches, oracle_run
from tones_model import (DEFAULT_WINDOW, LANES, LONG_PRELUDE, LONG_ROWS, NO_SIGNAL, NTONES, RECORD, STANDARD_TONES, STATE, WAVE_BATCH, WAVE_RATE,
                         alias_of, coeffs, detector_set, draw_audio, draw_flags, fresh_state, full_scale_audio, has_tone, long_call_masks,
                         long_call_planes, run_in_calls, silence, tone_audio, tones_model, two_tone_audio, vote)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TONES_SYMBOLS = {"mi_tones_create", "mi_tones_destroy", "mi_tones_set_rows", "mi_tones_process_device", "mi_tones_download", "mi_tones_state_size",
                 "mi_tones_get_state", "mi_tones_set_state", "mi_tones_set_timing", "mi_tones_last_launch_ms", "mi_tones_plan_host", "mi_tones_table",
                 "mi_tones_vote_host"}
SENT = 0xA5
STAR = ord("*")
# the generated capture of the end-to-end cases (here and in test_gpu_tones.py): two NFM channels, bandwidth 12500, no ctcss configured;
# a kind-2 carrier (1 kHz tone + 100 Hz CTCSS) on the first and a kind-1 carrier (1 kHz tone alone) on the second, both off for 12
# batches and on for 12, so that the squelch opens on a settled noise floor
E2E_BATCHES, E2E_GATE_BATCHES = 24, 12


def e2e_setup(pkg):
    centre = 120000000
    dev = pkg.device_cfg(centerfreq=centre)
    offsets = (250000, -250000)
    chans = [pkg.channel_cfg(centre + o, modulation=pkg.MOD_NFM, bandwidth=12500) for o in offsets]
    carriers = [(offsets[0], 2, 3072, 0), (offsets[1], 1, 3072, 0)]
    nbytes = (bytes_for_batches(dev, E2E_BATCHES) + 255) // 256 * 256
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate * E2E_GATE_BATCHES * WAVE_BATCH // WAVE_RATE, carriers=carriers)
    return dev, chans, cfg, nbytes


def e2e_verdict(pkg, records, row_first):
    """the vote on either row under the defaults, by the library and by the model: 100.0 found on row 0, nothing found on row 1"""
    votes = []
    for r in range(2):
        mine = records[row_first[r]:row_first[r + 1]]
        v = pkg.tones_vote_host(mine)
        assert (v.windows, v.votes, v.tone, v.freq_hz, v.share, v.found) == vote(mine)
        print(f"row {r}: best / mean per window {[(int(x['best']), round(float(x['best_power'] / x['mean_power']), 2)) for x in mine]}, "
              f"{v.votes} of {v.windows} windows for tone {v.tone} ({v.freq_hz} Hz), found {v.found}")
        votes.append(v)
    assert votes[0].found == 1 and votes[0].freq_hz == 100.0 and votes[0].tone == 12 and votes[0].windows >= 2
    assert votes[1].found == 0 and votes[1].windows >= 2
    return votes


# ---------------- the model against the oracle ----------------

def oracle_inputs(window):
    """three windows each of four table tones in noise, and of noise alone"""
    rng = np.random.default_rng(window)
    n = 3 * window
    return {f: tone_audio(rng, n, f, amp=0.1 if f else 0.0, sigma=0.05) for f in (100.0, 151.4, 67.0, 254.1, 0.0)}


def decisions_against(api, window):
    """mismatches between `api`'s CTCSS decision and the model's, over every target, input and window"""
    bad, checked, positive = [], 0, 0
    for name, x in oracle_inputs(window).items():
        axc = np.full((1, -(-len(x) // WAVE_BATCH)), STAR, np.uint8)
        wave = np.zeros((1, axc.shape[1] * WAVE_BATCH), np.float32)
        wave[0, :len(x)] = x
        rec, powers, _, _ = tones_model(axc, wave, window=window)
        assert len(rec) >= 3
        for target in range(NTONES):
            chosen = detector_set(target, window)
            assert len(chosen) == libs.oracle_lib().ao_ctcss_detector_count(float(STANDARD_TONES[target]), float(WAVE_RATE), window)
            flags, found, not_found = api.ctcss_run(float(STANDARD_TONES[target]), float(WAVE_RATE), window, x)
            assert found + not_found == 3
            for w in range(3):
                want = bool(flags[(w + 1) * window - 1] & 1)
                got = has_tone(powers[w, :NTONES], chosen)
                checked += 1
                positive += want
                if want != got:
                    bad.append((name, target, w))
    return bad, checked, positive


@pytest.mark.parametrize("window", [DEFAULT_WINDOW, 800])
def test_model_powers_reproduce_the_oracle_s_decision_for_every_target(window):
    """From the bank's 51 powers the oracle's detector set is rebuilt for each target -- the target first, then the table's tones at
    least 5 Hz away, without coefficient duplicates, summed in that order --: the decision equals ao_ctcss_run's in every window."""
    bad, checked, positive = decisions_against(libs.oracle(), window)
    print(f"window {window}: {checked} decisions, {positive} of them 'tone present', {len(bad)} mismatches")
    assert checked == 51 * 3 * 5 and positive >= 12 and not bad, bad[:10]
    ref = libs.ref()
    if ref is not None:  # the reference's own ctcss.cpp, where it is built
        bad, checked, _ = decisions_against(ref, window)
        assert checked == 51 * 3 * 5 and not bad, bad[:10]


def test_noise_alone_needs_the_vote():
    """on noise alone the strongest of the 51 powers is several times their mean, so `best > mean` in one window is no detection"""
    rng = np.random.default_rng(11)
    n = 6 * DEFAULT_WINDOW
    wave = tone_audio(rng, n // WAVE_BATCH * WAVE_BATCH + WAVE_BATCH, 0.0, amp=0.0)[None]
    rec, _, _, _ = tones_model(np.full((1, wave.shape[1] // WAVE_BATCH), STAR, np.uint8), wave)
    ratio = rec["best_power"] / rec["mean_power"]
    print("best / mean on noise alone:", ratio)
    assert len(rec) == 6 and (ratio > 2.0).all() and vote(rec)[5] == 0


@pytest.mark.parametrize("window,distinct", [(800, 11), (2000, 25), (3200, 37), (6400, 51), (64000, 51)])
def test_table_against_the_plan_and_the_model(pkg, window, distinct):
    freq, coeff, alias = pkg.tones_table(window)
    assert freq.tobytes() == STANDARD_TONES.tobytes()
    assert coeff.tobytes() == coeffs(window).tobytes()
    assert np.array_equal(alias, alias_of(window)) and len(set(alias.tolist())) == distinct == len(set(coeff.tolist()))
    assert all(alias[t] <= t and coeff[alias[t]] == coeff[t] for t in range(NTONES))
    if window == DEFAULT_WINDOW:  # the plan's slow window: entry 0 of a channel's detector set is its target's coefficient
        d0, c0, a0 = pkg.tones_table(0)
        assert c0.tobytes() == coeff.tobytes() and np.array_equal(a0, alias)
        for t in range(NTONES):
            plan = pkg.Plan(pkg.device_cfg(), [pkg.channel_cfg(120000000, modulation=pkg.MOD_NFM, ctcss=float(freq[t]))])
            assert plan.channel(0).ctcss_slow_window == window
            assert np.float32(plan.ctcss_coeffs(0, True)[0]).tobytes() == coeff[t].tobytes(), t
            plan.close()
    if window == 800:  # ... and its fast window
        plan = pkg.Plan(pkg.device_cfg(), [pkg.channel_cfg(120000000, modulation=pkg.MOD_NFM, ctcss=100.0)])
        assert plan.channel(0).ctcss_fast_window == 800 and np.float32(plan.ctcss_coeffs(0, False)[0]).tobytes() == coeff[12].tobytes()
        plan.close()


# ---------------- mi_tones_plan_host against the model ----------------

def case(rows, nb, window, seed=0, p_open=0.85):
    rng = np.random.default_rng([seed, rows, nb, window])
    axc = draw_flags(rng, rows, nb, p_open)
    axc[0] = STAR  # one row without a reset
    return axc, draw_audio(rng, rows, nb * WAVE_BATCH)


def assert_twin_equals_model(pkg, axc, wave, window, cuts, what, enabled=None, masks=None, calls=None):
    """masks: the enabled rows of each call; calls: the model's run_in_calls over the same arguments, where the caller has it already"""
    rows = axc.shape[0]
    masks = [np.ones(rows, np.uint8) if enabled is None else enabled] * len(cuts) if masks is None else masks
    calls, want_state = run_in_calls(axc, wave, cuts, window, masks=masks) if calls is None else calls
    state, total = None, 0
    for n, en, (done, want_rec, want_pw, want_first, want_after) in zip(cuts, masks, calls):
        rec, pw, first, count, state = pkg.tones_plan_host(en, axc[:, done:done + n], wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], state, window)
        assert tuple(count) == (len(want_rec), len(want_rec)), f"{what} at batch {done}: counts {count} vs {len(want_rec)}"
        assert np.array_equal(first, want_first), f"{what} at batch {done}: row_first_record"
        assert rec.tobytes() == want_rec.tobytes(), f"{what} at batch {done}: records\n{rec}\n{want_rec}"
        assert pw.tobytes() == want_pw.tobytes(), f"{what} at batch {done}: powers"
        assert state.tobytes() == want_after.tobytes(), f"{what} at batch {done}: state blob"
        total += len(rec)
    return total, want_state


@pytest.mark.parametrize("window", [800, 2000, 6400, 64000])
@pytest.mark.parametrize("rows", [1, 5])
def test_plan_host_equals_the_model(pkg, rows, window):
    """16 batches as one call, as 16 calls and as 3 + 5 + 8: at 2000 a window ends on a batch's last sample, 64000 is longer than
    the call (no record, the state alone)"""
    axc, wave = case(rows, 16, window)
    totals = []
    for cuts in ((16,), (1,) * 16, (3, 5, 8)):
        total, state = assert_twin_equals_model(pkg, axc, wave, window, cuts, f"{rows} rows, window {window}, cuts {cuts}")
        totals.append((total, state.tobytes()))
    assert totals[0] == totals[1] == totals[2], "a call cut anywhere changes nothing"
    assert (totals[0][0] == 0) == (window == 64000)
    if window == 64000:
        assert int(state[0]["count"]) == 16 * WAVE_BATCH and state[0]["q1"][:NTONES].any()
    if window == 2000:
        rec = tones_model(axc, wave, window=window)[0]
        assert (rec["end_sample"] == WAVE_BATCH - 1).all() and list(rec["seq"][rec["row"] == 0]) == list(range(16))


LONG_NB = [64, 65, 128, 130]
LONG_WINDOWS = [800, 2000, 6400, 64000]


def assert_long_call_conditions(nb, window, calls):
    """What makes long_call_planes worth running, from the model's two calls alone (here and before the device runs them)"""
    prelude, (_, rec, _, first, after) = calls[0][4], calls[1]
    of = lambda name: rec[first[LONG_ROWS[name]]:first[LONG_ROWS[name] + 1]]
    ends = lambda name: [(int(x["seq"]), int(x["end_batch"]), int(x["end_sample"])) for x in of(name)]
    assert (prelude["count"] == LONG_PRELUDE * WAVE_BATCH % window).all() and (prelude["seq"] == LONG_PRELUDE * WAVE_BATCH // window).all()
    a = of("A")
    assert len(a) == (int(prelude[0]["count"]) + nb * WAVE_BATCH) // window
    if window == 800:
        assert len(a) >= 129, "three trips of the walk's window loop"
    if window == 64000 and nb >= 128:
        end = a["end_batch"].astype(np.int64) * WAVE_BATCH + a["end_sample"]
        assert ((end - window < 64 * WAVE_BATCH) & (64 * WAVE_BATCH <= end)).any(), "a window across the boundary of the walk's trips"
    b = LONG_ROWS["B"]
    assert len(of("B")) == 0 and after[b]["count"] == 0 and not after[b]["q1"].any() and not after[b]["q2"].any()
    assert prelude[b]["q1"].any() == (LONG_PRELUDE * WAVE_BATCH % window != 0), "where the prelude leaves a count, the reset has something to clear"
    c, d = LONG_ROWS["C"], LONG_ROWS["D"]
    rowless = lambda x: np.rec.fromarrays([x[n] for n in RECORD.names[1:]]).tobytes()
    assert len(of("C")) and len(of("D")) and rowless(of("C")) != rowless(of("D"))
    # ... and not by their audio alone: the windows end elsewhere, or (no window ends behind batch 63) the counts left differ
    assert ends("C") != ends("D") or (window > 2000 and after[c]["count"] != after[d]["count"])
    e = LONG_ROWS["E"]
    assert int(after[e]["count"]) == ((min(nb, 67) - 62) * WAVE_BATCH % window if nb <= 67 else 0)
    assert bool(after[e]["q1"].any()) == bool(after[e]["count"])
    i = LONG_ROWS["I"]
    assert len(of("I")) == 0 and after[i].tobytes() == prelude[i].tobytes() and len(prelude[i].tobytes()) == 520 and any(prelude[i].tobytes())


@pytest.mark.parametrize("window", LONG_WINDOWS)
@pytest.mark.parametrize("nb", LONG_NB)
def test_plan_host_equals_the_model_past_64_batches(pkg, nb, window):
    """long_call_planes as a 3-batch call and one of 64, 65, 128 or 130 on one state: the rows the device's walk takes in more than one
    64-batch trip -- whole trips of signal, a reset on either side of the trip boundary, a run across it, a silent first trip -- with
    the conditions that make them so asserted from the model"""
    axc, wave = long_call_planes(nb, window)
    cuts, masks = (LONG_PRELUDE, nb), long_call_masks()
    calls = run_in_calls(axc, wave, cuts, window, masks=masks)
    assert_long_call_conditions(nb, window, calls[0])
    assert_twin_equals_model(pkg, axc, wave, window, cuts, f"long call of {nb}, window {window}", masks=masks, calls=calls)


def test_reset_one_batch_before_a_window_completes(pkg):
    """window 6400 = 3.2 batches: a NO_SIGNAL batch at 3 throws three batches of samples away, and the window count goes on from 0"""
    rng = np.random.default_rng(3)
    axc = np.full((2, 12), STAR, np.uint8)
    axc[1, 3] = NO_SIGNAL
    wave = np.stack([tone_audio(rng, 12 * WAVE_BATCH, 100.0)] * 2)
    assert_twin_equals_model(pkg, axc, wave, DEFAULT_WINDOW, (12,), "reset")
    assert_twin_equals_model(pkg, axc, wave, DEFAULT_WINDOW, (3, 1, 8), "reset, cut at the reset")
    rec, _, first, _ = tones_model(axc, wave)
    assert list(np.diff(first)) == [3, 2]
    assert [(int(x["end_batch"]), int(x["end_sample"]), int(x["seq"])) for x in rec[3:]] == [(7, 399, 0), (10, 799, 1)]
    assert (rec["best"] == 12).all()


def test_disabled_rows_keep_every_byte_of_their_state(pkg):
    axc, wave = case(5, 8, 2000, seed=4)
    state = tones_model(*case(5, 3, 2000, seed=5), window=6400)[3]  # mid-window: counts 6000 here would be refused at window 2000
    state["count"] %= 2000
    en = np.array([1, 0, 1, 0, 1], np.uint8)
    want_rec, want_pw, want_first, want_after = tones_model(axc, wave, state, en, 2000)
    rec, pw, first, count, after = pkg.tones_plan_host(en, axc, wave, state, 2000)
    assert rec.tobytes() == want_rec.tobytes() and pw.tobytes() == want_pw.tobytes() and after.tobytes() == want_after.tobytes()
    before, after = state.view(np.uint8).reshape(5, 520), after.reshape(5, 520)
    assert np.array_equal(before[en == 0], after[en == 0]) and before[1].any() and not np.array_equal(before[0], after[0])
    assert set(rec["row"]) == {0, 2, 4} and first[1] == first[2] and first[3] == first[4]


def raw_plan(pkg, axc, wave, window, cap, room, state=None, powers=True, en=None):
    """mi_tones_plan_host through ctypes with buffers of `room` records, told `cap`, every byte SENT beforehand"""
    rows, nb = axc.shape
    state = np.zeros(rows * 520, np.uint8) if state is None else state
    rec = np.full(room * 40, SENT, np.uint8)
    pw = np.full(room * LANES * 4, SENT, np.uint8)
    first, count = np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().mi_tones_plan_host(C.byref(pkg.TonesCfg(window)), p(np.ones(rows, np.uint8) if en is None else en), rows, p(axc), nb, nb, p(wave),
                                      0 if wave is None else wave.shape[1], p(state), p(rec), p(pw) if powers else None, cap, p(first), p(count))
    return rc, rec, pw, first, count, state


def test_capacity_short_of_the_total_and_sentinels(pkg):
    axc, wave = case(3, 8, 800, seed=6)
    want, want_pw, want_first, want_state = tones_model(axc, wave, window=800)
    cap = len(want) // 2
    assert cap >= 2
    rc, rec, pw, first, count, state = raw_plan(pkg, axc, wave, 800, cap, cap + 3)
    assert rc == pkg.MI_OK and tuple(count) == (len(want), cap)
    assert rec[:cap * 40].tobytes() == want[:cap].tobytes() and (rec[cap * 40:] == SENT).all(), "records behind the capacity"
    assert pw[:cap * 256].tobytes() == want_pw[:cap].tobytes() and (pw[cap * 256:] == SENT).all(), "powers behind the capacity"
    assert np.array_equal(first, want_first) and state.tobytes() == want_state.tobytes()
    rc, rec, pw, _, count, _ = raw_plan(pkg, axc, wave, 800, len(want) + 2, len(want) + 2, powers=False)
    assert rc == pkg.MI_OK and rec[:len(want) * 40].tobytes() == want.tobytes() and (rec[len(want) * 40:] == SENT).all() and (pw == SENT).all()


def test_special_inputs(pkg):
    """silence: every power 0, best 0 and second 1 by the tie rule, no vote; full scale: finite powers; two tones: best and second"""
    rng = np.random.default_rng(7)
    n = 4 * WAVE_BATCH
    wave = np.stack([silence(n), full_scale_audio(rng, n), two_tone_audio(rng, n, 123.0, 203.5)])
    axc = np.full((3, 4), STAR, np.uint8)
    total, _ = assert_twin_equals_model(pkg, axc, wave, DEFAULT_WINDOW, (4,), "special inputs")
    rec = tones_model(axc, wave)[0]
    assert total == 3 and tuple(rec[0])[4:9] == (0, 1, 0.0, 0.0, 0.0) and vote(rec[:1], min_windows=1)[5] == 0
    assert np.isfinite(rec["best_power"]).all() and rec[1]["best_power"] > 0
    assert (int(rec[2]["best"]), int(rec[2]["second"])) == (18, 41)
    alias = alias_of(800)
    rec8 = tones_model(axc, wave, window=800)[0]
    assert (alias[rec8["best"]] == rec8["best"]).all(), "of an alias group the first one is named"


# ---------------- fixed checks ----------------

def records_of(best, strong):
    rec = np.zeros(len(best), RECORD)
    rec["best"], rec["mean_power"] = best, 1.0
    rec["best_power"] = np.where(strong, 2.0, 1.0)  # equal to the mean is no vote: the comparison is strict
    return rec


@pytest.mark.parametrize("best,strong,kw,want", [
    ([12, 12, 12, 12], [1, 1, 1, 1], {}, (4, 4, 12, 100.0, 1.0, 1)),
    ([12, 12, 3, 4], [1, 1, 1, 1], {}, (4, 2, 12, 100.0, 0.5, 1)),             # exactly the share
    ([12, 12, 3, 4, 5], [1, 1, 1, 1, 1], {}, (5, 2, 12, 100.0, 0.4, 0)),       # short of it
    ([12], [1], {}, (1, 1, 12, 100.0, 1.0, 0)),                                # one window is not enough by default
    ([12], [1], dict(min_windows=1), (1, 1, 12, 100.0, 1.0, 1)),
    ([30, 7, 30, 7], [1, 1, 1, 1], {}, (4, 2, 7, 85.4, 0.5, 1)),               # a tie goes to the lowest index
    ([12, 12, 12], [0, 0, 0], {}, (3, 0, 0, 0.0, 0.0, 0)),                     # no window votes
    ([12, 12, 12, 5], [1, 1, 1, 0], dict(min_share_permille=750), (4, 3, 12, 100.0, 0.75, 1)),
    ([12, 12, 12, 5], [1, 1, 1, 0], dict(min_share_permille=751), (4, 3, 12, 100.0, 0.75, 0)),
    ([], [], {}, (0, 0, 0, 0.0, 0.0, 0)),
])
def test_vote_at_its_thresholds_and_ties(pkg, best, strong, kw, want):
    rec = records_of(np.array(best, np.uint32), np.array(strong, bool))
    want = want[:3] + (float(np.float32(want[3])),) + want[4:]  # the table holds floats
    assert vote(rec, **{"min_windows": 2, "min_share_permille": 500, **kw}) == want
    v = pkg.tones_vote_host(rec, **kw)
    assert (v.windows, v.votes, v.tone, v.freq_hz, v.share, v.found) == want


def test_refusals(pkg):
    axc, wave = case(2, 3, 800, seed=8)
    assert raw_plan(pkg, axc, wave, 800, 16, 16)[0] == pkg.MI_OK
    assert raw_plan(pkg, axc, wave, 0, 16, 16)[0] == pkg.MI_OK, "0 is the default window"
    for window in (799, 64001, 1):
        assert raw_plan(pkg, axc, wave, window, 16, 16)[0] == pkg.MI_ERR_INVALID
        assert b"window" in pkg.lib().mi_last_error()
    assert raw_plan(pkg, axc, wave, 800, 0, 16)[0] == pkg.MI_ERR_INVALID
    assert raw_plan(pkg, axc, None, 800, 16, 16)[0] == pkg.MI_ERR_INVALID, "the audio is required"
    assert raw_plan(pkg, axc, np.zeros((2, 3 * WAVE_BATCH - 4), np.float32), 800, 16, 16)[0] == pkg.MI_ERR_INVALID
    bad = fresh_state(2)
    bad[1]["count"] = 800
    assert raw_plan(pkg, axc, wave, 800, 16, 16, state=bad.view(np.uint8).reshape(-1).copy())[0] == pkg.MI_ERR_INVALID
    assert b"state" in pkg.lib().mi_last_error()
    bad[1]["count"] = 799
    assert raw_plan(pkg, axc, wave, 800, 16, 16, state=bad.view(np.uint8).reshape(-1).copy())[0] == pkg.MI_OK
    for field, lane, value in (("q1", 51, 1.0), ("q2", 63, -0.0)):  # a padding lane, even a negative zero
        bad = fresh_state(2)
        bad[0][field][lane] = value
        assert raw_plan(pkg, axc, wave, 800, 16, 16, state=bad.view(np.uint8).reshape(-1).copy())[0] == pkg.MI_ERR_INVALID
    for bad_window in (1, 70000):
        with pytest.raises(pkg.MiError) as e:
            pkg.tones_table(bad_window)
        assert e.value.code == pkg.MI_ERR_INVALID
    rec = records_of(np.array([51], np.uint32), np.array([True]))
    for kw, r in ((dict(), rec), (dict(min_share_permille=1001), rec[:0])):
        with pytest.raises(pkg.MiError) as e:
            pkg.tones_vote_host(r, **kw)
        assert e.value.code == pkg.MI_ERR_INVALID
    if pkg.device_count() == 0:  # create is refused before anything else where no device is
        with pytest.raises(pkg.MiError) as e:
            pkg.Tones([1, 1], max_batches=4)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE
    for kw in (dict(window=700), dict(max_batches=0), dict(max_batches=(1 << 20) + 1), dict(window=800, max_batches=1 << 20)):
        with pytest.raises(pkg.MiError) as e:  # the argument checks come before the device is looked for
            pkg.Tones(np.ones(8), **{"max_batches": 4, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID, kw


def test_library_exports_the_tone_finder_s_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    assert re.search(r"\bMI_TONES_STANDARD = 51, MI_TONES_LANES = 64, MI_TONES_STATE_ROW_BYTES = 520\b", header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_tones_")}
    assert declared == TONES_SYMBOLS
    lib = pkg.lib()
    assert not [s for s in sorted(declared) if not hasattr(lib, s)]
    assert declared <= set(pkg.ABI_SYMBOLS)
    assert C.sizeof(pkg.ToneRecord) == 40 == pkg.TONE_RECORD_DTYPE.itemsize == RECORD.itemsize and C.sizeof(pkg.TonesCfg) == 4
    assert pkg.TONES_STATE_DTYPE.itemsize == 520 == STATE.itemsize and C.sizeof(pkg.TonesVote) == 32 and C.sizeof(pkg.TonesRule) == 8
    assert [(n, pkg.TONE_RECORD_DTYPE.fields[n][1]) for n in pkg.TONE_RECORD_DTYPE.names] == [(n, RECORD.fields[n][1]) for n in RECORD.names]
    assert (pkg.TONES_STANDARD, pkg.TONES_LANES) == (NTONES, LANES)


# ---------------- end to end on the CPU ----------------

def test_end_to_end_capture_through_the_oracle_the_twin_and_the_vote(pkg):
    """The generated capture through the CPU oracle, then mi_tones_plan_host over its audio and flags, then the vote: tone 100.0 on the
    row whose carrier has it and nothing on the plain NFM row, under the default window and the default rule."""
    dev, chans, cfg, nbytes = e2e_setup(pkg)
    n, wo, axc, _ = oracle_run(dev, chans, pkg.iqgen_host(cfg, 0, 0, nbytes // 2), E2E_BATCHES)
    assert n == E2E_BATCHES
    print("flags:", [bytes(a).decode() for a in axc])
    rec, pw, first, count, state = pkg.tones_plan_host(np.ones(2), axc, wo)
    want = tones_model(axc, wo)
    assert rec.tobytes() == want[0].tobytes() and pw.tobytes() == want[1].tobytes() and state.tobytes() == want[3].tobytes()
    e2e_verdict(pkg, rec, first)
