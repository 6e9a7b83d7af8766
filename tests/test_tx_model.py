"""The transmission splitter's rule, pinned without a GPU: the model of tx_model.py on its own (the hand cases literally, what each
flag family provokes, calls cut anywhere), then mi_tx_plan_host (csrc/plan.cpp) against it -- records as bytes, state blob, counts and
row_first_record -- and the exported symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tx_model import (BURST_SHAPES, DEFAULT_CFG, FAMILIES, HAND_CASES, NONE, RECORD, SMALL_CFG, STATE, block_energy, draw_audio, draw_bursts,
                      draw_family, features, flags_of, fresh_state, letters, run_in_calls, tx_model)
from gate_model import NO_SIGNAL, WAVE_BATCH, gate_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TX_SYMBOLS = {"mi_txsplit_create", "mi_txsplit_destroy", "mi_txsplit_set_rows", "mi_txsplit_process_device", "mi_txsplit_download",
              "mi_txsplit_state_size", "mi_txsplit_get_state", "mi_txsplit_set_state", "mi_txsplit_set_timing", "mi_txsplit_last_launch_ms",
              "mi_tx_plan_host"}
SENT = 0xA5


# ---------------- the model alone ----------------

def test_thresholds_follow_from_the_reference_s_constants():
    assert DEFAULT_CFG == (8, 4, 28800)
    assert 8 * 2000 == 1.0 * 16000 and 4 * 2000 == 0.5 * 16000 and 28800 * 2000 == 3600 * 16000


@pytest.mark.parametrize("case", range(len(HAND_CASES)))
def test_hand_cases(case):
    text, cfg, want_letters, want_closes = HAND_CASES[case]
    assert len(text) == len(want_letters)
    rec, first, state, file_of, closes = tx_model(flags_of(text), cfg=cfg)
    assert letters(file_of[0]) == want_letters
    assert [b for _, b, _ in closes] == want_closes
    assert list(first) == [0, len(rec)] and list(rec["seq"]) == list(range(1, len(rec) + 1))
    assert [int(c) for c in rec["close_batch"] if c != NONE] == want_closes
    assert int(rec["nblocks"].sum()) == len(text) - want_letters.count(".")
    assert int(state[0]["clock"]) == len(text)


def test_hand_cases_spelt_out():
    """the strings of the issue, literally"""
    got = [letters(tx_model(flags_of(t), cfg=c)[3][0]) for t, c, _, _ in HAND_CASES]
    assert got[0] == "aaa...........b"
    assert got[1] == "aaa....aaa......"
    assert got[2] == "aaa.....aaa....."
    assert got[3] == "aaaaaaaaaaaaa..aaaa......."
    assert got[4] == "aaaaaaaaaaaaa.....bbbb........"
    assert got[5] == "aaaaaaaaaaabbbbbbbbbbbcccccccc"


def test_travelling_set_is_the_gate_s_open_trail_rule():
    rng = np.random.default_rng(3)
    for fam in FAMILIES:
        axc = draw_family(fam, rng, 5, 130)
        _, _, _, file_of, _ = tx_model(axc, cfg=SMALL_CFG)
        index, _, _ = gate_model(np.full(5, 2, np.uint8), axc)
        assert [(r, b) for r, b in zip(*np.nonzero(file_of))] == [tuple(int(v) for v in x) for x in index], fam


def test_every_family_does_its_job():
    rng = np.random.default_rng(4)
    seen = dict(idle_close=False, appended=False, max_split=False, empty_record=False, across_calls=False)
    assert not tx_model(draw_family("p0", rng, 3, 65))[0].size, "no signal, no file"
    rec = tx_model(draw_family("p100", rng, 3, 65), cfg=SMALL_CFG)[0]
    assert (rec["nblocks"][rec["close_batch"] != NONE] == SMALL_CFG[2] + 1).all() and len(rec) == 3 * 6, "an unbroken signal splits at max only"
    for fam, cfg, cuts in (("bursts", DEFAULT_CFG, (40, 25)), ("bursts", SMALL_CFG, (1, 63, 1)), ("p05", DEFAULT_CFG, (65,)), ("p50", SMALL_CFG, (33, 32))):
        got = features(draw_family(fam, rng, 3, 65), cuts, cfg)
        print(fam, cfg, cuts, got)
        for k, v in got.items():
            seen[k] |= v
    bursts = features(draw_bursts(rng, 8, 130), (130,), DEFAULT_CFG)
    assert bursts["idle_close"] and bursts["appended"], "the gaps graze idle > 4 and duration > 8 from both sides"
    assert all(seen.values()), seen
    # a file left open by one call and closed by the silence of the next: a record without blocks
    axc = flags_of("*" * 10 + " " * 10)
    calls, _, _, _ = run_in_calls(axc, (12, 8))
    rec = calls[1][1]
    assert len(rec) == 1 and rec[0]["nblocks"] == 0 and rec[0]["flags"] == 1 and rec[0]["close_batch"] == 15 - 12 and rec[0]["first_batch"] == NONE


def assert_cut_changes_nothing(axc, cuts, cfg):
    _, state, file_of, closes = run_in_calls(axc, (axc.shape[1],), cfg)
    calls, cut_state, cut_file_of, cut_closes = run_in_calls(axc, cuts, cfg)
    assert np.array_equal(file_of, cut_file_of) and closes == cut_closes, cuts
    assert state.tobytes() == cut_state.tobytes(), cuts
    for r in range(axc.shape[0]):  # the records of the calls, per row in order, name the same blocks of the same files
        mine = [(int(x["seq"]), done + int(x["first_batch"]), int(x["nblocks"])) for done, rec, _ in calls for x in rec if x["row"] == r and x["nblocks"]]
        assert sum(n for _, _, n in mine) == int((file_of[r] > 0).sum())
        for seq, first, n in mine:
            written = np.flatnonzero(file_of[r])
            assert (file_of[r][written[written >= first][:n]] == seq).all()


def test_a_call_cut_anywhere_changes_nothing():
    rng = np.random.default_rng(5)
    axc = draw_bursts(rng, 2, 60)
    for cfg in (DEFAULT_CFG, SMALL_CFG):
        for cut in range(1, 60):
            assert_cut_changes_nothing(axc, (cut, 60 - cut), cfg)
    for fam in ("bursts", "p05", "p50"):
        axc = draw_family(fam, rng, 3, 400)
        for _ in range(4):
            at = np.sort(rng.choice(np.arange(1, 400), 5, replace=False))
            cuts = tuple(int(x) for x in np.diff(np.concatenate([[0], at, [400]])))
            assert_cut_changes_nothing(axc, cuts, SMALL_CFG if fam == "p50" else DEFAULT_CFG)


def test_energy_order_is_not_a_plain_sum():
    """the defined order against math.fsum: equal to rounding, and the halving tree is what it says (two hand-made blocks)"""
    import math
    rng = np.random.default_rng(6)
    blocks = draw_audio(rng, 3, WAVE_BATCH)
    got = block_energy(blocks)
    for g, b in zip(got, blocks):
        exact = math.fsum(float(x) * float(x) for x in b)
        assert abs(g - exact) <= 2000 * 2.0**-53 * exact
    one = np.zeros(WAVE_BATCH, np.float32)
    one[4 * 499 + 3] = 0.5  # float4 number 499 belongs to thread 243
    assert block_energy(one[None])[0] == 0.25


# ---------------- mi_tx_plan_host against the model ----------------

def warm_state(rng, rows, cfg):
    """a state in mid-run: what a 9-batch burst call leaves"""
    return tx_model(draw_bursts(rng, rows, 9), cfg=cfg)[2]


def assert_plan_equals_model(pkg, axc, state, wave, cfg, what, enabled=None, nbatches=None):
    rows = axc.shape[0]
    nb = axc.shape[1] if nbatches is None else nbatches
    en = np.ones(rows, np.uint8) if enabled is None else enabled
    rec, first, count, after = pkg.tx_plan_host(en, axc, state, wave, cfg, nbatches=nb)
    want_rec, want_first, want_after, _, _ = tx_model(axc[:, :nb], state, en, wave, cfg)
    assert tuple(count) == (len(want_rec), len(want_rec)), f"{what}: counts {count} vs {len(want_rec)}"
    assert np.array_equal(first, want_first), f"{what}: row_first_record"
    assert rec.tobytes() == want_rec.tobytes(), f"{what}: records\n{rec}\n{want_rec}"
    assert after.tobytes() == want_after.tobytes(), f"{what}: state blob"
    return rec, after


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows,nbatches", BURST_SHAPES)
def test_plan_host_equals_the_model(pkg, rows, nbatches, family):
    rng = np.random.default_rng([rows, nbatches, FAMILIES.index(family)])
    axc = draw_family(family, rng, rows, nbatches)
    wave = draw_audio(rng, rows, nbatches * WAVE_BATCH)
    for cfg in (SMALL_CFG, DEFAULT_CFG):
        for state in (fresh_state(rows), warm_state(rng, rows, cfg)):
            assert_plan_equals_model(pkg, axc, state, wave, cfg, f"{rows} x {nbatches}, {family}, cfg {cfg}")
    rec, _ = assert_plan_equals_model(pkg, axc, None, None, DEFAULT_CFG, "no audio")
    assert not rec["peak"].any() and not rec["energy"].any()


def test_plan_host_defaults_and_padded_strides(pkg):
    rng = np.random.default_rng(7)
    axc, wave = draw_bursts(rng, 3, 80), draw_audio(rng, 3, 80 * WAVE_BATCH)
    a = pkg.tx_plan_host(np.ones(3), axc, waveout=wave, cfg=None, nbatches=65)
    b = pkg.tx_plan_host(np.ones(3), axc, waveout=wave, cfg=(0, 0, 0), nbatches=65)
    c = pkg.tx_plan_host(np.ones(3), axc, waveout=wave, cfg=DEFAULT_CFG, nbatches=65)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    assert_plan_equals_model(pkg, axc, None, wave, DEFAULT_CFG, "65 of 80 batches", nbatches=65)


def test_disabled_rows_keep_every_byte_of_their_state(pkg):
    rng = np.random.default_rng(8)
    rows = 6
    axc = draw_bursts(rng, rows, 65)
    wave = draw_audio(rng, rows, 65 * WAVE_BATCH)
    state = warm_state(rng, rows, SMALL_CFG)
    en = np.array([1, 0, 1, 0, 0, 1], np.uint8)
    rec, after = assert_plan_equals_model(pkg, axc, state, wave, SMALL_CFG, "disabled rows", enabled=en)
    before, after = state.view(np.uint8).reshape(rows, 32), after.reshape(rows, 32)
    assert np.array_equal(before[en == 0], after[en == 0]) and not np.array_equal(before[0], after[0])
    assert set(rec["row"]) == {0, 2, 5}


def raw_plan(pkg, axc, wave, cfg, cap, room, state=None):
    """mi_tx_plan_host through ctypes with a record buffer of `room` entries, told `cap`, all bytes SENT beforehand"""
    rows, nb = axc.shape
    state = np.zeros(rows * 32, np.uint8) if state is None else state
    rec = np.full(room * 40, SENT, np.uint8)
    first, count = np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = pkg.lib().mi_tx_plan_host(C.byref(pkg.TxCfg(*cfg)), p(np.ones(rows, np.uint8)), rows, p(axc), nb, nb, p(wave), 0 if wave is None else wave.shape[1],
                                   p(state), p(rec), cap, p(first), p(count))
    return rc, rec, first, count, state


def test_capacity_short_of_the_total(pkg):
    rng = np.random.default_rng(9)
    axc, wave = draw_bursts(rng, 3, 65), draw_audio(rng, 3, 65 * WAVE_BATCH)
    want, want_first, want_state, _, _ = tx_model(axc, wave=wave, cfg=SMALL_CFG)
    cap = len(want) // 2
    assert cap >= 2
    rc, rec, first, count, state = raw_plan(pkg, axc, wave, SMALL_CFG, cap, cap + 3)
    assert rc == pkg.MI_OK and tuple(count) == (len(want), cap)
    assert rec[:cap * 40].tobytes() == want[:cap].tobytes() and (rec[cap * 40:] == SENT).all(), "records behind the capacity"
    assert np.array_equal(first, want_first) and state.tobytes() == want_state.tobytes()


def test_the_reference_s_own_thresholds_reach_the_hour_split(pkg):
    """1 x 60 000 batches, flags only: an unbroken signal is cut at 28 800 batches twice"""
    axc = np.full((1, 60000), ord("*"), np.uint8)
    axc[0, 59000:] = NO_SIGNAL
    rec, _ = assert_plan_equals_model(pkg, axc, None, None, DEFAULT_CFG, "1 x 60000")
    assert [int(x) for x in rec["close_batch"]] == [28801, 57602, 59000 + 5]
    assert [int(x) for x in rec["nblocks"]] == [28801, 28801, 59001 - 57602]


def test_argument_errors(pkg):
    axc = np.full((2, 3), ord("*"), np.uint8)
    assert raw_plan(pkg, axc, None, DEFAULT_CFG, 8, 8)[0] == pkg.MI_OK
    assert raw_plan(pkg, axc, None, DEFAULT_CFG, 0, 8)[0] == pkg.MI_ERR_INVALID
    bad = np.zeros(2 * 32, np.uint8)
    bad[28] = 2  # `open` is 0 or 1
    assert raw_plan(pkg, axc, None, DEFAULT_CFG, 8, 8, state=bad)[0] == pkg.MI_ERR_INVALID
    assert b"state" in pkg.lib().mi_last_error()
    short = np.zeros((2, 3 * WAVE_BATCH - 4), np.float32)
    assert raw_plan(pkg, axc, short, DEFAULT_CFG, 8, 8)[0] == pkg.MI_ERR_INVALID
    f = pkg.lib().mi_tx_plan_host
    assert f(None, None, 2, None, 3, 3, None, 0, None, None, 8, None, None) == pkg.MI_ERR_INVALID


def test_library_exports_the_splitter_s_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_txsplit_") or s.startswith("mi_tx_")}
    assert declared == TX_SYMBOLS
    lib = pkg.lib()
    assert not [s for s in sorted(declared) if not hasattr(lib, s)]
    assert declared <= set(pkg.ABI_SYMBOLS)
    assert C.sizeof(pkg.TxRecord) == 40 == pkg.TX_RECORD_DTYPE.itemsize == RECORD.itemsize and C.sizeof(pkg.TxCfg) == 12
    assert pkg.TX_STATE_DTYPE.itemsize == 32 == STATE.itemsize and pkg.TX_NONE == NONE
    assert [(n, pkg.TX_RECORD_DTYPE.fields[n][1]) for n in pkg.TX_RECORD_DTYPE.names] == [(n, RECORD.fields[n][1]) for n in RECORD.names]
    assert re.search(r"\bMI_TX_STATE_ROW_BYTES = 32\b", header)
