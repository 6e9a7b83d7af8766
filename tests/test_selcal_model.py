"""The SELCAL decoder stage without a GPU: the header's symbols, sizes and tables; the numpy model of selcal_model.py against a float64
DFT; the host twin mi_selcal_plan_host against the model as bytes -- windows, codes, prefix, counts and state --; what every seeded
builder must and must not decode; mi_selcal_code_text; and every refusal that needs no handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from selcal_model import (CODE_REC, DEFAULTS, DONE, FIRST, GAP, HISTORY, HZ_16, HZ_32, LETTERS_16, LETTERS_32, MODE_16, MODE_32, MODE_CUSTOM, NB, NONE8, OVER,
                          SECOND, STATE, WAVE_BATCH, WINDOW, WINDOW_REC, E2E_CODE, SHORT, code_row, e2e_setup, short_codes, code_text, coeffs, fresh_state, hann, run_in_calls, selcal_model, stacked, table,
                          tonality_constant, window_records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELCAL_SYMBOLS = {"mi_selcal_" + s for s in ("create", "destroy", "set_rows", "process_device", "download", "state_size", "get_state", "set_state", "set_timing",
                                              "last_launch_ms", "plan_host", "table", "settings", "window", "code_text")}
SENT = 0xA5
CUSTOM2 = [700.0, 1100.0]
_cache = {}


def builders(mode):
    if mode not in _cache:
        _cache[mode] = stacked(mode)
    return _cache[mode]


def model_calls(mode, cuts):
    """the model over a mode's stacked builders in calls of `cuts`, computed once"""
    key = (mode, tuple(cuts))
    if key not in _cache:
        _cache[key] = run_in_calls(builders(mode)[1], cuts, mode=mode)
    return _cache[key]


def raw_plan(pkg, cfg, en, plane, nb, state, cap, want_windows=True, guard=2):
    """mi_selcal_plan_host over sentinel-filled outputs `guard` entries longer than told: (rc, codes bytes, windows, row_first, count, state)"""
    rows = plane.shape[0]
    codes = np.full((cap + guard) * CODE_REC.itemsize, SENT, np.uint8)
    win = np.full(rows * 2 * nb * WINDOW_REC.itemsize + guard, SENT, np.uint8) if want_windows else None
    first = np.full(rows + 1 + guard, 0xA5A5A5A5, np.uint32)
    count = np.full(2 + guard, 0xA5A5A5A5, np.uint32)
    state = state.copy()
    en = np.asarray(en, np.uint8)
    rc = pkg.lib().mi_selcal_plan_host(C.byref(cfg) if cfg is not None else None, en.ctypes.data, rows, nb, plane.ctypes.data, plane.shape[1], state.ctypes.data,
                                       None if win is None else win.ctypes.data, codes.ctypes.data, cap, first.ctypes.data, count.ctypes.data)
    return rc, codes, win, first, count, state


def check_twin_call(pkg, what, cfg, en, plane, nb, state, want, cap=0, want_windows=True, pad=0):
    """one call of the twin against the model's (codes, windows, row_first, state after): every byte, and the sentinels behind them"""
    rows = plane.shape[0]
    w_codes, w_win, w_first, w_state = want
    room = cap or max(1, rows * pkg.selcal_max_codes(nb, cfg))
    lay = np.full((rows, (nb + pad) * WAVE_BATCH), np.float32(0.25))  # what lies behind the call must not be read
    lay[:, :nb * WAVE_BATCH] = plane
    rc, codes, win, first, count, after = raw_plan(pkg, cfg, en, lay, nb, state, room, want_windows)
    assert rc == pkg.MI_OK, pkg.lib().mi_last_error()
    total, k = len(w_codes), min(len(w_codes), room)
    assert (int(count[0]), int(count[1])) == (total, k) and (count[2:] == 0xA5A5A5A5).all(), f"{what}: counts {count[:2]}, the model has {total}"
    assert np.array_equal(first[:rows + 1], w_first) and (first[rows + 1:] == 0xA5A5A5A5).all(), f"{what}: row_first_code"
    assert codes[:k * CODE_REC.itemsize].tobytes() == w_codes[:k].tobytes(), f"{what}: codes\n{codes[:k * 32].view(CODE_REC)}\nwant\n{w_codes[:k]}"
    assert (codes[k * CODE_REC.itemsize:] == SENT).all(), f"{what}: something was written behind code {k}"
    if want_windows:
        got = win[:rows * 2 * nb * WINDOW_REC.itemsize].view(WINDOW_REC).reshape(rows, 2 * nb)
        on = np.asarray(en, bool)
        assert got[on].tobytes() == w_win[on].tobytes(), f"{what}: window records"
        assert (got[~on].view(np.uint8) == SENT).all() and (win[rows * 2 * nb * WINDOW_REC.itemsize:] == SENT).all(), f"{what}: a disabled row's windows were written"
    assert after.tobytes() == w_state.tobytes(), f"{what}: state blob after"
    return after


# ---------------- symbols, sizes, tables ----------------

def test_library_exports_the_selcal_stage_s_symbols_and_sizes(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    assert re.search(r"MI_SELCAL_WINDOW = 2000, MI_SELCAL_HOP = 1000, MI_SELCAL_HISTORY = 1002, MI_SELCAL_MAX_TONES = 32, MI_SELCAL_STATE_ROW_BYTES = 4048", header)
    assert "written from memory" in header and "synthetic signals only" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", code) if s.startswith("mi_selcal_")}
    assert declared == SELCAL_SYMBOLS and SELCAL_SYMBOLS <= set(pkg.ABI_SYMBOLS)
    assert not [s for s in sorted(declared) if not hasattr(pkg.lib(), s)]
    assert C.sizeof(pkg.SelcalCfg) == 168 and pkg.SELCAL_WINDOW_DTYPE.itemsize == 24 == WINDOW_REC.itemsize
    assert pkg.SELCAL_CODE_DTYPE.itemsize == 32 == CODE_REC.itemsize and pkg.SELCAL_STATE_DTYPE.itemsize == 4048 == STATE.itemsize
    for a, b in ((pkg.SELCAL_WINDOW_DTYPE, WINDOW_REC), (pkg.SELCAL_CODE_DTYPE, CODE_REC), (pkg.SELCAL_STATE_DTYPE, STATE)):
        assert [(n, a.fields[n][1]) for n in a.names] == [(n, b.fields[n][1]) for n in b.names]
    assert (pkg.SELCAL_WINDOW, pkg.SELCAL_HISTORY, pkg.SELCAL_NONE8) == (WINDOW, HISTORY, NONE8)
    assert (pkg.SELCAL_FIRST, pkg.SELCAL_OVER, pkg.SELCAL_GAP, pkg.SELCAL_SECOND, pkg.SELCAL_DONE) == (FIRST, OVER, GAP, SECOND, DONE)


def test_tone_tables_against_the_formula_and_the_header(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    f32, c32, l32 = pkg.selcal_table(pkg.selcal_cfg(MODE_32))
    f16, c16, l16 = pkg.selcal_table()
    assert l32 == LETTERS_32 and l16 == LETTERS_16 == "ABCDEFGHJKLMPQRS" and len(f32) == 32 and len(f16) == 16
    assert f32.tobytes() == np.array(HZ_32, np.float32).tobytes() and f16.tobytes() == np.array(HZ_16, np.float32).tobytes() == f32[::2].tobytes()
    for k, (f, letter) in enumerate(zip(HZ_32, LETTERS_32)):
        assert abs(f - 312.6 * 10 ** (0.0225 * k)) <= 0.15, (k, f)
        assert re.search(rf"\b{letter} {f}\b", header), f"the header does not give {letter} {f}"
    assert np.all(np.diff(f32) > 16.0)
    assert c32.tobytes() == coeffs(HZ_32).tobytes() and c16.tobytes() == coeffs(HZ_16).tobytes()
    f, c, letters = pkg.selcal_table(pkg.selcal_cfg(MODE_CUSTOM, freq=CUSTOM2))
    assert list(f) == CUSTOM2 and letters == "??" and c.tobytes() == coeffs(CUSTOM2).tobytes()
    filled, cc = pkg.selcal_settings()
    assert {k: getattr(filled, k) for k in DEFAULTS} == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in DEFAULTS.items()}
    assert filled.ntones == 16 and cc == tonality_constant(hann()) and abs(float(cc) - 2000 / 3) < 1.0


def test_window_from_its_formula(pkg):
    w = pkg.selcal_window()
    exact = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WINDOW) / (WINDOW - 1))
    assert np.all(np.abs(w.astype(np.float64) - exact) <= np.spacing(np.maximum(w, np.float32(1e-30))))
    assert w.tobytes() == w[::-1].tobytes() and w.tobytes() == hann().tobytes() and w[0] == 0.0 and w.max() <= 1.0


# The largest |p - p64| over the tones of a window, relative to the window's largest p, measured on the CPU over every window of both
# modes' builders that is not silent: 8.5e-5 with 16 tones, 1.53e-4 with 32 (float32 recurrence of 2000 steps against a float64 DFT of the same float32 y).  The bound
# is four times that.
DFT_ERROR_MEASURED = 1.53e-4


@pytest.mark.parametrize("mode", [MODE_16, MODE_32])
def test_model_powers_against_a_float64_dft(mode):
    plane = builders(mode)[1]
    frames = np.lib.stride_tricks.sliding_window_view(plane, WINDOW, axis=1)[:, ::1000].reshape(-1, WINDOW)
    hz = table(mode)[0]
    rec, p = window_records(frames, coeffs(hz), dict(DEFAULTS))
    live = rec["energy"] != 0
    y = (frames.astype(np.float32) * hann()).astype(np.float64)[live]
    omega = 2.0 * np.pi * hz.astype(np.float64) / 16000
    # the recurrence ends one step short of the DFT's phase reference, which the magnitude does not see
    p64 = np.abs(y @ np.exp(-1j * np.outer(np.arange(WINDOW), omega))) ** 2
    err = np.max(np.abs(p[live] - p64), axis=1) / np.max(p64, axis=1)
    print(f"mode {mode}: {live.sum()} windows, worst relative error {err.max():.3g}")
    assert err.max() <= 4 * DFT_ERROR_MEASURED


# ---------------- the twin against the model ----------------

@pytest.mark.parametrize("mode,cuts", [(MODE_16, (24,)), (MODE_16, (11, 13)), (MODE_16, (1,) * 24), (MODE_32, (24,)), (MODE_32, (11, 13))])
def test_twin_equals_model_on_every_builder(pkg, mode, cuts):
    names, plane, _ = builders(mode)
    cfg = pkg.selcal_cfg(mode)
    state, done = fresh_state(len(names)), 0
    for i, (n, want) in enumerate(zip(cuts, model_calls(mode, cuts))):
        state = check_twin_call(pkg, f"mode {mode}, call {i} at batch {done}", cfg, np.ones(len(names)), plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], n,
                                state, want, pad=i % 2)
        done += n
    whole = model_calls(mode, (24,))[0]
    total = sum(len(c[0]) for c in model_calls(mode, cuts))
    assert total == len(whole[0]) and state.tobytes() == whole[3].tobytes(), "the cuts change what is decoded"


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("nb", [1, 4])
def test_twin_equals_model_at_small_shapes(pkg, rows, nb):
    plane = builders(MODE_16)[1][8:8 + rows, 2 * WAVE_BATCH:(2 + 2 * nb) * WAVE_BATCH]  # (from inside the first pulse on)
    state = fresh_state(rows)
    for i in range(2):
        part = plane[:, i * nb * WAVE_BATCH:(i + 1) * nb * WAVE_BATCH]
        want = selcal_model(part, state)
        state = check_twin_call(pkg, f"{rows} rows, {nb} batches, call {i}", None, np.ones(rows), part, nb, state, want)
    assert state["phase"].any() and state["window"][0] == 4 * nb


def test_twin_disabled_row_capped_codes_null_windows_and_short_min_run(pkg):
    names, plane, _ = builders(MODE_16)
    rows = len(names)
    en = np.ones(rows, np.uint8)
    en[[0, 9]] = 0
    st = fresh_state(rows)
    st["x"][:] = np.random.default_rng(5).normal(0, 0.1, (rows, HISTORY)).astype(np.float32)
    st["window"], st["seq"] = 0xFFFFFFF0, 7  # (the window number wraps inside the call)
    want = selcal_model(plane, st, en)
    after = check_twin_call(pkg, "rows 0 and 9 disabled", None, en, plane, NB, st, want)
    assert after[0].tobytes() == st[0].tobytes() and after[9].tobytes() == st[9].tobytes() and want[0]["last_window"].min() < 48
    assert len(want[0]) >= 8
    for cap in (1, 3):
        check_twin_call(pkg, f"cap {cap}", None, en, plane, NB, st, want, cap=cap)
    check_twin_call(pkg, "no windows", None, en, plane, NB, st, want, want_windows=False)
    want = selcal_model(short_codes(), **SHORT)  # several codes a row, overlong pulses, gaps over max_gap
    assert len(want[0]) >= 6 and np.diff(want[2]).max() == 3 and np.diff(want[2]).min() <= 1
    check_twin_call(pkg, "min_run 2", pkg.selcal_cfg(MODE_16, **SHORT), np.ones(6), short_codes(), 18, fresh_state(6), want)
    check_twin_call(pkg, "min_run 2, cap 4", pkg.selcal_cfg(MODE_16, **SHORT), np.ones(6), short_codes(), 18, fresh_state(6), want, cap=4)
    f, kw = CUSTOM2, dict(mode=MODE_CUSTOM, freq=CUSTOM2)
    two = np.stack([code_row((0, 1), None, np.array(f), seed=3), np.zeros(NB * WAVE_BATCH)]).astype(np.float32)
    want = selcal_model(two, **kw)
    assert (want[1]["third"] == NONE8).all() and (want[1][0]["pair"] == 0x100).sum() >= 14
    check_twin_call(pkg, "a table of two tones", pkg.selcal_cfg(MODE_CUSTOM, freq=f), np.ones(2), two, NB, fresh_state(2), want)


# ---------------- what decodes and what does not ----------------

@pytest.mark.parametrize("mode", [MODE_16, MODE_32])
def test_every_builder_decodes_what_it_should(pkg, mode):
    names, plane, texts = builders(mode)
    codes, windows, first, _ = model_calls(mode, (24,))[0]
    assert sum(1 for t in texts if t) >= 15 and sum(1 for t in texts if not t) >= 11
    for r, (name, want) in enumerate(zip(names, texts)):
        mine = codes[first[r]:first[r + 1]]
        got = [code_text(c["tone"], mode) for c in mine]
        assert got == want and [pkg.selcal_code_text(c["tone"], mode) for c in mine] == want, f"{name}: decoded {got}, sent {want}"
        if not want:
            continue
        c, pairs = mine[0], windows[r]["pair"]
        p1, p2 = int(c["tone"][0]) | int(c["tone"][1]) << 8, int(c["tone"][2]) | int(c["tone"][3]) << 8
        second = np.flatnonzero(pairs == p2)
        # the emitting window is the min_run-th of the second pulse, which begins where the first window names its pair
        assert c["last_window"] == second[0] + DEFAULTS["min_run"] - 1 and c["batch"] == c["last_window"] // 2, name
        assert pairs[c["first_window"]] == p1 and not (pairs[:c["first_window"]] == p1).any() and c["run1"] >= DEFAULTS["min_run"], name
        assert c["gap"] == second[0] - c["first_window"] - c["run1"], name
    # where the pulses lie: a window all inside the second pulse names it, so the pulse is seen at most one window before the first such
    for r, name in enumerate(names):
        if name.startswith("offset"):
            start2 = WAVE_BATCH + int(name.split()[1]) + 16000 + 3200
            full = -(-start2 // 1000) + 1  # window n covers samples 1000 (n - 1) .. 1000 (n + 1)
            assert full - 1 <= np.flatnonzero(windows[r]["pair"] == 0x703 if mode == MODE_16 else windows[r]["pair"] == 0x703)[0] <= full, name
    drop = names.index("a dropout inside the first pulse")
    c = codes[first[drop]]
    assert c["run1"] >= 16 and (windows[drop]["pair"][c["first_window"]:c["first_window"] + c["run1"]] == 0).sum() >= 1, "the dropout was not inside the run"


def test_the_clean_signal_alone_stays_inside_the_conditions():
    """before noise, twist or a dropout are added: a clean code's windows inside a pulse have tonality near 1, twist near 1 and a
    separation far over the threshold, so the positives test the decoder and not a signal that is marginal by itself"""
    x = code_row((2, 11), (5, 13), np.array(HZ_16), seed=52).astype(np.float32)[None, :]
    _, win, _, _ = selcal_model(x)
    inside = win[0][5:15]
    c = tonality_constant(hann())
    assert ((inside["p_best"] + inside["p_second"]) / (c * inside["energy"]) > 0.95).all()
    assert (inside["p_best"] / inside["p_second"] < 1.2).all() and (inside["p_second"] / inside["p_third"] > 1000).all()


def test_code_text(pkg):
    assert pkg.selcal_code_text([0, 1, 2, 3]) == "AB-CD" and pkg.selcal_code_text([15, 14, 8, 11]) == "SR-JM"
    assert pkg.selcal_code_text([0, 1, 30, 31], MODE_32) == "AT-S9" and pkg.selcal_code_text([0, 31, 2, 3], MODE_CUSTOM) == "??-??"
    for tones, mode in (([0, 1, 2, 16], MODE_16), ([0, 1, 2, 32], MODE_32), ([0, 1, 2, 32], MODE_CUSTOM), ([0, 1, 2, 3], 3)):
        with pytest.raises(pkg.MiError) as e:
            pkg.selcal_code_text(tones, mode)
        assert e.value.code == pkg.MI_ERR_INVALID


def test_end_to_end_call_through_the_oracle_the_twin_and_the_voice_band(pkg):
    """an AM carrier with a call on it as u8 I/Q through the CPU oracle, then mi_selcal_plan_host over its audio: the code that was
    sent, once; and the same through the voice band stage's twin at (300, 3400)"""
    from common import oracle_run
    dev, chans, iq, nb = e2e_setup(pkg)
    n, wo, axc, _ = oracle_run(dev, chans, iq, nb)
    assert n == nb and (axc[0][7:] == ord("*")).all(), "the squelch is not open when the call begins"
    codes = pkg.selcal_plan_host([1], wo[:1])[0]
    assert [pkg.selcal_code_text(c["tone"]) for c in codes] == [E2E_CODE]
    filtered = pkg.vband_plan_host([1], np.ascontiguousarray(wo[:1]), rows_cfg=[(300, 3400)])[0]
    assert [pkg.selcal_code_text(c["tone"]) for c in pkg.selcal_plan_host([1], filtered)[0]] == [E2E_CODE]


# ---------------- refusals ----------------

BOUNDS = [("min_energy", 1e-12, 1e6, 0.9e-12, 1.1e6), ("min_tonality", 0.01, 1.0, 0.009, 1.01), ("max_twist", 1.0, 1000.0, 0.99, 1001.0),
          ("min_separation", 1.0, 1000.0, 0.99, 1001.0), ("min_run", 2, 64, 1, 65), ("max_gap", 1, 64, None, 65)]


def test_settings_bounds_on_both_sides(pkg):
    for name, lo, hi, below, above in BOUNDS:
        extra = dict(max_run=1024) if name == "min_run" else {}
        for ok in (lo, hi):
            assert getattr(pkg.selcal_settings(pkg.selcal_cfg(**{name: ok, **extra}))[0], name) == (np.float32(ok) if isinstance(ok, float) else ok)
        for bad in (below, above):
            if bad is None:
                continue
            with pytest.raises(pkg.MiError) as e:
                pkg.selcal_settings(pkg.selcal_cfg(**{name: bad, **extra}))
            assert e.value.code == pkg.MI_ERR_INVALID and name in str(e.value), (name, bad)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(pkg.MiError):
            pkg.selcal_settings(pkg.selcal_cfg(min_energy=bad))
    assert pkg.selcal_settings(pkg.selcal_cfg(min_run=8, max_run=8))[0].max_run == 8 and pkg.selcal_settings(pkg.selcal_cfg(max_run=1024))[0].max_run == 1024
    assert pkg.selcal_settings(pkg.selcal_cfg(min_run=30))[0].max_run == 30, "the default max_run is not below min_run"
    for kw in (dict(min_run=9, max_run=8), dict(max_run=1025)):
        with pytest.raises(pkg.MiError) as e:
            pkg.selcal_settings(pkg.selcal_cfg(**kw))
        assert "max_run" in str(e.value)
    c = pkg.selcal_cfg()
    c.zero = 1
    with pytest.raises(pkg.MiError):
        pkg.selcal_settings(c)


def test_custom_table_bounds_and_mode(pkg):
    ok = [[250.0, 266.0], [1984.0, 2000.0], list(250.0 + 16.0 * np.arange(32))]
    for f in ok:
        assert len(pkg.selcal_table(pkg.selcal_cfg(MODE_CUSTOM, freq=f))[0]) == len(f)
    bad = [[700.0], list(250.0 + 16.0 * np.arange(33)), [249.9, 400.0], [1990.0, 2000.1], [700.0, 715.9], [800.0, 700.0], [700.0, 700.0],
           [700.0, float("nan")], [float("nan"), 700.0]]
    for f in bad:
        with pytest.raises(pkg.MiError) as e:
            pkg.selcal_table(pkg.selcal_cfg(MODE_CUSTOM, freq=f))
        assert e.value.code == pkg.MI_ERR_INVALID and ("custom" in str(e.value)), f
    with pytest.raises(pkg.MiError) as e:
        pkg.selcal_table(pkg.selcal_cfg(3))
    assert "mode" in str(e.value)


def test_plan_host_and_create_refusals(pkg):
    plane = np.zeros((2, 2 * WAVE_BATCH), np.float32)
    st = fresh_state(2)
    assert raw_plan(pkg, None, [1, 1], plane, 2, st, 4)[0] == pkg.MI_OK
    for kw in (dict(nb=0), dict(nb=3), dict(cap=0)):
        assert raw_plan(pkg, None, [1, 1], plane, kw.get("nb", 2), st, kw.get("cap", 4))[0] == pkg.MI_ERR_INVALID, kw
    L = pkg.lib()
    assert L.mi_selcal_plan_host(None, None, 2, 2, plane.ctypes.data, 4000, st.ctypes.data, None, None, 4, None, None) == pkg.MI_ERR_INVALID
    assert b"NULL" in L.mi_last_error()
    assert raw_plan(pkg, pkg.selcal_cfg(min_run=1), [1, 1], plane, 2, st, 4)[0] == pkg.MI_ERR_INVALID and b"min_run" in L.mi_last_error()

    def bad_state(**fields):
        s = fresh_state(2)
        for k, v in fields.items():
            s[k][1] = v
        return raw_plan(pkg, None, [1, 1], plane, 2, s, 4)[0]

    good = [dict(phase=FIRST, pair1=0x100, run1=22), dict(phase=OVER, pair1=0xF0E, run1=23), dict(phase=GAP, pair1=0x100, run1=8, gap=8),
            dict(phase=SECOND, pair1=0x100, pair2=0x200, run1=8, run2=7, gap=0), dict(phase=DONE, pair1=0x100, pair2=0x302, run1=22, run2=8, gap=8)]
    for g in good:
        assert bad_state(**g) == pkg.MI_OK, g
    bad = [dict(phase=6), dict(zero=1), dict(pair1=0x100), dict(run1=1), dict(phase=FIRST, pair1=0x100, run1=23), dict(phase=FIRST, pair1=0x100, run1=0),
           dict(phase=FIRST, pair1=0x101, run1=1), dict(phase=FIRST, pair1=0x1000, run1=1), dict(phase=FIRST, pair1=0x001, run1=1),
           dict(phase=FIRST, pair1=0x10100, run1=1), dict(phase=FIRST, pair1=0x100, run1=1, pair2=0x200), dict(phase=OVER, pair1=0x100, run1=22),
           dict(phase=GAP, pair1=0x100, run1=7, gap=1), dict(phase=GAP, pair1=0x100, run1=8, gap=9), dict(phase=GAP, pair1=0x100, run1=8, gap=0),
           dict(phase=SECOND, pair1=0x100, pair2=0x100, run1=8, run2=1), dict(phase=SECOND, pair1=0x100, pair2=0x200, run1=8, run2=8),
           dict(phase=SECOND, pair1=0x100, pair2=0x200, run1=8, run2=0), dict(phase=DONE, pair1=0x100, pair2=0x200, run1=8, run2=7)]
    for b in bad:
        assert bad_state(**b) == pkg.MI_ERR_INVALID and b"state" in L.mi_last_error(), b
    if pkg.device_count() == 0:  # create is refused before anything else where no device is
        with pytest.raises(pkg.MiError) as e:
            pkg.Selcal([1, 1], max_batches=4)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE
    for kw in (dict(max_batches=0), dict(cfg=pkg.selcal_cfg(max_gap=65)), dict(max_batches=1 << 24), dict(cfg=pkg.selcal_cfg(MODE_CUSTOM, freq=[700.0]))):
        with pytest.raises(pkg.MiError) as e:  # the argument checks come before the device is looked for
            pkg.Selcal(np.ones(8), **{"max_batches": 4, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID, kw
