"""The ELT detector stage without a GPU: the numpy model of elt_model.py against a float64 FFT; the host twin mi_elt_plan_host against
the model as bytes -- frame records, events, prefix, counts and state --; what every seeded builder and walker sequence must and must
not raise; the capacity bound reached; mi_elt_event_text; and long runs of noise and voice through the twin."""
import ctypes as C

import numpy as np
import pytest

from elt_model import (BOUND_NB, BINS, BIN0, DEFAULTS, DOWN, END, EVENT_REC, FRAME, FRAME_REC, FRAMES, HISTORY, HOP, NB, NONE8, OFFSET_NB, ONSET, STATE, UP, WAVE_BATCH,
                       beacon, carried_edge_state, coeffs, elt_model, event_text, fresh_state, frame_records, hann, max_events, run_in_calls, settings, stacked,
                       start_offsets, tonality_constant, voice_like, walk, walker_sequences, Walker, bound_cases, bound_signals)

SENT = 0xA5
_cache = {}


def model_calls(cuts):
    """the model over the stacked builders in calls of `cuts`, computed once"""
    if cuts not in _cache:
        _cache[cuts] = run_in_calls(stacked()[1], cuts)
    return _cache[cuts]


def raw_plan(pkg, cfg, en, plane, nb, state, cap, want_frames=True, guard=2):
    """mi_elt_plan_host over sentinel-filled outputs `guard` entries longer than told: (rc, events bytes, frames, row_first, count, state)"""
    rows = plane.shape[0]
    events = np.full((cap + guard) * EVENT_REC.itemsize, SENT, np.uint8)
    fr = np.full(rows * FRAMES * nb * FRAME_REC.itemsize + guard, SENT, np.uint8) if want_frames else None
    first = np.full(rows + 1 + guard, 0xA5A5A5A5, np.uint32)
    count = np.full(2 + guard, 0xA5A5A5A5, np.uint32)
    state = state.copy()
    en = np.asarray(en, np.uint8)
    rc = pkg.lib().mi_elt_plan_host(C.byref(cfg) if cfg is not None else None, en.ctypes.data, rows, nb, plane.ctypes.data, plane.shape[1], state.ctypes.data,
                                    None if fr is None else fr.ctypes.data, events.ctypes.data, cap, first.ctypes.data, count.ctypes.data)
    return rc, events, fr, first, count, state


def check_twin_call(pkg, what, cfg, en, plane, nb, state, want, cap=0, want_frames=True, pad=0):
    """one call of the twin against the model's (events, frames, row_first, state after): every byte, and the sentinels behind them"""
    rows = plane.shape[0]
    w_events, w_fr, w_first, w_state = want
    room = cap or max(1, rows * pkg.elt_max_events(nb, cfg))
    lay = np.full((rows, (nb + pad) * WAVE_BATCH), np.float32(0.25))  # what lies behind the call must not be read
    lay[:, :nb * WAVE_BATCH] = plane
    rc, events, fr, first, count, after = raw_plan(pkg, cfg, en, lay, nb, state, room, want_frames)
    assert rc == pkg.MI_OK, pkg.lib().mi_last_error()
    total, k = len(w_events), min(len(w_events), room)
    assert (int(count[0]), int(count[1])) == (total, k) and (count[2:] == 0xA5A5A5A5).all(), f"{what}: counts {count[:2]}, the model has {total}"
    assert np.array_equal(first[:rows + 1], w_first) and (first[rows + 1:] == 0xA5A5A5A5).all(), f"{what}: row_first_event"
    assert events[:k * 32].tobytes() == w_events[:k].tobytes(), f"{what}: events\n{events[:k * 32].view(EVENT_REC)}\nwant\n{w_events[:k]}"
    assert (events[k * 32:] == SENT).all(), f"{what}: something was written behind event {k}"
    if want_frames:
        got = fr[:rows * FRAMES * nb * 16].view(FRAME_REC).reshape(rows, FRAMES * nb)
        on = np.asarray(en, bool)
        assert got[on].tobytes() == w_fr[on].tobytes(), f"{what}: frame records"
        assert (got[~on].view(np.uint8) == SENT).all() and (fr[rows * FRAMES * nb * 16:] == SENT).all(), f"{what}: a disabled row's frames were written"
    assert after.tobytes() == w_state.tobytes(), f"{what}: state blob after"
    return after


# ---------------- window, coefficients, the model against an FFT ----------------

def test_window_and_coefficients_from_their_formulas(pkg):
    w = pkg.elt_window()
    exact = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME) / (FRAME - 1))
    assert np.all(np.abs(w.astype(np.float64) - exact) <= np.spacing(np.maximum(w, np.float32(1e-30))))
    assert w.tobytes() == w[::-1].tobytes() and w.tobytes() == hann().tobytes() and w[0] == 0.0 and w.max() <= 1.0
    c = pkg.elt_coeffs()
    exact = 2.0 * np.cos(2.0 * np.pi * np.arange(BIN0, BIN0 + BINS) / FRAME)
    assert np.all(np.abs(c.astype(np.float64) - exact) <= np.spacing(np.abs(c))) and c.tobytes() == coeffs().tobytes()
    filled, cc = pkg.elt_settings()
    assert {k: getattr(filled, k) for k in DEFAULTS} == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in DEFAULTS.items()}
    assert cc == tonality_constant(hann()) and abs(float(cc) - 85.0) < 0.5


# The largest |p - p64| on the largest bin of a frame, relative to that bin's p64, measured on the CPU over every frame of the builders
# that is not silent: 6.26e-5 (float32 recurrence of 256 steps against a float64 FFT of the same float32 y).  The bound is four times that.
FFT_ERROR_MEASURED = 6.26e-5


def test_model_powers_against_a_float64_fft():
    plane = stacked()[1]
    frames = np.lib.stride_tricks.sliding_window_view(plane, FRAME, axis=1)[:, ::HOP].reshape(-1, FRAME)
    rec, p = frame_records(frames, dict(DEFAULTS))
    live = rec["energy"] != 0
    y = (frames.astype(np.float32) * hann()).astype(np.float64)[live]
    p64 = np.abs(np.fft.rfft(y, axis=1)[:, BIN0:BIN0 + BINS]) ** 2
    top = np.argmax(p64, axis=1)
    rows = np.arange(len(top))
    err = np.abs(p[live][rows, top] - p64[rows, top]) / p64[rows, top]
    print(f"{live.sum()} frames, worst relative error on the largest bin {err.max():.3g}")
    assert err.max() <= 4 * FFT_ERROR_MEASURED


# ---------------- the twin against the model ----------------

@pytest.mark.parametrize("cuts", [(48,), (5, 43), (1,) * 48])
def test_twin_equals_model_on_every_builder(pkg, cuts):
    names, plane, _ = stacked()
    state, done = fresh_state(len(names)), 0
    for i, (n, want) in enumerate(zip(cuts, model_calls(cuts))):
        state = check_twin_call(pkg, f"call {i} at batch {done}", None, np.ones(len(names)), plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], n, state, want,
                                pad=i % 2)
        done += n
    whole = model_calls((48,))[0]
    events = np.concatenate([c[0] for c in model_calls(cuts)])
    key = lambda es: [(int(e["row"]), int(e["seq"]), int(e["kind"]), int(e["frame"]), int(e["sweeps"])) for e in es]  # noqa: E731
    assert sorted(key(events)) == sorted(key(whole[0])) and state.tobytes() == whole[3].tobytes(), "the cuts change what is detected"


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("cuts", [(48,), (5, 43), (1,) * 48])
def test_twin_equals_model_at_small_shapes(pkg, rows, cuts):
    plane = stacked()[1][10:10 + rows]  # (six sweeps then silence, restart, flip, punched ...)
    state, done = fresh_state(rows), 0
    for i, n in enumerate(cuts):
        part = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = elt_model(part, state)
        state = check_twin_call(pkg, f"{rows} rows, cuts {cuts[:2]}, call {i}", None, np.ones(rows), part, n, state, want)
        done += n
    assert state["frame"][0] == FRAMES * NB and state["seq"][0] == 2


def test_twin_on_the_80_start_offsets(pkg):
    plane = start_offsets()
    want = elt_model(plane)
    check_twin_call(pkg, "start offsets", None, np.ones(HOP), plane, OFFSET_NB, fresh_state(HOP), want)
    assert list(np.diff(want[2])) == [1] * HOP and (want[0]["kind"] == ONSET).all() and (want[0]["dir"] == DOWN).all()
    assert len(set(want[0]["frame"])) >= 2, "every offset falls on the same frame: the rows do not try the hop"


def test_twin_carried_edges_disabled_row_padded_strides_capped_outputs(pkg):
    names, plane, _ = stacked()
    rows = len(names)
    en = np.ones(rows, np.uint8)
    en[[0, 10]] = 0
    st = fresh_state(rows)
    st["x"][:] = np.random.default_rng(5).normal(0, 0.1, (rows, HISTORY)).astype(np.float32)
    st["frame"], st["seq"] = 0xFFFFFF00, 7  # (the frame number wraps inside the call, inside sweeps and chains)
    want = elt_model(plane, st, en)
    after = check_twin_call(pkg, "rows 0 and 10 disabled", None, en, plane, NB, st, want, pad=3)
    assert after[0].tobytes() == st[0].tobytes() and after[10].tobytes() == st[10].tobytes() and len(want[0]) >= 10
    assert want[0]["frame"].min() < 1200 and want[0]["first_frame"].max() > 0xFFFFFF00
    for cap in (1, 3):
        check_twin_call(pkg, f"cap {cap}", None, en, plane, NB, st, want, cap=cap)
    check_twin_call(pkg, "no frames", None, en, plane, NB, st, want, want_frames=False)
    # one carried sample, the newest and the oldest that weighs (x[2] is read too, and meets w[0] = 0), in front of silence: frames
    # 0 .. 2 (resp. frame 0) see it
    edge = carried_edge_state()
    zero = np.zeros((2, WAVE_BATCH), np.float32)
    want = elt_model(zero, edge)
    assert list(np.flatnonzero(want[1]["energy"][0])) == [0, 1, 2] and list(np.flatnonzero(want[1]["energy"][1])) == [0]
    check_twin_call(pkg, "carried edges", None, np.ones(2), zero, 1, edge, want)
    edge["x"][1, 3], edge["x"][1, :3] = 0.0, 0.5  # the two oldest are never read, the third meets w[0] = 0
    want = elt_model(zero, edge)
    assert not want[1]["energy"][1].any()
    check_twin_call(pkg, "carried samples that must not count", None, np.ones(2), zero, 1, edge, want)


CAP = dict(min_sweeps=2, min_len=25, max_len=60, max_gap=3, max_drop=1)


def capacity_rows():
    """a 7 Hz beacon that flips from downward to upward and stops two sweeps later, laid so that one call of two batches holds the END of
    the downward alarm, the ONSET of the upward one and its END: float32 [1][12 * 2000], and the calls' lengths"""
    n, per = 12 * WAVE_BATCH, RATE_7
    flip = 480 + int(4 * per)
    return (beacon(n, 7.0, start=480, stop=flip) + beacon(n, 7.0, down=False, start=flip, stop=flip + int(2 * per) + 40))[None, :].astype(np.float32), (6, 2, 4)


RATE_7 = 16000 / 7.0


def test_the_capacity_bound_is_reached(pkg):
    """With min_sweeps * min_len = 50 frames a call of 50 frames can hold one ONSET and, with an alarm carried in, two ENDs: three events,
    which is elt_max_events(2).  The row emits exactly those in its second call."""
    plane, cuts = capacity_rows()
    s = settings(**CAP)
    cfg = pkg.elt_cfg(**CAP)
    assert max_events(2, s) == 3 == pkg.elt_max_events(2, cfg) and [pkg.elt_max_events(n) for n in (1, 10, 48, 96)] == [3, 5, 11, 21]
    calls = run_in_calls(plane, cuts, **CAP)
    assert list(calls[1][0]["kind"]) == [END, ONSET, END] and list(calls[1][0]["dir"]) == [DOWN, UP, UP], calls[1][0]
    assert calls[0][3]["alarmed"][0] == 1 and calls[1][3]["alarmed"][0] == 0
    state, done = fresh_state(1), 0
    for i, (n, want) in enumerate(zip(cuts, calls)):
        state = check_twin_call(pkg, f"capacity, call {i}", cfg, [1], plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], n, state, want)
        done += n


# ---------------- what raises an alarm and what does not ----------------

def test_every_builder_raises_what_it_should(pkg):
    names, _, kinds = stacked()
    events, frames, first, _ = model_calls((48,))[0]
    assert sum(1 for k in kinds if k) >= 11 and sum(1 for k in kinds if not k) >= 15
    for r, (name, want) in enumerate(zip(names, kinds)):
        mine = events[first[r]:first[r + 1]]
        assert list(mine["kind"]) == want, f"{name}: events {[event_text(e) for e in mine]}"
        for e in mine:
            assert pkg.elt_event_text(e) == event_text(e), name
            assert e["sweeps"] >= 6 and e["dir"] == (UP if "upward" in name or (name.endswith("flips") and e["seq"] == 2) else DOWN), (name, e)
    at_noise = names.index("a beacon at the noise's power")
    assert (frames[at_noise]["bin"] != NONE8).mean() >= 0.95
    first_onset = events[first[1]]  # 3 Hz: six sweeps of 66.7 frames, the alarm at the seventh's first frame
    assert 395 <= first_onset["frame"] <= 405 and first_onset["batch"] == first_onset["frame"] // FRAMES and first_onset["first_frame"] == 0


@pytest.mark.parametrize("name,decisions,kw,want", walker_sequences(), ids=[s[0] for s in walker_sequences()])
def test_walker_sequences(name, decisions, kw, want):
    s = settings(**kw)
    st = fresh_state(1)
    events = walk(decisions, st[0], s)
    kinds = [e[2] for e in events]
    assert kinds == want, events
    assert all(a != b for a, b in zip(kinds, kinds[1:])), "a row's records alternate"
    assert st["count"][0] == 0 and st["alarmed"][0] == 0 and st["open"][0] == 0 and st["frame"][0] == len(decisions)
    st2 = fresh_state(1)  # the same from a frame counter about to wrap: every difference is modulo 2^32
    st2["frame"] = 0xFFFFFFFF - len(decisions) // 2
    again = walk(decisions, st2[0], s)
    assert [(e[2], e[9], (e[6] - e[7]) & 0xFFFFFFFF) for e in again] == [(e[2], e[9], e[6] - e[7]) for e in events]
    assert len(events) <= max_events(-(-len(decisions) // FRAMES), s)


# ---------------- every settings bound in the library's walker, on audio ----------------

_bound = {}


def bound_plane(name):
    if not _bound:
        _bound.update({k: v[None, :].astype(np.float32) for k, v in bound_signals().items()})
    return _bound[name]


def measured(name, **kw):
    """the model's walker over a bound signal under settings that close nothing early: (closed segments, following steps)"""
    s = settings(**kw)
    frames = elt_model(bound_plane(name), **kw)[1][0]
    wk = Walker(fresh_state(1)[0], s)
    for f, b in enumerate(frames["bin"]):
        wk.feed(int(b), f)
    return wk.closed, wk.steps


def test_the_bound_signals_measure_as_the_cases_say():
    """what bound_cases() places its settings on: sweep lengths, spans, gaps, steps and drops as the model's walker sees them"""
    length = lambda c: c[1] - c[0] + 1  # noqa: E731
    closed, steps = measured("4 Hz")
    assert {length(c) for c in closed} == {50, 51} and length(closed[0]) == 51 and {c[6] for c in closed[1:]} == {1} and max(steps) == (1, 0)
    assert {abs(c[2] - c[3]) for c in measured("700 Hz wide")[0]} == {11}
    closed, steps = measured("10 Hz", min_len=20)
    assert {length(c) for c in closed} == {20, 21} and max(a for a, _ in steps) == 2 and all(c[5] for c in closed)
    closed, steps = measured("10 Hz, a frame punched", min_len=20, max_step=31)
    assert max(d for _, d in steps) == 1 and {a for a, d in steps if d == 1} == {4} and max(a for a, d in steps if d == 0) == 2
    closed, _ = measured("a pause", max_gap=1024)
    assert [c[6] for c in closed if c[5]][:4] == [None, 1, 1, 24]
    closed, _ = measured("a narrow sweep inside", max_gap=1024)
    assert [(c[5], c[6]) for c in closed][:5] == [(True, None), (True, 1), (True, 1), (False, None), (True, 68)] and abs(closed[3][2] - closed[3][3]) == 8
    closed, _ = measured("six sweeps at 4 Hz, then silence")
    assert [length(c) for c in closed] == [51, 50, 50, 50, 50, 51]
    assert sum(c[5] for c in measured("five sweeps")[0]) == 5 and sum(c[5] for c in measured("six sweeps")[0]) == 6
    for name, drops in (("two frames punched", 2), ("three frames punched", 3)):
        assert max(d for _, d in measured(name, max_drop=4)[1]) == drops


@pytest.mark.parametrize("case", bound_cases(), ids=[c[0] for c in bound_cases()])
@pytest.mark.parametrize("cuts", [(BOUND_NB,), (7, 25)])
def test_twin_on_both_sides_of_every_settings_bound(pkg, case, cuts):
    """mi_elt_plan_host -- mi::elt_step, the text the device runs too -- against the model on audio whose sweeps sit exactly on a
    setting and one beyond it: the bytes, and what must and must not be raised"""
    name, signal, kw, kinds, first_frame = case
    plane, cfg = bound_plane(signal), pkg.elt_cfg(**kw)
    state, done, events = fresh_state(1), 0, []
    for i, (n, want) in enumerate(zip(cuts, run_in_calls(plane, cuts, **kw))):
        state = check_twin_call(pkg, f"{name}, call {i}", cfg, [1], plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], n, state, want)
        events += list(want[0])
        done += n
    assert [int(e["kind"]) for e in events] == kinds and (first_frame is None or events[0]["first_frame"] == first_frame), events
    if name == "a flip before the alarm":
        assert events[0]["dir"] == UP


def test_event_text(pkg):
    e = np.zeros(1, EVENT_REC)
    e["kind"], e["dir"], e["bin_from"], e["bin_to"], e["frame"], e["first_frame"], e["sweeps"] = ONSET, DOWN, 24, 8, 401, 0, 6
    assert pkg.elt_event_text(e[0]) == "ONSET down 1500.0 -> 500.0 Hz, 6 sweeps, 2.005 s"
    e["kind"], e["dir"], e["bin_from"], e["bin_to"], e["frame"], e["first_frame"], e["sweeps"] = END, UP, 5, 26, 3, 0xFFFFFFFD, 40
    assert pkg.elt_event_text(e[0]) == "END up 312.5 -> 1625.0 Hz, 40 sweeps, 0.030 s"
    for field, value in (("kind", 0), ("kind", 3), ("dir", 0), ("dir", 3), ("bin_from", 1), ("bin_to", 34)):
        bad = e.copy()
        bad[field] = value
        with pytest.raises(pkg.MiError) as err:
            pkg.elt_event_text(bad[0])
        assert err.value.code == pkg.MI_ERR_INVALID and "ELT stage" in str(err.value)


@pytest.mark.parametrize("what", ["white noise", "voice-like"])
def test_ten_minutes_through_the_twin_raise_nothing(pkg, what):
    nb, state, total = 600, None, 0
    rng = np.random.default_rng(90)
    for part in range(8):  # 8 x 75 s
        n = nb * WAVE_BATCH
        x = rng.normal(0.0, 0.2, n) if what == "white noise" else voice_like(n, 91 + part)
        events, _, _, _, state = pkg.elt_plan_host([1], x[None, :].astype(np.float32), state=state, want_frames=False)
        total += len(events)
    assert state.view(STATE)["frame"][0] == 8 * nb * FRAMES and total == 0, f"{what}: {total} events in ten minutes"
