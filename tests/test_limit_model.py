"""The peak limiter stage's definition, pinned without a GPU: mi_limit_plan_host (csrc/poststage_host.cpp) against the numpy model of
limit_model.py as bytes -- the plane and the state blob --, the four consequences the header draws from the definition at the indices
it states, mi_limit_pregain_host against a sort in Python, the exported symbols and every refusal that needs no handle (a handle
needs a device: test_gpu_limit.py has the refusals of mi_limit_process_device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import limit_model as lm
from limit_model import CEILING, HISTORY, LOOKAHEAD, WAVE_BATCH, WINDOW, audio, limit_model, settings_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_SYMBOLS = {"mi_limit_default_row", "mi_limit_create", "mi_limit_destroy", "mi_limit_set_rows", "mi_limit_process_device", "mi_limit_state_size",
                 "mi_limit_get_state", "mi_limit_set_state", "mi_limit_set_timing", "mi_limit_last_launch_ms", "mi_limit_plan_host", "mi_limit_pregain_host"}
SENT = np.float32(-7.5)  # no output of the stage: it clamps to a ceiling of 1 at the most
INVALID, NO_DEVICE = -1, -2
ROW_BYTES = 4344
CUTS = [(4,), (1, 3), (2, 1, 1)]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def in_calls(pkg, wave, cfg, cuts):
    """the twin over consecutive calls of the lengths `cuts`, the state carried through the blob -> (the planes side by side, state)"""
    rows, state, done, outs = wave.shape[0], None, 0, []
    for n in cuts:
        part = np.ascontiguousarray(wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH])
        got, state = pkg.limit_plan_host(np.ones(rows), part, cfg, state)
        outs.append(got)
        done += n
    return np.concatenate(outs, axis=1), state


# ---------------- the twin against the model ----------------

@pytest.mark.parametrize("kind", ["one", "three", "per_row"])
@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("rows", [1, 5])
def test_twin_equals_model_on_every_builder(pkg, rows, nb, kind):
    """a call of nb batches and one more batch behind it, whose 1086 samples of history are the carried state; the blob is the row's
    last 1086 input samples, and nothing leaves the ceiling"""
    for name in lm.BUILDERS:
        cfg = settings_for(name, rows, kind)
        wave = audio(name, rows, nb + 1)
        state = model_state = None
        for lo, hi in ((0, nb), (nb, nb + 1)):
            part = np.ascontiguousarray(wave[:, lo * WAVE_BATCH:hi * WAVE_BATCH])
            want, model_state = limit_model(part, cfg, model_state)
            got, state = pkg.limit_plan_host(np.ones(rows), part, cfg, state)
            assert got.tobytes() == want.tobytes(), f"{name}: plane, batches {lo} .. {hi}"
            assert state.tobytes() == model_state.tobytes(), f"{name}: state"
            assert state.view(np.float32).reshape(rows, HISTORY).tobytes() == part[:, -HISTORY:].tobytes()
            for r in range(rows):
                assert (np.abs(got[r]) <= np.float32(cfg[r][1])).all(), f"{name}, row {r}: over the ceiling"


@pytest.mark.parametrize("cuts", CUTS)
def test_call_cuts_give_identical_planes(pkg, cuts):
    """the same 4 batches as one call, as 1 + 3 and as 2 + 1 + 1, the state carried through the blob: a block's history comes from
    the row's previous batch or from the carried state, and the bytes do not depend on which"""
    rows, nb = 5, 4
    for name in lm.BUILDERS:
        cfg = settings_for(name, rows, "three")
        wave = audio(name, rows, nb)
        whole, whole_state = limit_model(wave, cfg)
        got, state = in_calls(pkg, wave, cfg, cuts)
        assert got.tobytes() == whole.tobytes() and state.tobytes() == whole_state.tobytes(), f"{name}, cuts {cuts}"


def test_a_disabled_row_padded_strides_and_sentinels(pkg):
    """rows 1 and 3 sit the second of three calls out: their output rows keep the sentinel, their carried samples keep their bytes,
    and the third call continues from the first call's tail.  The planes are laid out for a batch more than the call (input) and two
    more (output); nothing behind the call is read (it holds 5.0: a stage that read it would turn the gain down) or written."""
    rows, n = 5, 2
    cfg = settings_for("loud_noise", rows, "per_row")
    wave = audio("loud_noise", rows, 3 * n)
    masks = [np.ones(rows, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(rows, np.uint8)]
    state, model_state = None, None
    for i, en in enumerate(masks):
        w = np.full((rows, (n + 1) * WAVE_BATCH), np.float32(5.0))
        w[:, :n * WAVE_BATCH] = wave[:, i * n * WAVE_BATCH:(i + 1) * n * WAVE_BATCH]
        out = np.full((rows, (n + 2) * WAVE_BATCH + 4), SENT)
        want, model_state = limit_model(w, cfg, model_state, en, nbatches=n, out=out)
        got, state = pkg.limit_plan_host(en, w, cfg, state, nbatches=n, out=out.copy())
        assert got.tobytes() == want.tobytes() and state.tobytes() == model_state.tobytes(), f"call {i}"
        assert (got[:, n * WAVE_BATCH:] == SENT).all() and (got[en == 0] == SENT).all() and (got[en == 1, :n * WAVE_BATCH] != SENT).all()
        tails = state.view(np.float32).reshape(rows, HISTORY)
        assert tails[0].tobytes() == w[0, n * WAVE_BATCH - HISTORY:n * WAVE_BATCH].tobytes()
        held = (1 if i == 1 else i + 1) * n * WAVE_BATCH
        assert tails[1].tobytes() == wave[1, held - HISTORY:held].tobytes()


def test_set_rows_counts_the_carried_samples_under_the_new_pregain(pkg):
    """the state holds x, not u: a sample of 0.5 at the end of a call under pregain 1 is under the ceiling there, and turns the gain
    of the next call down when that call runs under pregain 4 -- as if the whole sequence had run under 4"""
    first = np.full((1, WAVE_BATCH), np.float32(0.1))
    first[0, -1] = 0.5
    second = np.full((1, WAVE_BATCH), np.float32(0.1))
    quiet, state = pkg.limit_plan_host([1], first, (1.0, float(CEILING)))
    assert quiet[0, LOOKAHEAD:].tobytes() == first[0, :-LOOKAHEAD].tobytes()
    got, after = pkg.limit_plan_host([1], second, (4.0, float(CEILING)), state)
    whole, _ = limit_model(np.concatenate([first, second], axis=1), (4.0, float(CEILING)))
    assert got.tobytes() == whole[:, WAVE_BATCH:].tobytes() == limit_model(second, (4.0, float(CEILING)), state)[0].tobytes()
    u = np.float32(0.1) * np.float32(4.0)
    assert CEILING * (1 - 1e-5) <= got[0, LOOKAHEAD - 1] <= CEILING, "the carried sample under the new pregain, held at the ceiling"
    assert (got[0, LOOKAHEAD:WINDOW - 1] < u).all() and (got[0, WINDOW + LOOKAHEAD:] == u).all()
    assert after.view(np.float32).tobytes() == second[0, -HISTORY:].tobytes()


# ---------------- what follows from the definition ----------------

def own_run(name, rows=2, nb=3):
    """(wave, cfg, the model's plane over the whole of it) at the builder's own settings"""
    wave = audio(name, rows, nb)
    cfg = settings_for(name, rows, "one")
    return wave, cfg, limit_model(wave, cfg)[0]


def test_builders_reach_what_they_are_for():
    for name in lm.BUILDERS:
        wave, cfg, _ = own_run(name)
        over = (np.abs(wave * np.float32(cfg[0][0])) > np.float32(cfg[0][1])).any()
        assert over == (name not in lm.UNDER_CEILING), name
    assert 2.4 < np.abs(audio("four_voices", 2, 3)).max() <= 2.5 and np.abs(audio("voice", 2, 3)).max() <= 0.7
    sub = audio("subnormal", 2, 3)
    assert (np.abs(sub) < 2.0 ** -125).all() and (sub != 0).all()
    assert np.signbit(audio("minus_zero", 1, 2)).all()
    # the carried places: after every batch but the last, the state holds the peak at the place the name says, or not at all
    for name, back in (("carried_1", 1), ("carried_63", 63), ("carried_1023", 1023), ("carried_1024", 1024), ("carried_1086", 1086), ("beyond_history", None)):
        wave = audio(name, 1, 3)
        _, state = limit_model(wave[:, :2 * WAVE_BATCH])
        at = np.flatnonzero(np.abs(state["x"][0]) == lm.PEAK)
        assert at.tolist() == ([] if back is None else [HISTORY - back]), name
        last, _ = limit_model(wave[:, 2 * WAVE_BATCH:], state=state)
        gain_moved = last[0, LOOKAHEAD:].tobytes() != wave[0, 2 * WAVE_BATCH:-LOOKAHEAD].tobytes() or last[0, :LOOKAHEAD].tobytes() != wave[0, 2 * WAVE_BATCH - LOOKAHEAD:2 * WAVE_BATCH].tobytes()
        assert gain_moved == (back is not None), f"{name}: the last call's gain"


def test_ceiling_holds_on_every_builder(pkg):
    for name in lm.BUILDERS:
        for kind in ("one", "three", "per_row"):
            wave = audio(name, 5, 3)
            cfg = settings_for(name, 5, kind)
            got, _ = pkg.limit_plan_host(np.ones(5), wave, cfg)
            for r in range(5):
                assert np.abs(got[r]).max() <= np.float32(cfg[r][1]), f"{name}, {kind}, row {r}"


def test_under_the_ceiling_the_stage_is_a_delay(pkg):
    """out[n] is x[n - 63] * pregain bit for bit, signed zeros and subnormal values included; the first 63 outputs carry the fresh
    state's zeros times the pregain"""
    for name in lm.UNDER_CEILING:
        for pregain in (1.0, 0.75):
            wave = audio(name, 2, 3)
            got, _ = pkg.limit_plan_host([1, 1], wave, (pregain, float(CEILING)))
            want = np.concatenate([np.zeros((2, LOOKAHEAD), np.float32), wave[:, :-LOOKAHEAD]], axis=1) * np.float32(pregain)
            assert got.tobytes() == want.tobytes() == limit_model(wave, (pregain, float(CEILING)))[0].tobytes(), f"{name} under pregain {pregain}"


@pytest.mark.parametrize("name,q", list(lm.LONE_PEAKS.items()))
def test_timeline_of_a_lone_peak(pkg, name, q):
    """the gain (out over the delayed input, which the bed keeps off zero) leaves 1.0 first for the output that carries input sample
    q - 63 (or at the row's first sample where q < 63), is lowest and within the header's rounding of ceiling / a[q] for input samples
    q .. q + 960, and is exactly 1.0 again from input sample q + 1024 on"""
    wave = audio(name, 1, 3)
    got, _ = pkg.limit_plan_host([1], wave)
    x, out = wave[0], got[0]
    assert np.abs(x[q]) == lm.PEAK and np.count_nonzero(np.abs(x) > CEILING) == 1
    first = max(q - LOOKAHEAD, 0)  # input sample
    carried = lambda i: out[i + LOOKAHEAD]  # the output that carries input sample i
    for i in range(0, first):
        assert carried(i).tobytes() == x[i].tobytes(), f"input sample {i}: the gain has left 1.0 early"
    assert carried(first) != x[first] and abs(carried(first)) < abs(x[first])
    floor = np.float32(CEILING / lm.PEAK)
    for i in range(q, q + WINDOW - LOOKAHEAD):
        gain = np.float64(carried(i)) / np.float64(x[i])
        assert gain <= np.float64(floor) * (1 + 80 * 2.0 ** -24), f"input sample {i}: gain {gain}"
        assert gain >= np.float64(floor) * (1 - 80 * 2.0 ** -24), f"input sample {i}: gain {gain} under the lone peak's"
    assert abs(carried(q)) <= CEILING
    for i in range(q + WINDOW - LOOKAHEAD, q + WINDOW):  # the release: between the floor and 1.0, rising
        gain = np.float64(carried(i)) / np.float64(x[i])
        assert np.float64(floor) * (1 - 80 * 2.0 ** -24) <= gain < 1.0
    assert out[q + WINDOW + LOOKAHEAD:].tobytes() == x[q + WINDOW:len(x) - LOOKAHEAD].tobytes(), "the gain is 1.0 again from input sample q + 1024 on"


def test_steady_tone_is_scaled_by_one_number(pkg):
    """a steady 1 kHz tone at twice the ceiling: from output sample 1086 on the output is the delayed input times one float32 gain,
    the product rounded once -- no distortion"""
    wave = audio("loud_tone", 2, 3)
    got, _ = pkg.limit_plan_host([1, 1], wave)
    for r in range(2):
        peak = np.abs(wave[r]).max()
        r1 = np.float32(CEILING) / peak
        s = np.float32(0.0)
        for _ in range(LOOKAHEAD + 1):
            s = np.float32(s + r1)
        g = np.float32(s * np.float32(0.015625))
        want = wave[r, HISTORY - LOOKAHEAD:-LOOKAHEAD] * g
        assert got[r, HISTORY:].tobytes() == np.clip(want, -CEILING, CEILING).tobytes()
        assert 0.49 < float(g) < 0.51


def test_mixer_row_figures(pkg):
    """printed, not asserted: what the stage does to the level of a mixer's row"""
    wave = audio("four_voices", 1, 4)
    got, _ = pkg.limit_plan_host([1], wave)
    _, g = lm.gains(np.concatenate([np.zeros(HISTORY, np.float32), wave[0]]), *lm.DEFAULT_ROW)
    rms = lambda v: float(np.sqrt(np.mean(np.asarray(v, np.float64) ** 2)))
    print(f"four voices: output RMS / input RMS = {rms(got[0]) / rms(wave[0]):.4f}, share of samples with a gain below 1: {float(np.mean(g < 1)):.4f}")


# ---------------- the pregain helper ----------------

def records_of(pkg, rows):
    """[(row, nblocks, peak)] -> records"""
    rec = np.zeros(len(rows), pkg.TX_RECORD_DTYPE)
    for i, (row, nblocks, peak) in enumerate(rows):
        rec[i]["row"], rec[i]["nblocks"], rec[i]["peak"], rec[i]["seq"] = row, nblocks, peak, i + 1
    return rec


def pregain_by_sorting(rows, row, ceiling, percentile):
    peaks = sorted(np.float32(p) for r, nb, p in rows if r == row and nb > 0 and p > 0)
    if not peaks:
        return np.float32(1.0), 0
    peak = peaks[(len(peaks) - 1) * (percentile or 90) // 100]
    return np.clip(np.float32(ceiling) / peak, np.float32(2.0 ** -10), np.float32(2.0 ** 10)), len(peaks)


def test_pregain_helper(pkg):
    rng = np.random.default_rng(7)
    rows = [(int(rng.integers(0, 3)), int(rng.integers(0, 4)), float(rng.choice([0.0, 0.05, 0.2, 0.2, 0.4, 0.9, 1.0]) * rng.choice([1.0, 1.0, 0.37]))) for _ in range(200)]
    rec = records_of(pkg, rows)
    for row in (0, 1, 2, 3):  # (3: no record of that row)
        for percentile in (0, 1, 50, 89, 90, 99, 100):
            for ceiling in (float(CEILING), 0.0625, 1.0):
                got = pkg.limit_pregain_host(rec, row, ceiling, percentile)
                want = pregain_by_sorting(rows, row, ceiling, percentile)
                assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], (row, percentile, ceiling)
    assert pkg.limit_pregain_host(rec, 3) == (np.float32(1.0), 0) and pkg.limit_pregain_host(rec[:0], 0) == (np.float32(1.0), 0)
    assert pkg.limit_pregain_host(records_of(pkg, [(0, 0, 0.5), (0, 2, 0.0), (1, 2, 0.5)]), 0) == (np.float32(1.0), 0)
    # ties, and the percentile's edges on five records: indices 4 * p // 100
    five = records_of(pkg, [(0, 1, p) for p in (0.5, 0.125, 0.25, 0.25, 1.0)])
    for percentile, peak in ((1, 0.125), (24, 0.125), (25, 0.25), (50, 0.25), (74, 0.25), (75, 0.5), (0, 0.5), (99, 0.5), (100, 1.0)):
        assert pkg.limit_pregain_host(five, 0, 0.5, percentile) == (np.float32(0.5 / peak), 5), percentile
    # the clamp at both ends
    assert pkg.limit_pregain_host(records_of(pkg, [(0, 1, 1e-6)]), 0, 1.0, 100) == (np.float32(1024.0), 1)
    assert pkg.limit_pregain_host(records_of(pkg, [(0, 1, 5000.0)]), 0, 0.0625, 100) == (np.float32(2.0 ** -10), 1)
    assert pkg.limit_pregain_host(records_of(pkg, [(0, 1, 1.0 / 1024)]), 0, 1.0, 100) == (np.float32(1024.0), 1)
    L = pkg.lib()
    g, used = C.c_float(), C.c_uint32()
    for bad, text in ((dict(ceiling=0.06), b"limiter pregain: ceiling must be finite and within 0.0625 .. 1"), (dict(ceiling=1.5), None), (dict(ceiling=float("nan")), None),
                      (dict(ceiling=float("inf")), None), (dict(percentile=101), b"limiter pregain: percentile must be 1 .. 100, or 0 for 90"),
                      (dict(records=None), b"NULL argument"), (dict(g=None), b"NULL argument"), (dict(used=None), b"NULL argument")):
        a = dict(records=ptr(five), n=5, row=0, ceiling=0.5, percentile=0, g=C.byref(g), used=C.byref(used))
        a.update(bad)
        assert L.mi_limit_pregain_host(*a.values()) == INVALID, bad
        if text:
            assert L.mi_last_error() == text
    assert L.mi_limit_pregain_host(None, 0, 0, 0.5, 0, C.byref(g), C.byref(used)) == 0 and g.value == 1.0 and used.value == 0


# ---------------- sizes, symbols, refusals ----------------

def test_sizes_symbols_and_the_default_row(pkg):
    assert C.sizeof(pkg.LimitRow) == 8 and pkg.LIMIT_ROW_DTYPE.itemsize == 8 and pkg.LIMIT_STATE_DTYPE.itemsize == ROW_BYTES == 4 * HISTORY
    assert (pkg.LIMIT_LOOKAHEAD, pkg.LIMIT_WINDOW, pkg.LIMIT_HISTORY) == (LOOKAHEAD, WINDOW, HISTORY) == (63, 1024, 1086)
    assert pkg.lib().mi_limit_state_size(None) == 0
    d = pkg.limit_default_row()
    assert (np.float32(d[0]), np.float32(d[1])) == lm.DEFAULT_ROW and abs(20 * np.log10(d[1]) + 1.0) < 1e-6
    wave = audio("loud_noise", 2, 1)
    assert pkg.limit_plan_host([1, 1], wave)[0].tobytes() == pkg.limit_plan_host([1, 1], wave, lm.DEFAULT_ROW)[0].tobytes()
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    assert "MI_LIMIT_LOOKAHEAD = 63, MI_LIMIT_WINDOW = 1024, MI_LIMIT_HISTORY = 1086, MI_LIMIT_STATE_ROW_BYTES = 4344" in header
    section = header[header.index("peak limiter stage"):header.index("enum { MI_LIMIT_LOOKAHEAD")]
    assert "MI_GATE_OPEN_TRAIL" in section and "no stereo link" in section and "synthetic signals only" in section
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_limit")}
    assert declared == LIMIT_SYMBOLS and LIMIT_SYMBOLS <= set(pkg.ABI_SYMBOLS)
    assert all(hasattr(pkg.lib(), s) for s in LIMIT_SYMBOLS)


PREGAIN_TEXT = b"limiter stage: pregain must be finite and within 2^-10 .. 2^10"
CEILING_TEXT = b"limiter stage: ceiling must be finite and within 0.0625 .. 1"
F = np.float32
BAD_SETTINGS = [((float("nan"), 0.5), PREGAIN_TEXT), ((float("inf"), 0.5), PREGAIN_TEXT), ((float("-inf"), 0.5), PREGAIN_TEXT), ((0.0, 0.5), PREGAIN_TEXT),
                ((-1.0, 0.5), PREGAIN_TEXT), ((np.nextafter(F(2.0 ** -10), F(0)), 0.5), PREGAIN_TEXT), ((np.nextafter(F(1024), F(2048)), 0.5), PREGAIN_TEXT),
                ((1.0, float("nan")), CEILING_TEXT), ((1.0, float("inf")), CEILING_TEXT), ((1.0, 0.0), CEILING_TEXT), ((1.0, -0.5), CEILING_TEXT),
                ((1.0, np.nextafter(F(0.0625), F(0))), CEILING_TEXT), ((1.0, np.nextafter(F(1), F(2))), CEILING_TEXT)]
GOOD_SETTINGS = [(2.0 ** -10, 0.0625), (1024.0, 1.0), (1.0, float(CEILING)), (2.0 ** -10, 1.0), (1024.0, 0.0625)]


def rows_of(pkg, *pairs):
    return np.array(pairs, np.float32).view(pkg.LIMIT_ROW_DTYPE).reshape(-1)


def test_both_sides_of_every_settings_bound(pkg):
    wave = np.zeros((1, WAVE_BATCH), np.float32)
    for s in GOOD_SETTINGS:
        assert lm.settings_ok(*s)
        pkg.limit_plan_host([1], wave, s)
    for s, text in BAD_SETTINGS:
        assert not lm.settings_ok(F(s[0]), F(s[1]))
        for en in ([1], [0]):  # (those of a disabled row too)
            with pytest.raises(pkg.MiError) as e:
                pkg.limit_plan_host(en, wave, s)
            assert e.value.code == pkg.MI_ERR_INVALID and pkg.lib().mi_last_error() == text, s


def test_refusals(pkg):
    L = pkg.lib()
    null = b"NULL argument"

    def refused(rc, code=INVALID, text=None):
        assert rc == code
        if text is not None:
            assert L.mi_last_error() == text

    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(8192, np.uint8)
    good = rows_of(pkg, *[lm.DEFAULT_ROW] * 4)
    refused(L.mi_limit_create(ptr(good), None, 4, 1, 0, C.byref(out)), text=null)
    refused(L.mi_limit_create(ptr(good), ptr(en), 4, 1, 0, None), text=null)
    geometry = b"limiter stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
    for rows, max_batches in ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, 1 << 12), ((1 << 20) - 1, 17)):
        refused(L.mi_limit_create(None, ptr(en), rows, max_batches, 0, C.byref(out)), text=geometry)
    for bad, text in BAD_SETTINGS:  # (the arguments alone decide: before a device is looked for; a bad row anywhere, a disabled one too)
        for at in (0, 3):
            cfg = rows_of(pkg, *[lm.DEFAULT_ROW if r != at else bad for r in range(4)])
            refused(L.mi_limit_create(ptr(cfg), ptr(np.array([1, 1, 1, 0], np.uint8)), 4, 1, 0, C.byref(out)), text=text)
    assert not out.value
    if pkg.device_count() < 1:
        for cfg in (None, ptr(good)):
            refused(L.mi_limit_create(cfg, ptr(en), 4, 1, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the limiter stage runs on the GPU only")
        assert not out.value
        with pytest.raises(pkg.MiError) as e:
            pkg.Limit(np.ones(3), max_batches=2)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE
    # a NULL handle, before anything else
    refused(L.mi_limit_set_rows(None, ptr(good), ptr(en)), text=null)
    refused(L.mi_limit_process_device(None, ptr(some), 0, 1, ptr(some), 0, None), text=null)
    refused(L.mi_limit_set_timing(None, 1), text=null)
    refused(L.mi_limit_last_launch_ms(None, ptr(some)), text=null)
    refused(L.mi_limit_get_state(None, ptr(some), ROW_BYTES), text=b"limiter stage state: NULL argument or wrong length")
    refused(L.mi_limit_set_state(None, ptr(some), ROW_BYTES), text=b"limiter stage state: NULL argument or wrong length")
    assert L.mi_limit_state_size(None) == 0
    L.mi_limit_destroy(None)
    # the twin
    rows, nb = 2, 2
    n = nb * WAVE_BATCH
    wave, plane, state = np.zeros((rows, n), np.float32), np.zeros((rows, n), np.float32), np.zeros(rows * ROW_BYTES, np.uint8)
    cfg2 = rows_of(pkg, (1.0, 0.5), (2.0, 1.0))

    def plan(**over):
        a = dict(cfg=ptr(cfg2), en=ptr(en), rows=rows, nb=nb, wave=ptr(wave), row_stride=n, state=ptr(state), out=ptr(plane), out_stride=n)
        a.update(over)
        return L.mi_limit_plan_host(*a.values())

    assert plan() == 0 and plan(cfg=None) == 0
    for name in ("en", "wave", "state", "out"):
        refused(plan(**{name: None}), text=null)
    for bad, text in BAD_SETTINGS:
        refused(plan(cfg=ptr(rows_of(pkg, (1.0, 0.5), bad))), text=text)
    for over in (dict(rows=0), dict(rows=-1), dict(nb=0), dict(nb=-1)):
        refused(plan(**over), text=b"limit plan needs rows >= 1 and nbatches >= 1")
    for over in (dict(row_stride=n - 1), dict(out_stride=n - 1)):
        refused(plan(**over), text=b"a row stride is shorter than the call")
    # overlap of input and output: the same plane, a shifted one, the output's last float on the input's first and the reverse
    overlap = b"the output overlaps the input plane"
    big = np.zeros(4 * rows * n, np.float32)
    at = lambda i: C.c_void_p(big.ctypes.data + 4 * i)
    span = rows * n
    for w_at, o_at in ((0, 0), (0, 1), (1, 0), (0, span - 1), (span - 1, 0), (100, n)):
        refused(plan(wave=at(w_at), out=at(o_at)), text=overlap)
    assert plan(wave=at(0), out=at(span)) == 0 and plan(wave=at(span), out=at(0)) == 0
    # (rows interleaved in one allocation overlap as ranges: refused, though no float is shared)
    refused(plan(wave=at(0), row_stride=2 * n, out=at(n), out_stride=2 * n), text=overlap)
