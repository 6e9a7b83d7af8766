"""The noise reduction stage's definition, pinned without a GPU: the window, mi_denoise_plan_host (csrc/poststage_host.cpp) against
the numpy model of denoise_model.py as bytes -- the plane and the state blob --, the float32 model against its float64 restatement,
what the stage does to noise, to a steady tone and to silence, the exported symbols and every refusal."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import denoise_model as dm
from denoise_model import BINS, DEPTH, FRAME, HOP, THREE_CLASSES, WAVE_BATCH, audio, denoise_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENOISE_SYMBOLS = {"mi_denoise_default_row", "mi_denoise_create", "mi_denoise_destroy", "mi_denoise_set_rows", "mi_denoise_process_device",
                   "mi_denoise_state_size", "mi_denoise_get_state", "mi_denoise_set_state", "mi_denoise_set_timing", "mi_denoise_last_launch_ms",
                   "mi_denoise_window", "mi_denoise_plan_host"}
SENT = np.float32(-7.5)  # no output of the stage: it clamps to [-1, 1]
INVALID, NO_DEVICE = -1, -2
ROW_BYTES = 9196
# tools/denoise_classes.py at the default row (12 dB, over 4.5), seed 0, through the host twin: the level of white noise of deviation
# 0.03 in the last second of three, and of a 1 kHz tone 10 dB above that noise in its bin over the same second
NOISE_REDUCTION_DB, TONE_CHANGE_DB = -9.18, -11.97
# The largest |float32 model - float64 restatement| of a block over the largest |x| of the 2500 samples the block depends on, over
# every builder but three at 2 rows x 5 batches, stepping_noise and tx_after_silence at 13 as well, at the default row and at two
# other rows: 3.6e-7 (the square wave; white noise 1.2e-7 to 1.6e-7, the stepping noise 2.3e-7, a lone sample 1.1e-7).  Asserted is
# four times that, the margin of the spectrum stage.  The three left out are
# silence and -0.0, where both sides are exactly zero and that is asserted instead, and the subnormal values: their float32 P
# underflows to zero, so the float32 gain is g_min by definition where the float64 one is not, and the difference is the definition's.
F64_MEASURED = 3.6e-7
F64_BOUND = 4 * F64_MEASURED


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def classes_for(rows, kind):
    """one class, three classes, or one class per row"""
    if kind == "one":
        return [dm.DEFAULT_ROW] * rows
    if kind == "three":
        return [THREE_CLASSES[r % 3] for r in range(rows)]
    return [(3.0 + 4.0 * r, 0.5 + 1.25 * r) for r in range(rows)]


# ---------------- window ----------------

def test_window(pkg):
    w, want, w64 = pkg.denoise_window(), dm.window(), dm.window64()
    assert w.dtype == np.float32 and w.shape == (FRAME,)
    assert (np.abs(w.astype(np.float64) - w64) <= np.spacing(want).astype(np.float64)).all(), "more than one float32 step from the formula"
    assert w.tobytes() == w[::-1].tobytes(), "not symmetric bit for bit"
    unit = w.astype(np.float64)[:HOP] ** 2 + w.astype(np.float64)[HOP:] ** 2
    assert (np.abs(unit - 1.0) <= 2 * np.spacing(np.float32(1.0))).all(), "w^2 does not overlap to 1 within two float32 steps"


def test_default_row(pkg):
    assert pkg.denoise_default_row() == dm.DEFAULT_ROW == (12.0, 4.5)
    wave = audio("noise_mid", 2, 1)
    assert pkg.denoise_plan_host([1, 1], wave)[0].tobytes() == pkg.denoise_plan_host([1, 1], wave, dm.DEFAULT_ROW)[0].tobytes()


# ---------------- the twin against the model ----------------

@pytest.mark.parametrize("kind", ["one", "three", "per_row"])
@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("rows", [1, 5])
def test_twin_equals_model_on_every_builder(pkg, rows, nb, kind):
    """a call of nb batches and one more batch behind it, whose first frames reach into the carried samples and whose m reads the
    carried minima"""
    cfg = classes_for(rows, kind)
    for name in dm.BUILDERS:
        wave = audio(name, rows, nb + 1)
        state = model_state = None
        for lo, hi in ((0, nb), (nb, nb + 1)):
            part = np.ascontiguousarray(wave[:, lo * WAVE_BATCH:hi * WAVE_BATCH])
            want, model_state = denoise_model(part, cfg, model_state)
            got, state = pkg.denoise_plan_host(np.ones(rows), part, cfg, state)
            assert got.tobytes() == want.tobytes(), f"{name}: plane, batches {lo} .. {hi}"
            assert state.tobytes() == model_state.tobytes(), f"{name}: state"
            assert state.view(pkg.DENOISE_STATE_DTYPE)["x"].tobytes() == part[:, -FRAME:].tobytes()
            assert (np.abs(got) <= 1).all()


@pytest.mark.parametrize("cuts", [(12,), (5, 7), (1,) * 12])
def test_twelve_batches_and_their_cuts(pkg, cuts):
    """12 batches as one call, as 5 + 7 and as twelve calls of one, and a batch behind them: the sliding minimum reads the carried
    rows and the call's own, and a block's bytes do not depend on where its 500 samples of history and its seven earlier M came from"""
    rows, nb = 5, 12
    cfg = classes_for(rows, "three")
    for name in ("stepping_noise", "tx_after_silence", "gated_noise"):
        wave = audio(name, rows, nb + 1)
        whole, whole_state = denoise_model(wave, cfg)
        state, done = None, 0
        for n in cuts + (1,):
            part = np.ascontiguousarray(wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH])
            got, state = pkg.denoise_plan_host(np.ones(rows), part, cfg, state)
            assert got.tobytes() == whole[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH].tobytes(), f"{name}, cuts {cuts}, batch {done}"
            done += n
        assert state.tobytes() == whole_state.tobytes()


def test_builders_reach_what_they_are_for():
    """silence and -0.0 give +0.0 throughout and leave M at +Inf; gated noise has silent frames beside counting ones and batches without
    a counting frame; the transmission's first batch has nothing but +Inf in front of it; the stepping noise moves m down at the step
    and up only eight batches later; a lone sample shows 250 samples later"""
    for name in ("silence", "minus_zero"):
        out, state = denoise_model(audio(name, 2, 2))
        assert (out.view(np.uint32) == 0).all() and np.isinf(state["m"]).all(), name
    g = audio("gated_noise", 5, 4)
    fr = dm._frames(np.concatenate([np.zeros((5, FRAME), np.float32), g], axis=1), 4)
    silent = (fr == 0).all(-1)
    assert silent.any() and (~silent).any() and (silent[:, 1:] != silent[:, :-1]).any()
    _, state = denoise_model(g)
    assert np.isinf(state["m"]).all(-1).any() and np.isfinite(state["m"]).all(-1).any()
    tx = audio("tx_after_silence", 1, 13)
    _, before = denoise_model(tx[:, :10 * WAVE_BATCH])
    assert np.isinf(before["m"]).all()
    _, after = denoise_model(tx[:, 10 * WAVE_BATCH:11 * WAVE_BATCH], state=before)
    assert np.isinf(after["m"][0, :-1]).all() and np.isfinite(after["m"][0, -1]).all()
    step = audio("stepping_noise", 1, 13)
    floors, state = [], None
    for b in range(13):
        _, state = denoise_model(step[:, b * WAVE_BATCH:(b + 1) * WAVE_BATCH], state=state)
        floors.append(float(state["m"][0, -1].astype(np.float64).mean()))
    assert max(floors[4:8]) < 0.05 * min(floors[:4]) and min(floors[9:]) > 20 * max(floors[4:8])  # 20 dB in power is a factor of 100
    for at in (0, 249, 250, 1999):
        x = audio(f"lone_{at}", 1, 2)
        out, _ = denoise_model(x, (0.0, 0.0))
        assert abs(out[0, at + HOP] - 0.75) < 1e-6 and np.abs(np.delete(out[0], at + HOP)).max() < 1e-6


def test_a_disabled_row_padded_strides_and_sentinels(pkg):
    """rows 1 and 3 sit the second of three calls out: their output rows keep the sentinel and their state keeps its bytes.  The planes
    are laid out for a batch more than the call (input) and two more (output); nothing behind the call is read (it holds 0.5) or
    written."""
    rows, n = 5, 2
    cfg = classes_for(rows, "per_row")
    wave = audio("noise_mid", rows, 3 * n)
    masks = [np.ones(rows, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(rows, np.uint8)]
    state = model_state = held = None
    for i, en in enumerate(masks):
        w = np.full((rows, (n + 1) * WAVE_BATCH), np.float32(0.5))
        w[:, :n * WAVE_BATCH] = wave[:, i * n * WAVE_BATCH:(i + 1) * n * WAVE_BATCH]
        out = np.full((rows, (n + 2) * WAVE_BATCH + 4), SENT)
        want, model_state = denoise_model(w, cfg, model_state, en, nbatches=n, out=out)
        got, state = pkg.denoise_plan_host(en, w, cfg, state, nbatches=n, out=out.copy())
        assert got.tobytes() == want.tobytes() and state.tobytes() == model_state.tobytes(), f"call {i}"
        assert (got[:, n * WAVE_BATCH:] == SENT).all() and (got[en == 0] == SENT).all() and (got[en == 1, :n * WAVE_BATCH] != SENT).all()
        blob = state.view(pkg.DENOISE_STATE_DTYPE)
        assert blob["x"][0].tobytes() == w[0, n * WAVE_BATCH - FRAME:n * WAVE_BATCH].tobytes()
        if i == 1:
            assert blob[1].tobytes() == held[1].tobytes() and blob[3].tobytes() == held[3].tobytes()
        held = blob.copy()


# ---------------- float32 against float64 ----------------

def block_errors(wave, cfg=None):
    """per block: the largest |float32 model - float64 restatement| over the largest |x| of the 2500 samples the block depends on
    (None where those are all zero: then both outputs must be)"""
    o32, _ = denoise_model(wave, cfg)
    o64, _ = dm.denoise_model64(wave, cfg)
    x = np.concatenate([np.zeros((wave.shape[0], FRAME)), wave.astype(np.float64)], axis=1)
    errs = []
    for r in range(wave.shape[0]):
        for b in range(wave.shape[1] // WAVE_BATCH):
            top = np.abs(x[r, b * WAVE_BATCH:(b + 1) * WAVE_BATCH + FRAME]).max()
            seg = slice(b * WAVE_BATCH, (b + 1) * WAVE_BATCH)
            if top == 0:
                assert not o32[r, seg].any() and not o64[r, seg].any()
                continue
            errs.append(float(np.abs(o32[r, seg].astype(np.float64) - o64[r, seg]).max() / top))
    return errs


def test_float32_model_against_the_float64_restatement():
    worst = {}
    for name in dm.BUILDERS:
        if name == "subnormal":
            continue
        shapes = [(2, 5)] + ([(2, 13)] if name in ("stepping_noise", "tx_after_silence") else [])
        for rows, nb in shapes:
            for cfg in (None, THREE_CLASSES[1:]):
                errs = block_errors(audio(name, rows, nb), cfg)
                if name in ("silence", "minus_zero"):
                    assert not errs
                worst[name] = max([worst.get(name, 0.0)] + errs)
    print("largest difference per builder:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) <= F64_BOUND, worst


# ---------------- what the stage is for ----------------

@pytest.mark.parametrize("cfg", [(0.0, 4.5), (12.0, 0.0), (0.0, 0.0)])
def test_reduction_0_and_over_0_give_a_pure_delay(pkg, cfg):
    for name in ("noise_mid", "voice_in_noise", "square", "stepping_noise"):
        x = audio(name, 2, 4)
        out, _ = pkg.denoise_plan_host([1, 1], x, cfg)
        assert out.tobytes() == denoise_model(x, cfg)[0].tobytes()
        delayed = np.concatenate([np.zeros((2, HOP)), x[:, :-HOP].astype(np.float64)], axis=1)
        err = np.abs(out.astype(np.float64) - delayed).max() / np.abs(x).max()
        print(f"{name}, {cfg}: {err:.2e}")
        assert err <= F64_BOUND


def test_white_noise_comes_out_reduced_and_a_steady_tone_with_it(pkg):
    """three seconds at the default row, the last second measured, against the figures tools/denoise_classes.py prints"""
    sec = 8 * WAVE_BATCH
    noise = dm.noise_at(1)(1, 24, 0)
    out, _ = pkg.denoise_plan_host([1], noise)
    reduction = dm.level_db(out[0, -sec:]) - dm.level_db(noise[0, -sec:])
    tone = dm.tone_in_noise(1, 24, 0)
    out, _ = pkg.denoise_plan_host([1], tone)
    change = 20.0 * math.log10(dm.tone_level(out[0, -sec:]) / dm.tone_level(tone[0, -sec:]))
    print(f"noise {reduction:+.2f} dB, tone {change:+.2f} dB")
    assert abs(reduction - NOISE_REDUCTION_DB) <= 1.0
    assert abs(change) < abs(TONE_CHANGE_DB) + 0.5


def test_silence_stays_exactly_zero(pkg):
    for name in ("silence", "minus_zero"):
        out, state = pkg.denoise_plan_host(np.ones(3), audio(name, 3, 4), THREE_CLASSES)
        blob = state.view(pkg.DENOISE_STATE_DTYPE)
        assert (out.view(np.uint32) == 0).all() and np.isinf(blob["m"]).all() and (blob["m"] > 0).all(), name


def test_the_first_batch_has_its_own_minimum_as_the_only_evidence(pkg):
    """a new handle's first batch: the frame of carried zeros is silent, so the frame behind it does not count and the other seven give
    M; the seven rows in front of it are +Inf, m is that M, and the plane is the model's.  Where a row's only frame that is not
    silent stands beside a silent one -- a lone sample at the very end of the batch -- nothing counts, M stays +Inf and the blob says
    so."""
    x = audio("noise_mid", 2, 1)
    out, state = pkg.denoise_plan_host([1, 1], x)
    want, model_state = denoise_model(x)
    assert out.tobytes() == want.tobytes() and state.tobytes() == model_state.tobytes()
    blob = state.view(pkg.DENOISE_STATE_DTYPE)
    assert np.isinf(blob["m"][:, :-1]).all() and np.isfinite(blob["m"][:, -1]).all() and (blob["m"][:, -1] > 0).all()
    out, state = pkg.denoise_plan_host([1], audio("lone_1999", 1, 1))
    assert np.isinf(state.view(pkg.DENOISE_STATE_DTYPE)["m"]).all() and out.tobytes() == denoise_model(audio("lone_1999", 1, 1))[0].tobytes()
    assert np.abs(out).max() < 1e-6  # (the sample itself shows in the next batch; this one holds the transform's rounding alone)


# ---------------- sizes, symbols, refusals ----------------

def test_sizes_and_symbols(pkg):
    assert C.sizeof(pkg.DenoiseRow) == 8 and pkg.DENOISE_ROW_DTYPE.itemsize == 8 and pkg.DENOISE_STATE_DTYPE.itemsize == ROW_BYTES == dm.STATE.itemsize
    assert (pkg.DENOISE_HOP, pkg.DENOISE_FRAME, pkg.DENOISE_FFT, pkg.DENOISE_BINS, pkg.DENOISE_DEPTH) == (HOP, FRAME, dm.FFT, BINS, DEPTH) == (250, 500, 512, 257, 8)
    assert pkg.lib().mi_denoise_state_size(None) == 0
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    for text in ("MI_DENOISE_HOP = 250", "MI_DENOISE_FRAME = 500", "MI_DENOISE_FFT = 512", "MI_DENOISE_BINS = 257", "MI_DENOISE_DEPTH = 8",
                 "MI_DENOISE_STATE_ROW_BYTES = 9196"):
        assert text in header, text
    section = header[header.index("noise reduction stage"):header.index("enum { MI_DENOISE_HOP")]
    assert "MI_GATE_OPEN_TRAIL" in section and "each block uses only its own gains" in section
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_denoise")}
    assert declared == DENOISE_SYMBOLS and DENOISE_SYMBOLS <= set(pkg.ABI_SYMBOLS)
    assert all(hasattr(pkg.lib(), s) for s in DENOISE_SYMBOLS)


DB_TEXT = b"noise reduction stage: reduction_db must be within 0 .. 40"
OVER_TEXT = b"noise reduction stage: over must be within 0 .. 64"
BAD_SETTINGS = [((-0.001, 4.5), DB_TEXT), ((40.001, 4.5), DB_TEXT), ((float("nan"), 4.5), DB_TEXT), ((float("inf"), 4.5), DB_TEXT),
                ((12.0, -0.001), OVER_TEXT), ((12.0, 64.001), OVER_TEXT), ((12.0, float("nan")), OVER_TEXT), ((12.0, float("inf")), OVER_TEXT)]
GOOD_SETTINGS = [(0.0, 0.0), (40.0, 64.0), (0.0, 64.0), (40.0, 0.0), (12.0, 4.5), (-0.0, -0.0)]


def rows_of(pkg, *pairs):
    return np.array(pairs, np.float32).view(pkg.DENOISE_ROW_DTYPE).reshape(-1)


def test_both_sides_of_every_settings_bound(pkg):
    L = pkg.lib()
    wave, plane = np.zeros((1, WAVE_BATCH), np.float32), np.zeros((1, WAVE_BATCH), np.float32)
    en = np.ones(1, np.uint8)
    for pair in GOOD_SETTINGS:
        state = pkg.denoise_fresh_state(1)
        assert dm.settings_ok(*pair)
        assert L.mi_denoise_plan_host(ptr(rows_of(pkg, pair)), ptr(en), 1, 1, ptr(wave), WAVE_BATCH, ptr(state), ptr(plane), WAVE_BATCH) == 0, pair
    for pair, text in BAD_SETTINGS:
        state = pkg.denoise_fresh_state(1)
        assert not dm.settings_ok(*pair)
        assert L.mi_denoise_plan_host(ptr(rows_of(pkg, pair)), ptr(en), 1, 1, ptr(wave), WAVE_BATCH, ptr(state), ptr(plane), WAVE_BATCH) == INVALID, pair
        assert L.mi_last_error() == text, pair
        with pytest.raises(pkg.MiError) as e:
            pkg.denoise_plan_host([1], wave, pair)
        assert e.value.code == pkg.MI_ERR_INVALID


def test_refusals(pkg):
    L = pkg.lib()
    null = b"NULL argument"

    def refused(rc, code=INVALID, text=None):
        assert rc == code
        if text is not None:
            assert L.mi_last_error() == text

    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(4 * ROW_BYTES, np.uint8)
    good = rows_of(pkg, *[dm.DEFAULT_ROW] * 4)
    refused(L.mi_denoise_create(ptr(good), None, 4, 1, 0, C.byref(out)), text=null)
    refused(L.mi_denoise_create(ptr(good), ptr(en), 4, 1, 0, None), text=null)
    geometry = b"noise reduction stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
    for rows, max_batches in ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, 1 << 12), ((1 << 20) - 1, 17)):
        refused(L.mi_denoise_create(None, ptr(en), rows, max_batches, 0, C.byref(out)), text=geometry)
    for bad, text in BAD_SETTINGS:  # (the arguments alone decide: before a device is looked for; a bad row anywhere, a disabled one too)
        for at in (0, 3):
            cfg = rows_of(pkg, *[dm.DEFAULT_ROW if r != at else bad for r in range(4)])
            refused(L.mi_denoise_create(ptr(cfg), ptr(np.array([1, 1, 1, 0], np.uint8)), 4, 1, 0, C.byref(out)), text=text)
    assert not out.value
    if pkg.device_count() < 1:
        for cfg in (None, ptr(good)):
            refused(L.mi_denoise_create(cfg, ptr(en), 4, 1, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the noise reduction stage runs on the GPU only")
        assert not out.value
        with pytest.raises(pkg.MiError) as e:
            pkg.Denoise(np.ones(3), max_batches=2)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE
    # a NULL handle, before anything else
    refused(L.mi_denoise_set_rows(None, ptr(good), ptr(en)), text=null)
    refused(L.mi_denoise_process_device(None, ptr(some), 0, 1, ptr(some), 0, None), text=null)
    refused(L.mi_denoise_set_timing(None, 1), text=null)
    refused(L.mi_denoise_last_launch_ms(None, ptr(some)), text=null)
    refused(L.mi_denoise_get_state(None, ptr(some), ROW_BYTES), text=b"noise reduction stage state: NULL argument or wrong length")
    refused(L.mi_denoise_set_state(None, ptr(some), ROW_BYTES), text=b"noise reduction stage state: NULL argument or wrong length")
    assert L.mi_denoise_state_size(None) == 0
    L.mi_denoise_destroy(None)
    refused(L.mi_denoise_window(None), text=null)
    # the twin
    rows, nb = 2, 2
    n = nb * WAVE_BATCH
    wave, plane, state = np.zeros((rows, n), np.float32), np.zeros((rows, n), np.float32), pkg.denoise_fresh_state(rows)
    cfg2 = rows_of(pkg, (12.0, 4.5), (20.0, 2.0))

    def plan(**over):
        a = dict(cfg=ptr(cfg2), en=ptr(en), rows=rows, nb=nb, wave=ptr(wave), row_stride=n, state=ptr(state), out=ptr(plane), out_stride=n)
        a.update(over)
        return L.mi_denoise_plan_host(*a.values())

    assert plan() == 0 and plan(cfg=None) == 0
    for name in ("en", "wave", "state", "out"):
        refused(plan(**{name: None}), text=null)
    for bad, text in BAD_SETTINGS:
        refused(plan(cfg=ptr(rows_of(pkg, (12.0, 4.5), bad))), text=text)
    for over in (dict(rows=0), dict(rows=-1), dict(nb=0), dict(nb=-1)):
        refused(plan(**over), text=b"denoise plan needs rows >= 1 and nbatches >= 1")
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
