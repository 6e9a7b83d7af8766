"""The voice band stage's definition, pinned without a GPU: the taps and their response, mi_vband_plan_host
(csrc/poststage_host.cpp) against the numpy model of vband_model.py as bytes -- the plane and the state blob --, what the filter does
to a tone under the voice band, the exported symbols and every refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vband_model as vm
from vband_model import HISTORY, PAIRS, TAPS, THREE_CLASSES, WAVE_BATCH, audio, vband_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VBAND_SYMBOLS = {"mi_vband_default_row", "mi_vband_create", "mi_vband_destroy", "mi_vband_set_rows", "mi_vband_process_device", "mi_vband_state_size",
                 "mi_vband_get_state", "mi_vband_set_state", "mi_vband_set_timing", "mi_vband_last_launch_ms", "mi_vband_taps", "mi_vband_plan_host"}
SENT = np.float32(-7.5)  # no output of the stage: it clamps to [-1, 1]
INVALID, NO_DEVICE = -1, -2
ROW_BYTES = 2040


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def classes_for(rows, kind):
    """one class, three classes, or one class per row"""
    if kind == "one":
        return [(100, 2500)] * rows
    if kind == "three":
        return [THREE_CLASSES[r % 3] for r in range(rows)]
    return [(50 + 10 * r, 2500 + 20 * r) for r in range(rows)]


# ---------------- taps ----------------

@pytest.mark.parametrize("hp,lp", PAIRS + [(0, 0), (50, 500), (4000, 7800), (4000, 0), (0, 7800), (1000, 2000)])
def test_taps_against_the_model(pkg, hp, lp):
    h, want = pkg.vband_taps(hp, lp), vm.taps(hp, lp)
    assert h.dtype == np.float32 and h.shape == (TAPS,)
    assert (np.abs(h.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all(), "more than one float32 step"
    assert h.tobytes() == h[::-1].tobytes(), "not symmetric bit for bit"


def test_both_settings_zero_give_a_unit_impulse(pkg):
    h = pkg.vband_taps(0, 0)
    want = np.zeros(TAPS, np.float32)
    want[255] = 1.0
    assert np.array_equal(h, want) and np.array_equal(vm.taps(0, 0), want)  # (h[0] = h[510] is -0.0: +0.0 times the window's -1.4e-17)
    wave = audio("noise", 1, 2)
    got, _ = pkg.vband_plan_host([1], wave, (0, 0))
    assert got[0, 255:].tobytes() == wave[0, :-255].tobytes() and not got[0, :255].any(), "a pure delay of 255 samples"


def test_default_row(pkg):
    assert pkg.vband_default_row() == (100, 2500) == vm.DEFAULT_ROW
    wave = audio("noise", 2, 1)
    assert pkg.vband_plan_host([1, 1], wave)[0].tobytes() == pkg.vband_plan_host([1, 1], wave, (100, 2500))[0].tobytes()


@pytest.mark.parametrize("hp,lp", PAIRS)
def test_response_of_the_returned_taps(pkg, hp, lp):
    """conditions on the design, not tolerances of the device: from a 2^17-point float64 FFT of the float32 taps, within +-0.01 dB from
    100 Hz inside each edge and below -70 dB from 100 Hz outside it.  Measured: +-0.0015 dB on all four; -72.86 dB for (100, 2500),
    whose lower stopband is DC alone, and -75.3 to -75.5 dB on the others."""
    for name, taps in (("float64 design", vm.design64(hp, lp)), ("returned float32 taps", pkg.vband_taps(hp, lp))):
        ripple, stop = vm.band_figures(taps, hp, lp)
        print(f"({hp}, {lp}) {name}: passband within {ripple:.5f} dB, stopband {stop:.2f} dB; sum |h| {np.abs(taps).sum():.4f}")
        assert ripple <= 0.01 and stop <= -70.0


# ---------------- the twin against the model ----------------

@pytest.mark.parametrize("kind", ["one", "three", "per_row"])
@pytest.mark.parametrize("nb", [1, 4])
@pytest.mark.parametrize("rows", [1, 5])
def test_twin_equals_model_on_every_builder(pkg, rows, nb, kind):
    """a call of nb batches and one more batch behind it, whose first 510 samples of history are the carried state"""
    cfg = classes_for(rows, kind)
    for name in vm.BUILDERS:
        wave = audio(name, rows, nb + 1)
        state = model_state = None
        for lo, hi in ((0, nb), (nb, nb + 1)):
            part = np.ascontiguousarray(wave[:, lo * WAVE_BATCH:hi * WAVE_BATCH])
            want, model_state = vband_model(part, cfg, model_state)
            got, state = pkg.vband_plan_host(np.ones(rows), part, cfg, state)
            assert got.tobytes() == want.tobytes(), f"{name}: plane, batches {lo} .. {hi}"
            assert state.tobytes() == model_state.tobytes(), f"{name}: state"
            assert state.view(np.float32).reshape(rows, HISTORY).tobytes() == part[:, -HISTORY:].tobytes()
            assert (np.abs(got) <= 1).all()


def test_builders_reach_what_they_are_for():
    """the square wave drives the clamp; silence and -0.0 give +0.0 throughout; the subnormal values give sums that are not zero; a
    lone sample shows in the block it is for, and in the last call only through tap 510 of output 0 where it is the oldest carried one"""
    h = vm.taps(100, 2500)
    sq = audio("square", 5, 2)
    raw = vm.fir(np.concatenate([np.zeros((5, HISTORY), np.float32), sq], axis=1), h)
    assert (np.abs(raw) > 1.0).any() and np.abs(vband_model(sq)[0]).max() == 1.0
    for name in ("silence", "minus_zero"):
        out = vband_model(audio(name, 2, 2), THREE_CLASSES[:2])[0]
        assert (out.view(np.uint32) == 0).all(), name
    assert vband_model(audio("subnormal", 2, 2))[0].any()
    first, _ = vband_model(audio("lone_first", 1, 2))
    assert first[0, 0] == np.float32(h[0] * np.float32(0.75)) and first[0, 0] != 0 and not first[0, TAPS:].any()
    last, _ = vband_model(audio("lone_last", 1, 2))
    assert not last[0, :WAVE_BATCH - 1].any() and last[0, WAVE_BATCH - 1] != 0 and last[0, WAVE_BATCH + HISTORY - 1] != 0 and not last[0, WAVE_BATCH + HISTORY:].any()
    for name, reach in (("lone_prev_batch_last", HISTORY), ("lone_carried_oldest", 1)):
        wave = audio(name, 1, 3)
        _, state = vband_model(wave[:, :2 * WAVE_BATCH])
        assert np.count_nonzero(state["x"]) == 1 and state["x"][0, 0 if reach == 1 else -1] == np.float32(0.75)
        out, _ = vband_model(wave[:, 2 * WAVE_BATCH:], state=state)
        assert out[0, 0] != 0 and out[0, reach - 1] != 0 and not out[0, reach:].any(), name


@pytest.mark.parametrize("cuts", [(4,), (1, 1, 1, 1), (1, 3)])
def test_call_cuts_give_identical_planes(pkg, cuts):
    """the same 4 batches as one call, as four calls and as 1 + 3, the state carried through the blob: a block's 510 samples of
    history come from the row's previous batch or from the carried state, and the bytes do not depend on which"""
    rows, nb = 5, 4
    cfg = classes_for(rows, "three")
    for name in ("voice_hum", "noise", "square", "lone_last"):
        wave = audio(name, rows, nb)
        whole, whole_state = vband_model(wave, cfg)
        state, done = None, 0
        for n in cuts:
            part = np.ascontiguousarray(wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH])
            got, state = pkg.vband_plan_host(np.ones(rows), part, cfg, state)
            assert got.tobytes() == whole[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH].tobytes(), f"{name}, cuts {cuts}, batch {done}"
            done += n
        assert state.tobytes() == whole_state.tobytes()


def test_a_disabled_row_padded_strides_and_sentinels(pkg):
    """rows 1 and 3 sit the second of three calls out: their output rows keep the sentinel, their carried samples keep their bytes,
    and the third call continues from the first call's tail.  The planes are laid out for a batch more than the call (input) and two
    more (output); nothing behind the call is read (it holds 0.5) or written."""
    rows, n = 5, 2
    cfg = classes_for(rows, "three")
    wave = audio("noise", rows, 3 * n)
    masks = [np.ones(rows, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(rows, np.uint8)]
    state, model_state = None, None
    for i, en in enumerate(masks):
        w = np.full((rows, (n + 1) * WAVE_BATCH), np.float32(0.5))
        w[:, :n * WAVE_BATCH] = wave[:, i * n * WAVE_BATCH:(i + 1) * n * WAVE_BATCH]
        out = np.full((rows, (n + 2) * WAVE_BATCH + 4), SENT)
        want, model_state = vband_model(w, cfg, model_state, en, nbatches=n, out=out)
        got, state = pkg.vband_plan_host(en, w, cfg, state, nbatches=n, out=out.copy())
        assert got.tobytes() == want.tobytes() and state.tobytes() == model_state.tobytes(), f"call {i}"
        assert (got[:, n * WAVE_BATCH:] == SENT).all() and (got[en == 0] == SENT).all() and (got[en == 1, :n * WAVE_BATCH] != SENT).all()
        tails = state.view(np.float32).reshape(rows, HISTORY)
        assert tails[0].tobytes() == w[0, n * WAVE_BATCH - HISTORY:n * WAVE_BATCH].tobytes()
        held = (1 if i == 1 else i + 1) * n * WAVE_BATCH
        assert tails[1].tobytes() == wave[1, held - HISTORY:held].tobytes()


# ---------------- what the filter is for ----------------

def test_a_tone_under_the_band_goes_and_the_voice_stays(pkg):
    """voice + 100 Hz through (300, 3400): after the first 510 samples the 100 Hz component of the output is at least 70 dB below the
    input's and the 1 kHz component within 0.01 dB of it, by float64 projections over whole periods.  The model alone and the twin.
    Measured: -92.1 dB and +0.00001 dB."""
    rows = 3
    wave = audio("voice_hum", rows, 4)
    model, _ = vband_model(wave, (300, 3400))
    twin, _ = pkg.vband_plan_host(np.ones(rows), wave, (300, 3400))
    assert twin.tobytes() == model.tobytes()
    for name, out in (("model", model), ("twin", twin)):
        for r in range(rows):
            tone = 20 * np.log10(vm.projection(out[r], vm.VOICE_TONE_HZ, HISTORY) / vm.projection(wave[r], vm.VOICE_TONE_HZ, HISTORY))
            voice = 20 * np.log10(vm.projection(out[r], vm.VOICE_PROBE_HZ, HISTORY) / vm.projection(wave[r], vm.VOICE_PROBE_HZ, HISTORY))
            print(f"{name}, row {r}: 100 Hz {tone:.2f} dB, 1 kHz {voice:+.6f} dB")
            assert tone <= -70.0 and abs(voice) <= 0.01


# ---------------- sizes, symbols, refusals ----------------

def test_sizes_and_symbols(pkg):
    assert C.sizeof(pkg.VbandRow) == 8 and pkg.VBAND_ROW_DTYPE.itemsize == 8 and pkg.VBAND_STATE_DTYPE.itemsize == ROW_BYTES
    assert (pkg.VBAND_TAPS, pkg.VBAND_HISTORY) == (TAPS, HISTORY) == (511, 510)
    assert pkg.lib().mi_vband_state_size(None) == 0
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    assert "MI_VBAND_TAPS = 511" in header and "MI_VBAND_HISTORY = 510" in header and "MI_VBAND_STATE_ROW_BYTES = 2040" in header
    assert "MI_GATE_OPEN_TRAIL" in header[header.index("voice band stage"):header.index("enum { MI_VBAND_TAPS")]
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_vband")}
    assert declared == VBAND_SYMBOLS and VBAND_SYMBOLS <= set(pkg.ABI_SYMBOLS)
    assert all(hasattr(pkg.lib(), s) for s in VBAND_SYMBOLS)


HP_TEXT = b"voice band stage: hp_hz must be 0 or 50 .. 4000"
LP_TEXT = b"voice band stage: lp_hz must be 0 or 500 .. 7800"
GAP_TEXT = b"voice band stage: lp_hz must be 0 or at least hp_hz + 200"
BAD_SETTINGS = [((1, 2500), HP_TEXT), ((49, 2500), HP_TEXT), ((4001, 0), HP_TEXT), ((0xFFFFFFFF, 0), HP_TEXT), ((0, 1), LP_TEXT), ((0, 499), LP_TEXT),
                ((0, 7801), LP_TEXT), ((100, 0xFFFFFFFF), LP_TEXT), ((301, 500), GAP_TEXT), ((2000, 2199), GAP_TEXT), ((4000, 4199), GAP_TEXT)]
GOOD_SETTINGS = [(0, 0), (50, 2500), (4000, 0), (4000, 4200), (0, 500), (0, 7800), (300, 500), (2000, 2200), (4000, 7800)]


def test_both_sides_of_every_settings_bound(pkg):
    L = pkg.lib()
    h = np.zeros(TAPS, np.float32)
    for (hp, lp) in GOOD_SETTINGS:
        assert vm.settings_ok(hp, lp) and L.mi_vband_taps(hp, lp, ptr(h)) == 0, (hp, lp)
    for (hp, lp), text in BAD_SETTINGS:
        assert not vm.settings_ok(hp, lp)
        assert L.mi_vband_taps(hp, lp, ptr(h)) == INVALID and L.mi_last_error() == text, (hp, lp)
        with pytest.raises(pkg.MiError) as e:
            pkg.vband_taps(hp, lp)
        assert e.value.code == pkg.MI_ERR_INVALID


def test_refusals(pkg):
    L = pkg.lib()
    null = b"NULL argument"

    def refused(rc, code=INVALID, text=None):
        assert rc == code
        if text is not None:
            assert L.mi_last_error() == text

    def rows_of(*pairs):
        return np.array(pairs, np.uint32).view(pkg.VBAND_ROW_DTYPE).reshape(-1)

    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(4096, np.uint8)
    good = rows_of(*[(100, 2500)] * 4)
    refused(L.mi_vband_create(ptr(good), None, 4, 1, 0, C.byref(out)), text=null)
    refused(L.mi_vband_create(ptr(good), ptr(en), 4, 1, 0, None), text=null)
    geometry = b"voice band stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
    for rows, max_batches in ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, 1 << 12), ((1 << 20) - 1, 17)):
        refused(L.mi_vband_create(None, ptr(en), rows, max_batches, 0, C.byref(out)), text=geometry)
    for bad, text in BAD_SETTINGS:  # (the arguments alone decide: before a device is looked for; a bad row anywhere, a disabled one too)
        for at in (0, 3):
            cfg = rows_of(*[(100, 2500) if r != at else bad for r in range(4)])
            refused(L.mi_vband_create(ptr(cfg), ptr(np.array([1, 1, 1, 0], np.uint8)), 4, 1, 0, C.byref(out)), text=text)
    assert not out.value
    if pkg.device_count() < 1:
        for cfg in (None, ptr(good)):
            refused(L.mi_vband_create(cfg, ptr(en), 4, 1, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the voice band stage runs on the GPU only")
        assert not out.value
        with pytest.raises(pkg.MiError) as e:
            pkg.Vband(np.ones(3), max_batches=2)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE
    # a NULL handle, before anything else
    refused(L.mi_vband_set_rows(None, ptr(good), ptr(en)), text=null)
    refused(L.mi_vband_process_device(None, ptr(some), 0, 1, ptr(some), 0, None), text=null)
    refused(L.mi_vband_set_timing(None, 1), text=null)
    refused(L.mi_vband_last_launch_ms(None, ptr(some)), text=null)
    refused(L.mi_vband_get_state(None, ptr(some), ROW_BYTES), text=b"voice band stage state: NULL argument or wrong length")
    refused(L.mi_vband_set_state(None, ptr(some), ROW_BYTES), text=b"voice band stage state: NULL argument or wrong length")
    assert L.mi_vband_state_size(None) == 0
    L.mi_vband_destroy(None)
    refused(L.mi_vband_taps(100, 2500, None), text=null)
    # the twin
    rows, nb = 2, 2
    n = nb * WAVE_BATCH
    wave, plane, state = np.zeros((rows, n), np.float32), np.zeros((rows, n), np.float32), np.zeros(rows * ROW_BYTES, np.uint8)
    cfg2 = rows_of((100, 2500), (300, 3400))

    def plan(**over):
        a = dict(cfg=ptr(cfg2), en=ptr(en), rows=rows, nb=nb, wave=ptr(wave), row_stride=n, state=ptr(state), out=ptr(plane), out_stride=n)
        a.update(over)
        return L.mi_vband_plan_host(*a.values())

    assert plan() == 0 and plan(cfg=None) == 0
    for name in ("en", "wave", "state", "out"):
        refused(plan(**{name: None}), text=null)
    for bad, text in BAD_SETTINGS:
        refused(plan(cfg=ptr(rows_of((100, 2500), bad))), text=text)
    for over in (dict(rows=0), dict(rows=-1), dict(nb=0), dict(nb=-1)):
        refused(plan(**over), text=b"vband plan needs rows >= 1 and nbatches >= 1")
    for over in (dict(row_stride=n - 1), dict(out_stride=n - 1)):
        refused(plan(**over), text=b"a row stride is shorter than the call")
    # overlap of input and output: the same plane, a shifted one, the output's last float on the input's first and the reverse
    overlap = b"the output overlaps the audio buffer"
    big = np.zeros(4 * rows * n, np.float32)
    at = lambda i: C.c_void_p(big.ctypes.data + 4 * i)
    span = rows * n
    for w_at, o_at in ((0, 0), (0, 1), (1, 0), (0, span - 1), (span - 1, 0), (100, n)):
        refused(plan(wave=at(w_at), out=at(o_at)), text=overlap)
    assert plan(wave=at(0), out=at(span)) == 0 and plan(wave=at(span), out=at(0)) == 0
    # (rows interleaved in one allocation overlap as ranges: refused, though no float is shared)
    refused(plan(wave=at(0), row_stride=2 * n, out=at(n), out_stride=2 * n), text=overlap)
