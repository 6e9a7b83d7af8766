"""Every refusal of the ELT stage that needs no GPU: code and words, both sides of every settings bound, the host twin's argument
checks, impossible state blobs, sizes and symbols.  (The refusals of mi_elt_process_device are in test_gpu_elt.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from elt_model import DEFAULTS, EVENT_REC, FRAME_REC, STATE, WAVE_BATCH, fresh_state, refused_states, state_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELT_SYMBOLS = {"mi_elt_" + s for s in ("create", "destroy", "set_rows", "process_device", "download", "state_size", "get_state", "set_state", "set_timing",
                                        "last_launch_ms", "plan_host", "settings", "window", "coeffs", "event_text")}


def settings_rc(pkg, **fields):
    c, out = pkg.EltCfg(), pkg.EltCfg()
    for k, v in fields.items():
        setattr(c, k, v)
    rc = pkg.lib().mi_elt_settings(C.byref(c), C.byref(out), None)
    return rc, pkg.lib().mi_last_error().decode(), out


BIG = 0xFFFFFFFF


@pytest.mark.parametrize("field,good,bad,words,extra", [
    ("min_energy", [0.0, 1e-12, 1e6], [0.9e-12, 1.1e6, -1.0, float("inf"), float("nan")], "min_energy must be finite and within 1e-12 .. 1e6", {}),
    ("min_tonality", [0.0, 0.01, 1.5], [0.009, 1.51, -0.5, float("inf"), float("nan")], "min_tonality must be within 0.01 .. 1.5", {}),
    ("band_lo", [0, 2, 26, 33], [1, 34, BIG], "band_lo must be within 2 .. 33 bins", {}),
    ("band_hi", [0, 4, 33], [3, 34, BIG], "band_hi must be within band_lo .. 33 bins", {}),
    ("min_span", [0, 1, 31], [32, BIG], "min_span must be within 1 .. 31 bins", {}),
    ("min_len", [0, 2, 4096], [1, 4097, BIG], "min_len must be within 2 .. 4096 frames", {}),
    ("max_len", [0, 40, 65536], [39, 65537, BIG], "max_len must be within min_len .. 65536 frames", {}),
    ("max_step", [0, 1, 31], [32, BIG], "max_step must be within 1 .. 31 bins", {}),
    ("max_drop", [0, 1, 64], [65, BIG], "max_drop must be within 1 .. 64 frames", {}),
    ("max_gap", [0, 1, 1024], [1025, BIG], "max_gap must be within 1 .. 1024 frames", {}),
    ("min_sweeps", [0, 1, 1024], [1025, BIG], "min_sweeps must be within 1 .. 1024 sweeps", {}),
    ("zero", [0], [1, BIG], "the settings' zero field must be 0", {}),
])
def test_both_sides_of_every_settings_bound(pkg, field, good, bad, words, extra):
    for v in good:
        rc, msg, out = settings_rc(pkg, **{field: v, **extra})
        assert rc == pkg.MI_OK, (field, v, msg)
        if field != "zero":
            assert getattr(out, field) == (v if isinstance(v, int) and v else np.float32(v if v else DEFAULTS[field])), (field, v)
    for v in bad:
        rc, msg, _ = settings_rc(pkg, **{field: v, **extra})
        assert rc == pkg.MI_ERR_INVALID and words in msg and msg.startswith("ELT stage: "), (field, v, msg)


def test_defaults_that_follow_another_setting(pkg):
    assert settings_rc(pkg, band_lo=30)[2].band_hi == 30 and settings_rc(pkg, min_len=200)[2].max_len == 200
    assert settings_rc(pkg, min_len=121, max_len=120)[0] == pkg.MI_ERR_INVALID and settings_rc(pkg, band_lo=10, band_hi=9)[0] == pkg.MI_ERR_INVALID


def test_sizes_and_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    assert re.search(r"MI_ELT_FRAME = 256, MI_ELT_HOP = 80, MI_ELT_HISTORY = 178, MI_ELT_FRAMES = 25, MI_ELT_BINS = 32, MI_ELT_BIN0 = 2, MI_ELT_STATE_ROW_BYTES = 776",
                     header)
    assert "written from memory of the ELT specifications" in header and "no off-air beacon has been through the stage" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", code) if s.startswith("mi_elt_")}
    assert declared == ELT_SYMBOLS and ELT_SYMBOLS <= set(pkg.ABI_SYMBOLS)
    assert not [s for s in sorted(declared) if not hasattr(pkg.lib(), s)]
    assert C.sizeof(pkg.EltCfg) == 48 and pkg.ELT_FRAME_DTYPE.itemsize == 16 == FRAME_REC.itemsize and pkg.ELT_EVENT_DTYPE.itemsize == 32 == EVENT_REC.itemsize
    assert pkg.ELT_STATE_DTYPE.itemsize == 776 == STATE.itemsize
    for a, b in ((pkg.ELT_FRAME_DTYPE, FRAME_REC), (pkg.ELT_EVENT_DTYPE, EVENT_REC), (pkg.ELT_STATE_DTYPE, STATE)):
        assert [(n, a.fields[n][1]) for n in a.names] == [(n, b.fields[n][1]) for n in b.names]


def test_null_arguments_and_the_helpers(pkg):
    L = pkg.lib()
    assert L.mi_elt_settings(None, None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_elt_window(None) == pkg.MI_ERR_INVALID and L.mi_elt_coeffs(None) == pkg.MI_ERR_INVALID
    e, out = np.zeros(1, EVENT_REC), np.zeros(96, np.uint8)
    assert L.mi_elt_event_text(None, out.ctypes.data) == pkg.MI_ERR_INVALID and L.mi_elt_event_text(e.ctypes.data, None) == pkg.MI_ERR_INVALID
    assert L.mi_elt_event_text(e.ctypes.data, out.ctypes.data) == pkg.MI_ERR_INVALID and b"not an event record the stage writes" in L.mi_last_error()
    assert L.mi_elt_state_size(None) == 0
    assert L.mi_elt_set_rows(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_elt_set_timing(None, 1) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_elt_last_launch_ms(None, None) == pkg.MI_ERR_INVALID
    assert L.mi_elt_get_state(None, None, 0) == pkg.MI_ERR_INVALID and b"ELT stage state" in L.mi_last_error()
    assert L.mi_elt_set_state(None, None, 0) == pkg.MI_ERR_INVALID and L.mi_elt_download(None, None, None, None, None, None) == pkg.MI_ERR_INVALID
    assert L.mi_elt_process_device(None, None, 0, 1, None, None, None, None, None) == pkg.MI_ERR_INVALID
    L.mi_elt_destroy(None)


def test_create_refusals_that_come_before_the_device(pkg):
    L = pkg.lib()
    en = np.ones(4, np.uint8)
    h = C.c_void_p()
    assert L.mi_elt_create(None, None, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_elt_create(None, en.ctypes.data, 4, 1, 0, 0, None) == pkg.MI_ERR_INVALID
    bad = pkg.EltCfg(max_gap=2000)
    assert L.mi_elt_create(C.byref(bad), en.ctypes.data, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"max_gap" in L.mi_last_error()
    for rows, nb in ((0, 1), (4, 0), (1 << 20, 1), (1 << 12, 1 << 12)):
        assert L.mi_elt_create(None, en.ctypes.data, rows, nb, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID, (rows, nb)
        assert b"ELT stage needs 1 <= rows < 2^20" in L.mi_last_error()
    if pkg.device_count() == 0:
        assert L.mi_elt_create(None, en.ctypes.data, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_NO_DEVICE and b"the ELT stage runs on the GPU only" in L.mi_last_error()


def test_the_host_twin_s_argument_checks_and_impossible_states(pkg):
    L = pkg.lib()
    rows, nb = 2, 1
    en, plane, state = np.ones(rows, np.uint8), np.zeros((rows, nb * WAVE_BATCH), np.float32), fresh_state(rows)
    events, first, count = np.zeros(8, EVENT_REC), np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)

    def call(cfg=None, en=en, rows=rows, nb=nb, plane=plane, stride=nb * WAVE_BATCH, state=state, events=events, cap=8, first=first, count=count):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        state = None if state is None else state.copy()  # (the twin updates the blob it is given)
        return L.mi_elt_plan_host(None if cfg is None else C.byref(cfg), p(en), rows, nb, p(plane), stride, p(state), None, p(events), cap, p(first), p(count))

    assert call() == pkg.MI_OK
    for kw in (dict(en=None), dict(plane=None), dict(state=None), dict(events=None), dict(first=None), dict(count=None)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error(), kw
    for kw in (dict(rows=0), dict(nb=0), dict(cap=0)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"ELT plan needs rows >= 1, nbatches >= 1 and max_events >= 1" in L.mi_last_error(), kw
    assert call(stride=WAVE_BATCH - 1) == pkg.MI_ERR_INVALID and b"a row stride is shorter than the call" in L.mi_last_error()
    assert call(cfg=pkg.EltCfg(max_drop=65)) == pkg.MI_ERR_INVALID and b"max_drop" in L.mi_last_error()
    # (the check comes before anything is read: no plane of that size exists)
    tiny = pkg.EltCfg(min_sweeps=1, min_len=2)
    assert call(cfg=tiny, rows=1 << 10, nb=0x7FFFFFFF, stride=0x7FFFFFFF * WAVE_BATCH) == pkg.MI_ERR_INVALID and b"do not fit the 32-bit count" in L.mi_last_error()
    good, bad = refused_states()
    for name, fields in good:
        assert call(state=state_of(rows, 1, fields)) == pkg.MI_OK, (name, L.mi_last_error())
    for name, fields in bad:
        assert call(state=state_of(rows, 1, fields)) == pkg.MI_ERR_INVALID and b"ELT plan: malformed state blob: " in L.mi_last_error(), name
