"""Every refusal of the packet stage that needs no GPU: code and words, both sides of every settings bound, the host twin's argument
checks and impossible state blobs, sizes and symbols.  (The refusals of mi_ax25_process_device are in test_gpu_ax25.py.)"""
import ctypes as C

import numpy as np
import pytest

import ax25_model as m
from ax25_model import FRAME_REC, STATE, WAVE_BATCH, fresh_state


def settings_rc(pkg, gain=(0.0, 0.0, 0.0), strict=0):
    c, out = pkg.Ax25Cfg(), pkg.Ax25Cfg()
    for g in range(3):
        c.gain[g] = gain[g]
    c.strict = strict
    rc = pkg.lib().mi_ax25_settings(C.byref(c), C.byref(out))
    return rc, pkg.lib().mi_last_error().decode(), out


@pytest.mark.parametrize("g", [0, 1, 2])
def test_both_sides_of_the_gain_bounds(pkg, g):
    default = np.float32(m.DEFAULT_GAIN[g])
    for v in (0.0, -0.0, 1e-45, 1e-30, 1.0, 3.0e38):
        gain = [0.0, 0.0, 0.0]
        gain[g] = v
        rc, _, out = settings_rc(pkg, gain)
        assert rc == pkg.MI_OK and out.gain[g] == (default if v == 0 else np.float32(v)), (g, v)
    for v in (-1e-45, -1.0, float("inf"), float("-inf"), float("nan")):
        gain = [0.0, 0.0, 0.0]
        gain[g] = v
        rc, msg, _ = settings_rc(pkg, gain)
        assert rc == pkg.MI_ERR_INVALID and "every gain must be finite and positive" in msg and msg.startswith("packet stage: "), (g, v, msg)


def test_both_sides_of_the_strict_bound(pkg):
    for v, want in ((0, 1), (1, 1), (pkg.AX25_STRICT_OFF, pkg.AX25_STRICT_OFF)):
        rc, _, out = settings_rc(pkg, strict=v)
        assert rc == pkg.MI_OK and out.strict == want
    for v in (2, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFF):
        rc, msg, _ = settings_rc(pkg, strict=v)
        assert rc == pkg.MI_ERR_INVALID and "strict must be 0, 1 or MI_AX25_STRICT_OFF" in msg


def test_null_arguments_sizes_and_symbols(pkg):
    L = pkg.lib()
    for s in pkg.ABI_SYMBOLS:
        if s.startswith("mi_ax25_"):
            assert hasattr(L, s), s
    assert sum(s.startswith("mi_ax25_") for s in pkg.ABI_SYMBOLS) == 15
    assert STATE.itemsize == pkg.AX25_STATE_DTYPE.itemsize == 10544 and FRAME_REC.itemsize == pkg.AX25_FRAME_DTYPE.itemsize == 352 and C.sizeof(pkg.Ax25Cfg) == 16
    assert L.mi_ax25_settings(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_ax25_templates(None) == pkg.MI_ERR_INVALID
    f = np.zeros(1, FRAME_REC)
    buf = C.create_string_buffer(pkg.AX25_TEXT_BYTES)
    assert L.mi_ax25_frame_text(None, buf, 384) == pkg.MI_ERR_INVALID and L.mi_ax25_frame_text(f.ctypes.data, None, 384) == pkg.MI_ERR_INVALID
    good = m.ui_frame(**m.SHORT)
    f["bytes"][0][:len(good)] = good
    for nbytes, rc, words in ((16, pkg.MI_ERR_INVALID, b"nbytes must be within 17 .. 330"), (331, pkg.MI_ERR_INVALID, b"nbytes must be within 17 .. 330"),
                              (len(good), pkg.MI_OK, b"")):
        f["nbytes"] = nbytes
        assert L.mi_ax25_frame_text(f.ctypes.data, buf, 384) == rc and words in L.mi_last_error(), nbytes
    assert L.mi_ax25_frame_text(f.ctypes.data, buf, 10) == pkg.MI_ERR_INVALID and b"the text buffer is shorter than the line" in L.mi_last_error()
    assert L.mi_ax25_state_size(None) == 0
    assert L.mi_ax25_set_rows(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_ax25_set_timing(None, 1) == pkg.MI_ERR_INVALID and L.mi_ax25_last_launch_ms(None, None) == pkg.MI_ERR_INVALID
    assert L.mi_ax25_get_state(None, None, 0) == pkg.MI_ERR_INVALID and b"packet stage state" in L.mi_last_error()
    assert L.mi_ax25_set_state(None, None, 0) == pkg.MI_ERR_INVALID and L.mi_ax25_download(None, None, None, None, None) == pkg.MI_ERR_INVALID
    assert L.mi_ax25_process_device(None, None, 0, 1, None, None, None, None, None) == pkg.MI_ERR_INVALID
    L.mi_ax25_destroy(None)


def test_create_refusals_that_come_before_the_device(pkg):
    L = pkg.lib()
    en = np.ones(4, np.uint8)
    h = C.c_void_p()
    assert L.mi_ax25_create(None, None, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_ax25_create(None, en.ctypes.data, 4, 1, 0, 0, None) == pkg.MI_ERR_INVALID
    bad = pkg.Ax25Cfg(strict=9)
    assert L.mi_ax25_create(C.byref(bad), en.ctypes.data, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"strict" in L.mi_last_error()
    for rows, nb in ((0, 1), (4, 0), (1 << 20, 1), (1 << 12, 1 << 12)):
        assert L.mi_ax25_create(None, en.ctypes.data, rows, nb, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID, (rows, nb)
        assert b"packet stage needs 1 <= rows < 2^20" in L.mi_last_error()
    if pkg.device_count() == 0:
        assert L.mi_ax25_create(None, en.ctypes.data, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_NO_DEVICE and b"the packet stage runs on the GPU only" in L.mi_last_error()


def test_the_host_twin_s_argument_checks_and_the_impossible_blobs(pkg):
    L = pkg.lib()
    rows, nb = 2, 1
    en, plane, state = np.ones(rows, np.uint8), np.zeros((rows, nb * WAVE_BATCH), np.float32), fresh_state(rows)
    frames, first, count = np.zeros(4, FRAME_REC), np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)

    def call(cfg=None, en=en, rows=rows, nb=nb, plane=plane, stride=nb * WAVE_BATCH, state=state, frames=frames, cap=4, first=first, count=count):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        state = None if state is None else state.copy()  # (the twin updates the blob it is given)
        return L.mi_ax25_plan_host(None if cfg is None else C.byref(cfg), p(en), rows, nb, p(plane), stride, p(state), None, p(frames), cap, p(first), p(count))

    assert call() == pkg.MI_OK
    for kw in (dict(en=None), dict(plane=None), dict(state=None), dict(frames=None), dict(first=None), dict(count=None)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error(), kw
    for kw in (dict(rows=0), dict(nb=0), dict(cap=0)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"packet plan needs rows >= 1, nbatches >= 1 and max_frames >= 1" in L.mi_last_error(), kw
    assert call(stride=WAVE_BATCH - 1) == pkg.MI_ERR_INVALID and b"a row stride is shorter than the call" in L.mi_last_error()
    assert call(cfg=pkg.Ax25Cfg(strict=2)) == pkg.MI_ERR_INVALID and b"strict" in L.mi_last_error()
    for what, blob, words in m.bad_blobs():
        rc = call(rows=1, en=en[:1], state=blob)
        if words is None:
            assert rc == pkg.MI_OK, (what, L.mi_last_error())
        else:
            assert rc == pkg.MI_ERR_INVALID and b"packet plan: malformed state blob: " in L.mi_last_error() and words.encode() in L.mi_last_error(), (what, L.mi_last_error())
