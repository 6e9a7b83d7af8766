"""Every refusal of the ACARS stage that needs no GPU: code and words, both sides of every settings bound, the host twin's argument
checks and impossible state blobs.  (The refusals of mi_acars_process_device are in test_gpu_acars.py.)"""
import ctypes as C

import numpy as np
import pytest

from acars_model import FRAME_REC, STATE, WAVE_BATCH, fresh_state


def settings_rc(pkg, **fields):
    c, out = pkg.AcarsCfg(), pkg.AcarsCfg()
    for k, v in fields.items():
        setattr(c, k, v)
    rc = pkg.lib().mi_acars_settings(C.byref(c), C.byref(out))
    return rc, pkg.lib().mi_last_error().decode(), out


@pytest.mark.parametrize("field,good,bad,words", [
    ("sync_errors", [0, 1, 4, 0x80000000], [5, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFF], "sync_errors must be within 1 .. 4 or MI_ACARS_SYNC_EXACT"),
    ("keep_bad", [0, 1], [2, 0xFFFFFFFF], "keep_bad must be 0 or 1"),
    ("hold_timing", [0, 1], [2, 0xFFFFFFFF], "hold_timing must be 0 or 1"),
    ("min_quality", [0.0, -0.0, 1e-30, 3.0e38], [-1e-30, float("inf"), float("nan")], "min_quality must be finite and not negative"),
])
def test_both_sides_of_every_settings_bound(pkg, field, good, bad, words):
    for v in good:
        rc, _, out = settings_rc(pkg, **{field: v})
        assert rc == pkg.MI_OK, (field, v)
        assert getattr(out, field) == (2 if field == "sync_errors" and v == 0 else np.float32(v) if field == "min_quality" else v)
    for v in bad:
        rc, msg, _ = settings_rc(pkg, **{field: v})
        assert rc == pkg.MI_ERR_INVALID and words in msg and msg.startswith("ACARS stage: "), (field, v, msg)


def test_null_arguments_and_the_helpers(pkg):
    L = pkg.lib()
    assert L.mi_acars_settings(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    out = pkg.AcarsCfg()
    assert L.mi_acars_settings(None, C.byref(out)) == pkg.MI_OK and out.sync_errors == 2
    h = np.zeros(20, np.float32)
    assert L.mi_acars_templates(None, h.ctypes.data) == pkg.MI_ERR_INVALID and L.mi_acars_templates(h.ctypes.data, None) == pkg.MI_ERR_INVALID
    text = pkg.AcarsText()
    f = np.zeros(1, FRAME_REC)
    assert L.mi_acars_frame_text(None, C.byref(text)) == pkg.MI_ERR_INVALID and L.mi_acars_frame_text(f.ctypes.data, None) == pkg.MI_ERR_INVALID
    for nbytes, rc in ((12, pkg.MI_ERR_INVALID), (13, pkg.MI_OK), (240, pkg.MI_OK), (241, pkg.MI_ERR_INVALID)):
        f["nbytes"] = nbytes
        assert L.mi_acars_frame_text(f.ctypes.data, C.byref(text)) == rc, nbytes
        if rc:
            assert b"nbytes must be within 13 .. 240" in L.mi_last_error()
    assert L.mi_acars_state_size(None) == 0
    assert L.mi_acars_set_rows(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_acars_set_timing(None, 1) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_acars_last_launch_ms(None, None) == pkg.MI_ERR_INVALID
    assert L.mi_acars_get_state(None, None, 0) == pkg.MI_ERR_INVALID and b"ACARS stage state" in L.mi_last_error()
    assert L.mi_acars_set_state(None, None, 0) == pkg.MI_ERR_INVALID and L.mi_acars_download(None, None, None, None, None) == pkg.MI_ERR_INVALID
    assert L.mi_acars_process_device(None, None, 0, 1, None, None, None, None, None, None) == pkg.MI_ERR_INVALID
    L.mi_acars_destroy(None)


def test_create_refusals_that_come_before_the_device(pkg):
    L = pkg.lib()
    en = np.ones(4, np.uint8)
    h = C.c_void_p()
    assert L.mi_acars_create(None, None, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_acars_create(None, en.ctypes.data, 4, 1, 0, 0, None) == pkg.MI_ERR_INVALID
    bad = pkg.AcarsCfg(sync_errors=9)
    assert L.mi_acars_create(C.byref(bad), en.ctypes.data, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"sync_errors" in L.mi_last_error()
    for rows, nb in ((0, 1), (4, 0), (1 << 20, 1), (1 << 12, 1 << 12)):
        assert L.mi_acars_create(None, en.ctypes.data, rows, nb, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID, (rows, nb)
        assert b"ACARS stage needs 1 <= rows < 2^20" in L.mi_last_error()


def test_the_host_twin_s_argument_checks(pkg):
    L = pkg.lib()
    rows, nb = 2, 1
    en, plane, state = np.ones(rows, np.uint8), np.zeros((rows, nb * WAVE_BATCH), np.float32), fresh_state(rows)
    frames, first, count = np.zeros(4, FRAME_REC), np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)

    def call(cfg=None, en=en, rows=rows, nb=nb, plane=plane, stride=nb * WAVE_BATCH, state=state, frames=frames, cap=4, first=first, count=count):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        state = None if state is None else state.copy()  # (the twin updates the blob it is given)
        return L.mi_acars_plan_host(None if cfg is None else C.byref(cfg), p(en), rows, nb, p(plane), stride, p(state), None, None, p(frames), cap, p(first), p(count))

    assert call() == pkg.MI_OK
    for kw in (dict(en=None), dict(plane=None), dict(state=None), dict(frames=None), dict(first=None), dict(count=None)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error(), kw
    for kw in (dict(rows=0), dict(nb=0), dict(cap=0)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"ACARS plan needs rows >= 1, nbatches >= 1 and max_frames >= 1" in L.mi_last_error(), kw
    assert call(stride=WAVE_BATCH - 1) == pkg.MI_ERR_INVALID and b"a row stride is shorter than the call" in L.mi_last_error()
    assert call(cfg=pkg.AcarsCfg(keep_bad=2)) == pkg.MI_ERR_INVALID and b"keep_bad" in L.mi_last_error()
    for field, value, words in (("zero", 1, b"the zero field is not 0"), ("phase", 2, b"an unknown walker phase"), ("crc", 1, b"an idle row with a walker field set")):
        bad = fresh_state(rows)
        bad[1][field] = value
        assert call(state=bad) == pkg.MI_ERR_INVALID and b"ACARS plan: malformed state blob: " in L.mi_last_error() and words in L.mi_last_error(), field
    bad = fresh_state(rows)
    bad["hist"][0][19] = 1 << 38
    assert call(state=bad) == pkg.MI_ERR_INVALID and b"more than 38 change bits" in L.mi_last_error()
    bad = fresh_state(rows)
    bad["bytes"][1][0] = 1
    assert call(state=bad) == pkg.MI_ERR_INVALID and b"a byte set behind the ones taken" in L.mi_last_error()
    # inside a frame: each impossible field on its own
    ok = fresh_state(1)
    ok["phase"], ok["nbytes"], ok["bytes"][0][0], ok["crc"], ok["parity_errors"] = 1, 1, 0x32, pkg.acars_crc(b"\x32"), 0
    assert call(rows=1, en=en[:1], state=ok) == pkg.MI_OK, L.mi_last_error()
    for field, value in (("u", 20), ("tau_sync", 20), ("prev", 2), ("nbits", 8), ("cur", 1), ("tail", 3), ("tail", 1), ("mismatches", 5), ("start_third", 6000),
                         ("end", 3), ("nbytes", 240), ("crc", 0), ("parity_errors", 1)):
        bad = ok.copy()
        bad[0][field] = value
        assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"an impossible walker state" in L.mi_last_error(), field
    assert STATE.itemsize == 496
