"""Every refusal of the pager stage that needs no GPU: code and words, both sides of every settings bound, the host twin's argument
checks and impossible state blobs.  (The refusals of mi_pocsag_process_device are in test_gpu_pocsag.py.)"""
import ctypes as C

import numpy as np
import pytest

from pocsag_model import MESSAGE, STATE, WAVE_BATCH, fresh_state


def settings_rc(pkg, **fields):
    c, out = pkg.PocsagCfg(), pkg.PocsagCfg()
    for k, v in fields.items():
        setattr(c, k, v)
    rc = pkg.lib().mi_pocsag_settings(C.byref(c), C.byref(out))
    return rc, pkg.lib().mi_last_error().decode(), out


@pytest.mark.parametrize("field,good,bad,default,words", [
    ("baud", [0, 512, 1200, 2400], [1, 511, 513, 1199, 2401, 4800, 0xFFFFFFFF], 1200, "baud must be 512, 1200 or 2400"),
    ("sync_errors", [0, 1, 4, 0x80000000], [5, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFF], 2, "sync_errors must be within 1 .. 4 or MI_POCSAG_SYNC_EXACT"),
    ("preamble_errors", [0, 1, 8, 0x80000000, 0x80000001], [9, 0x7FFFFFFF, 0x80000002, 0xFFFFFFFF], 4, "preamble_errors must be within 1 .. 8"),
    ("correct", [0, 1, 2, 0x80000000], [3, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFF], 1, "correct must be 1, 2 or MI_POCSAG_CORRECT_NONE"),
    ("hold_timing", [0, 1], [2, 0xFFFFFFFF], 0, "hold_timing must be 0 or 1"),
])
def test_both_sides_of_every_settings_bound(pkg, field, good, bad, default, words):
    for v in good:
        rc, _, out = settings_rc(pkg, **{field: v})
        assert rc == pkg.MI_OK, (field, v)
        assert getattr(out, field) == (default if v == 0 else v)
    for v in bad:
        rc, msg, _ = settings_rc(pkg, **{field: v})
        assert rc == pkg.MI_ERR_INVALID and words in msg and msg.startswith("pager stage: "), (field, v, msg)


def test_null_arguments_and_the_helpers(pkg):
    L = pkg.lib()
    assert L.mi_pocsag_settings(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    out = pkg.PocsagCfg()
    assert L.mi_pocsag_settings(None, C.byref(out)) == pkg.MI_OK and (out.baud, out.sync_errors, out.preamble_errors, out.correct) == (1200, 2, 4, 1)
    assert L.mi_pocsag_geometry(1200, None, None, None) == pkg.MI_OK and L.mi_pocsag_geometry(300, None, None, None) == pkg.MI_ERR_INVALID
    assert [pkg.pocsag_geometry(b) for b in (512, 0, 1200, 2400)] == [(15, 64, 2), (10, 150, 5), (10, 150, 5), (10, 300, 10)]
    assert L.mi_pocsag_decode(0, 3, None, None) == pkg.MI_ERR_INVALID and L.mi_pocsag_decode(0, 1, None, None) == 1
    text = C.create_string_buffer(pkg.POCSAG_TEXT_BYTES)
    msg = np.zeros(1, MESSAGE)
    assert L.mi_pocsag_message_text(None, 0, text, 8) == pkg.MI_ERR_INVALID and L.mi_pocsag_message_text(msg.ctypes.data, 0, None, 8) == pkg.MI_ERR_INVALID
    assert L.mi_pocsag_message_text(msg.ctypes.data, 3, text, 8) == pkg.MI_ERR_INVALID and b"text mode" in L.mi_last_error()
    msg["nwords"] = 81
    assert L.mi_pocsag_message_text(msg.ctypes.data, 0, text, 8) == pkg.MI_ERR_INVALID and b"nwords must be within 0 .. 80" in L.mi_last_error()
    msg["nwords"] = 80
    assert L.mi_pocsag_message_text(msg.ctypes.data, 1, text, 400) == pkg.MI_ERR_INVALID and b"does not fit" in L.mi_last_error()
    assert L.mi_pocsag_message_text(msg.ctypes.data, 1, text, 401) == pkg.MI_OK and text.value == b"0" * 400
    assert L.mi_pocsag_state_size(None) == 0
    assert L.mi_pocsag_set_rows(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_pocsag_set_timing(None, 1) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_pocsag_last_launch_ms(None, None) == pkg.MI_ERR_INVALID
    assert L.mi_pocsag_get_state(None, None, 0) == pkg.MI_ERR_INVALID and b"pager stage state" in L.mi_last_error()
    assert L.mi_pocsag_set_state(None, None, 0) == pkg.MI_ERR_INVALID and L.mi_pocsag_download(None, None, None, None, None) == pkg.MI_ERR_INVALID
    assert L.mi_pocsag_process_device(None, None, 0, 1, None, None, None, None, None, None) == pkg.MI_ERR_INVALID
    L.mi_pocsag_destroy(None)


def test_create_refusals_that_come_before_the_device(pkg):
    L = pkg.lib()
    en = np.ones(4, np.uint8)
    h = C.c_void_p()
    assert L.mi_pocsag_create(None, None, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_pocsag_create(None, en.ctypes.data, 4, 1, 0, 0, None) == pkg.MI_ERR_INVALID
    for bad, words in ((pkg.PocsagCfg(baud=600), b"baud"), (pkg.PocsagCfg(sync_errors=9), b"sync_errors"), (pkg.PocsagCfg(preamble_errors=9), b"preamble_errors"),
                       (pkg.PocsagCfg(correct=3), b"correct"), (pkg.PocsagCfg(hold_timing=2), b"hold_timing")):
        assert L.mi_pocsag_create(C.byref(bad), en.ctypes.data, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and words in L.mi_last_error()
    for rows, nb in ((0, 1), (4, 0), (1 << 20, 1), (1 << 12, 1 << 12)):
        assert L.mi_pocsag_create(None, en.ctypes.data, rows, nb, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID, (rows, nb)
        assert b"pager stage needs 1 <= rows < 2^20" in L.mi_last_error()


def test_the_host_twin_s_argument_checks_and_impossible_blobs(pkg):
    L = pkg.lib()
    rows, nb = 2, 1
    en, plane, state = np.ones(rows, np.uint8), np.zeros((rows, nb * WAVE_BATCH), np.float32), fresh_state(rows)
    msgs, first, count = np.zeros(12, MESSAGE), np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)

    def call(cfg=None, en=en, rows=rows, nb=nb, plane=plane, stride=nb * WAVE_BATCH, state=state, msgs=msgs, cap=12, first=first, count=count):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        state = None if state is None else state.copy()  # (the twin updates the blob it is given)
        return L.mi_pocsag_plan_host(None if cfg is None else C.byref(cfg), p(en), rows, nb, p(plane), stride, p(state), None, None, p(msgs), cap, p(first), p(count))

    assert call() == pkg.MI_OK
    for kw in (dict(en=None), dict(plane=None), dict(state=None), dict(msgs=None), dict(first=None), dict(count=None)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error(), kw
    for kw in (dict(rows=0), dict(nb=0), dict(cap=0)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"pager plan needs rows >= 1, nbatches >= 1 and max_messages >= 1" in L.mi_last_error(), kw
    assert call(stride=WAVE_BATCH - 1) == pkg.MI_ERR_INVALID and b"a row stride is shorter than the call" in L.mi_last_error()
    assert call(cfg=pkg.PocsagCfg(correct=3)) == pkg.MI_ERR_INVALID and b"correct" in L.mi_last_error()
    for field, value, words in (("zero", 1, b"the zero field is not 0"), ("phase", 2, b"an unknown walker phase"), ("nbits", 1, b"an idle row with a walker field"),
                                ("open", 1, b"an idle row with a walker field")):
        bad = fresh_state(rows)
        bad[field][1] = value
        assert call(state=bad) == pkg.MI_ERR_INVALID and b"pager plan: malformed state blob: " in L.mi_last_error() and words in L.mi_last_error(), field
    bad = fresh_state(rows)
    bad["msg"]["nwords"][1] = 1
    assert call(state=bad) == pkg.MI_ERR_INVALID and b"an idle row with a walker field or a byte of the message set" in L.mi_last_error()
    bad = fresh_state(rows)
    bad["hist"][0][20] = 1
    assert call(state=bad) == pkg.MI_ERR_INVALID and b"history bits in a lane the baud does not have" in L.mi_last_error()
    assert call(state=bad, cfg=pkg.PocsagCfg(baud=512)) == pkg.MI_OK
    # inside a transmission: each impossible field on its own
    ok = fresh_state(1)
    ok["phase"], ok["lane"], ok["lane_sync"], ok["pos"], ok["nbits"], ok["cur"], ok["mismatches"] = 1, 12, 11, 3, 4, 9, 1
    assert call(rows=1, en=en[:1], state=ok) == pkg.MI_OK, L.mi_last_error()
    for field, value, words in (("lane", 20, b"a lane the baud does not have"), ("lane_sync", 20, b"a lane the baud does not have"), ("lane", 3, b"two slicers"),
                                ("inverted", 2, b"counters"), ("open", 2, b"counters"), ("pos", 17, b"counters"), ("nbits", 32, b"counters"), ("cur", 16, b"counters"),
                                ("gbad", 4, b"counters"), ("mismatches", 5, b"counters"), ("wtwelfth", 24000, b"counters")):
        bad = ok.copy()
        bad[field] = value
        assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"an impossible walker state" in L.mi_last_error() and words in L.mi_last_error(), field
    bad = ok.copy()
    bad["msg"]["address"] = 5
    assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"a message set though none is open" in L.mi_last_error()
    # an open message
    ok["open"], ok["msg"]["address"], ok["msg"]["lane_sync"], ok["msg"]["sync_errors"], ok["msg"]["nwords"], ok["msg"]["words"][0][0] = 1, 0x1FFFFF, 11, 1, 1, 0x80000000
    assert call(rows=1, en=en[:1], state=ok) == pkg.MI_OK, L.mi_last_error()
    for field, value in (("row", 1), ("end_batch", 1), ("lane_end", 1), ("zero", 1), ("zero2", 1), ("address", 1 << 21), ("function", 4), ("nwords", 81), ("truncated", 2),
                         ("truncated", 1), ("twelfth", 24000), ("inverted", 1), ("lane_sync", 12), ("sync_errors", 2)):
        bad = ok.copy()
        bad["msg"][field] = value
        assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"an impossible open message (a field" in L.mi_last_error(), field
    for field, index, value, words in (("bad", 0, 2, b"a bad bit or a word behind nwords"), ("words", 1, 7, b"a bad bit or a word behind nwords"),
                                       ("bad", 0, 1, b"an nbad that the mask does not give")):
        bad = ok.copy()
        bad["msg"][field][0][index] = value
        assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and words in L.mi_last_error(), (field, index)
    bad = ok.copy()
    bad["msg"]["corrected"] = 5
    assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"more repairs than its words can have" in L.mi_last_error()
    assert STATE.itemsize == 800 and MESSAGE.itemsize == 368
