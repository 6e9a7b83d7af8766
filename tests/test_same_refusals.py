"""Every refusal of the SAME stage that needs no GPU: code and words, both sides of every settings bound, the host twin's argument
checks, impossible state blobs, sizes and symbols.  (The refusals of mi_same_process_device are in test_gpu_same.py.)"""
import ctypes as C

import numpy as np
import pytest

from same_model import BURST, MSG_REC, STATE, WAVE_BATCH, fresh_state


def settings_rc(pkg, **fields):
    c, out = pkg.SameCfg(), pkg.SameCfg()
    for k, v in fields.items():
        setattr(c, k, v)
    rc = pkg.lib().mi_same_settings(C.byref(c), C.byref(out))
    return rc, pkg.lib().mi_last_error().decode(), out


DEFAULT = dict(sync_errors=4, max_bad=4, gap_batches=20, space_gain=1.0)


@pytest.mark.parametrize("field,good,bad,words", [
    ("sync_errors", [0, 1, 4, 0x80000000], [5, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFF], "sync_errors must be within 1 .. 4 or MI_SAME_SYNC_EXACT"),
    ("max_bad", [0, 1, 16], [17, 0xFFFFFFFF], "max_bad must be within 1 .. 16"),
    ("gap_batches", [0, 1, 1000], [1001, 0xFFFFFFFF], "gap_batches must be within 1 .. 1000"),
    ("hold_timing", [0, 1], [2, 0xFFFFFFFF], "hold_timing must be 0 or 1"),
    ("min_quality", [0.0, -0.0, 1e-30, 3.0e38], [-1e-30, float("inf"), float("nan")], "min_quality must be finite and not negative"),
    ("space_gain", [0.0, -0.0, 1e-30, 0.5, 3.0e38], [-1e-30, float("inf"), float("-inf"), float("nan")], "space_gain must be finite and above 0"),
])
def test_both_sides_of_every_settings_bound(pkg, field, good, bad, words):
    for v in good:
        rc, _, out = settings_rc(pkg, **{field: v})
        assert rc == pkg.MI_OK, (field, v)
        assert getattr(out, field) == (DEFAULT[field] if field in DEFAULT and v == 0 else np.float32(v) if isinstance(v, float) else v)
    for v in bad:
        rc, msg, _ = settings_rc(pkg, **{field: v})
        assert rc == pkg.MI_ERR_INVALID and words in msg and msg.startswith("SAME stage: "), (field, v, msg)


def test_sizes_and_symbols(pkg):
    L = pkg.lib()
    for sym in pkg.ABI_SYMBOLS:
        if sym.startswith("mi_same_"):
            assert hasattr(L, sym), sym
    assert sum(s.startswith("mi_same_") for s in pkg.ABI_SYMBOLS) == 14
    assert C.sizeof(pkg.SameCfg) == 24 and C.sizeof(pkg.SameText) == 256
    assert pkg.SAME_MESSAGE_DTYPE == MSG_REC and pkg.SAME_STATE_DTYPE == STATE and STATE.itemsize == 1160 and MSG_REC.itemsize == 304
    assert [pkg.same_max_messages(n) for n in (1, 16, 48, 65)] == [7, 37, 101, 137]


def test_null_arguments_and_the_helpers(pkg):
    L = pkg.lib()
    assert L.mi_same_settings(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    out = pkg.SameCfg()
    assert L.mi_same_settings(None, C.byref(out)) == pkg.MI_OK and (out.sync_errors, out.max_bad, out.gap_batches, out.space_gain) == (4, 4, 20, 1.0)
    assert L.mi_same_templates(None) == pkg.MI_ERR_INVALID
    text = pkg.SameText()
    m = np.zeros(1, MSG_REC)
    assert L.mi_same_message_text(None, C.byref(text)) == pkg.MI_ERR_INVALID and L.mi_same_message_text(m.ctypes.data, None) == pkg.MI_ERR_INVALID
    assert L.mi_same_message_text(m.ctypes.data, C.byref(text)) == pkg.MI_ERR_INVALID and b"not a header whose fields are in order" in L.mi_last_error()
    assert L.mi_same_state_size(None) == 0
    assert L.mi_same_set_rows(None, None) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_same_set_timing(None, 1) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_same_last_launch_ms(None, None) == pkg.MI_ERR_INVALID
    assert L.mi_same_get_state(None, None, 0) == pkg.MI_ERR_INVALID and b"SAME stage state" in L.mi_last_error()
    assert L.mi_same_set_state(None, None, 0) == pkg.MI_ERR_INVALID and L.mi_same_download(None, None, None, None, None) == pkg.MI_ERR_INVALID
    assert L.mi_same_process_device(None, None, 0, 1, None, None, None, None, None, None) == pkg.MI_ERR_INVALID
    L.mi_same_destroy(None)


def test_create_refusals_that_come_before_the_device(pkg):
    L = pkg.lib()
    en = np.ones(4, np.uint8)
    h = C.c_void_p()
    assert L.mi_same_create(None, None, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error()
    assert L.mi_same_create(None, en.ctypes.data, 4, 1, 0, 0, None) == pkg.MI_ERR_INVALID
    bad = pkg.SameCfg(sync_errors=9)
    assert L.mi_same_create(C.byref(bad), en.ctypes.data, 4, 1, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID and b"sync_errors" in L.mi_last_error()
    for rows, nb in ((0, 1), (4, 0), (1 << 20, 1), (1 << 12, 1 << 12)):
        assert L.mi_same_create(None, en.ctypes.data, rows, nb, 0, 0, C.byref(h)) == pkg.MI_ERR_INVALID, (rows, nb)
        assert b"SAME stage needs 1 <= rows < 2^20" in L.mi_last_error()


def test_the_host_twin_s_argument_checks_and_impossible_states(pkg):
    L = pkg.lib()
    rows, nb = 2, 1
    en, plane, state = np.ones(rows, np.uint8), np.zeros((rows, nb * WAVE_BATCH), np.float32), fresh_state(rows)
    msgs, first, count = np.zeros(4, MSG_REC), np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)

    def call(cfg=None, en=en, rows=rows, nb=nb, plane=plane, stride=nb * WAVE_BATCH, state=state, msgs=msgs, cap=4, first=first, count=count):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        state = None if state is None else state.copy()  # (the twin updates the blob it is given)
        return L.mi_same_plan_host(None if cfg is None else C.byref(cfg), p(en), rows, nb, p(plane), stride, p(state), None, None, p(msgs), cap, p(first), p(count))

    assert call() == pkg.MI_OK
    for kw in (dict(en=None), dict(plane=None), dict(state=None), dict(msgs=None), dict(first=None), dict(count=None)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"NULL argument" in L.mi_last_error(), kw
    for kw in (dict(rows=0), dict(nb=0), dict(cap=0)):
        assert call(**kw) == pkg.MI_ERR_INVALID and b"SAME plan needs rows >= 1, nbatches >= 1 and max_messages >= 1" in L.mi_last_error(), kw
    assert call(stride=WAVE_BATCH - 1) == pkg.MI_ERR_INVALID and b"a row stride is shorter than the call" in L.mi_last_error()
    assert call(cfg=pkg.SameCfg(max_bad=17)) == pkg.MI_ERR_INVALID and b"max_bad" in L.mi_last_error()
    # (the check comes before anything is read: no plane of that size exists)
    assert call(nb=0x7FFFFFFF, stride=0x7FFFFFFF * WAVE_BATCH) == pkg.MI_ERR_INVALID and b"do not fit the 32-bit count" in L.mi_last_error()
    for field, value, words in (("zero", 1, b"the zero field is not 0"), ("phase", 2, b"an unknown walker phase"), ("grid", 8, b"no multiple of 16 below 768"),
                                ("grid", 768, b"no multiple of 16 below 768"), ("nbits", 1, b"an idle row with a burst field set"),
                                ("deaf", 65, b"deaf beyond 64"), ("an", 3, b"an impossible assembler state"), ("alen0", 4, b"a field set that its bursts do not use"),
                                ("aidle", 20, b"an impossible assembler state")):
        bad = fresh_state(rows)
        bad[1][field] = value
        assert call(state=bad) == pkg.MI_ERR_INVALID and b"SAME plan: malformed state blob: " in L.mi_last_error() and words in L.mi_last_error(), field
    for k in range(3):
        bad = fresh_state(rows)
        bad["bytes"][1][k][0] = 1
        assert call(state=bad) == pkg.MI_ERR_INVALID and b"a byte set behind a burst's length" in L.mi_last_error()
    # inside a burst, with one stored burst: each impossible field on its own
    ok = fresh_state(1)
    ok["phase"], ok["nbytes"], ok["an"], ok["alen0"] = BURST, 6, 1, 5
    ok["bytes"][0][0][:6] = np.frombuffer(b"ZCZC-W", np.uint8)
    ok["bytes"][0][1][:5] = np.frombuffer(b"ZCZC-", np.uint8)
    assert call(rows=1, en=en[:1], state=ok) == pkg.MI_OK, L.mi_last_error()
    for field, value in (("u", 16), ("kind", 1), ("nbits", 8), ("cur", 1), ("nbytes", 3), ("nbytes", 268), ("deaf", 1), ("start_unit", 50000), ("akind", 1),
                         ("nbad", 1), ("plus", 1), ("dashes", 1)):
        bad = ok.copy()
        bad[0][field] = value
        assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"an impossible walker state" in L.mi_last_error(), field
    bad = ok.copy()
    bad["bytes"][0][0][:4] = np.frombuffer(b"NNNN", np.uint8)
    assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"an impossible walker state" in L.mi_last_error()
    for field, value in (("alen0", 3), ("alen0", 269), ("atrunc0", 2), ("astart_unit", 50000), ("alen1", 4)):
        bad = ok.copy()
        bad[0][field] = value
        assert call(rows=1, en=en[:1], state=bad) == pkg.MI_ERR_INVALID and b"an impossible" in L.mi_last_error(), field
