"""The ACARS decoder stage without a GPU: the header's symbols, sizes, templates and checksum; the host twin mi_acars_plan_host against
the numpy model of acars_model.py as bytes -- frames, prefix, counts, bits, Q and state --; what every seeded builder must and must not
decode; the state blob's round trip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from acars_model import (CUT_ROW, ETB, ETX, FRAME, FRAME_REC, HISTORY, LONG_TEXT, MAX_BYTES, MIN_SNR_DB, NB, NBITS, NOISE_SNR_DB, NTAU, NWORDS, RAW, STATE,
                         TRACK_LIMIT_PPM, WAVE_BATCH, DRIFTS, DRIFT_BATCHES, acars_model, drift_rows, tracker_cases, crc_kermit, crc_other_order, frame_bytes, frame_fields, fresh_state, run_in_calls, stacked,
                         sync_pattern, templates)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACARS_SYMBOLS = {"mi_acars_" + s for s in ("create", "destroy", "set_rows", "process_device", "download", "state_size", "get_state", "set_state", "set_timing",
                                            "last_launch_ms", "plan_host", "settings", "templates", "crc", "frame_text")}
SENT = 0xA5
_cache = {}


def builders():
    if "b" not in _cache:
        _cache["b"] = stacked()
    return _cache["b"]


def model_calls(cuts, **kw):
    """the model over the stacked builders in calls of `cuts`, computed once"""
    key = (tuple(cuts), tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = run_in_calls(builders()[1], cuts, **kw)
    return _cache[key]


def raw_plan(pkg, cfg, en, plane, nb, state, cap, guard=2):
    """mi_acars_plan_host over sentinel-filled outputs `guard` entries longer than told"""
    rows = plane.shape[0]
    frames = np.full((cap + guard) * FRAME_REC.itemsize, SENT, np.uint8)
    bits = np.full(rows * nb * NTAU * NWORDS + guard, 0xA5A5A5A5, np.uint32)
    q = np.full(rows * nb * NTAU + guard, 0xA5A5A5A5, np.uint32)
    first = np.full(rows + 1 + guard, 0xA5A5A5A5, np.uint32)
    count = np.full(2 + guard, 0xA5A5A5A5, np.uint32)
    state = state.copy()
    en = np.asarray(en, np.uint8)
    rc = pkg.lib().mi_acars_plan_host(C.byref(cfg) if cfg is not None else None, en.ctypes.data, rows, nb, plane.ctypes.data, plane.shape[1], state.ctypes.data,
                                      bits.ctypes.data, q.ctypes.data, frames.ctypes.data, cap, first.ctypes.data, count.ctypes.data)
    return rc, frames, bits, q, first, count, state


def check_twin_call(pkg, what, cfg, en, plane, nb, state, want, cap=0, pad=0):
    """one call of the twin against the model's (frames, bits, q, row_first, state after): every byte, and the sentinels behind them"""
    rows = plane.shape[0]
    w_frames, w_bits, w_q, w_first, w_state = want
    room = cap or max(1, rows * pkg.acars_max_frames(nb))
    lay = np.full((rows, (nb + pad) * WAVE_BATCH), np.float32(0.25))  # what lies behind the call must not be read
    lay[:, :nb * WAVE_BATCH] = plane
    rc, frames, bits, q, first, count, after = raw_plan(pkg, cfg, en, lay, nb, state, room)
    assert rc == pkg.MI_OK, pkg.lib().mi_last_error()
    total, k = len(w_frames), min(len(w_frames), room)
    assert (int(count[0]), int(count[1])) == (total, k) and (count[2:] == 0xA5A5A5A5).all(), f"{what}: counts {count[:2]}, the model has {total}"
    assert np.array_equal(first[:rows + 1], w_first) and (first[rows + 1:] == 0xA5A5A5A5).all(), f"{what}: row_first_frame"
    assert frames[:k * FRAME_REC.itemsize].tobytes() == w_frames[:k].tobytes(), f"{what}: frames"
    assert (frames[k * FRAME_REC.itemsize:] == SENT).all(), f"{what}: something was written behind frame {k}"
    on = np.asarray(en, bool)
    g_bits, g_q = bits[:rows * nb * NTAU * NWORDS].reshape(rows, nb, NTAU, NWORDS), q[:rows * nb * NTAU].reshape(rows, nb, NTAU)
    assert g_bits[on].tobytes() == w_bits[on].tobytes() and g_q[on].tobytes() == w_q[on].tobytes(), f"{what}: bits or Q"
    assert (g_bits[~on] == 0xA5A5A5A5).all() and (g_q[~on] == 0xA5A5A5A5).all() and (bits[rows * nb * NTAU * NWORDS:] == 0xA5A5A5A5).all() and \
        (q[rows * nb * NTAU:] == 0xA5A5A5A5).all(), f"{what}: a disabled row's bits or Q were written"
    assert after.tobytes() == w_state.tobytes(), f"{what}: state blob after"
    return after


# ---------------- symbols, sizes, templates, checksum ----------------

def test_library_exports_the_acars_stage_s_symbols_and_sizes(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    assert re.search(r"MI_ACARS_HISTORY = 6, MI_ACARS_HYPOTHESES = 20, MI_ACARS_BITS = 300, MI_ACARS_BIT_WORDS = 10, MI_ACARS_SYNC_BITS = 39", header)
    assert "MI_ACARS_MAX_BYTES = 240" in header and "MI_ACARS_STATE_ROW_BYTES = 496" in header
    assert "written from memory of the air format" in header and "no off-air ACARS has been through the stage" in header
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", code) if s.startswith("mi_acars_")}
    assert declared == ACARS_SYMBOLS and ACARS_SYMBOLS <= set(pkg.ABI_SYMBOLS)
    assert not [s for s in sorted(declared) if not hasattr(pkg.lib(), s)]
    assert C.sizeof(pkg.AcarsCfg) == 16 and C.sizeof(pkg.AcarsText) == 248
    assert pkg.ACARS_FRAME_DTYPE.itemsize == 272 == FRAME_REC.itemsize and pkg.ACARS_STATE_DTYPE.itemsize == 496 == STATE.itemsize
    for a, b in ((pkg.ACARS_FRAME_DTYPE, FRAME_REC), (pkg.ACARS_STATE_DTYPE, STATE)):
        assert [(n, a.fields[n]) for n in a.names] == [(n, b.fields[n]) for n in b.names]
    assert (pkg.ACARS_HISTORY, pkg.ACARS_BITS, pkg.ACARS_MAX_BYTES, pkg.ACARS_RAW_BYTES, pkg.ACARS_FRAME) == (HISTORY, NBITS, MAX_BYTES, RAW, FRAME)
    filled = pkg.acars_settings()
    assert (filled.sync_errors, filled.keep_bad, filled.min_quality, filled.hold_timing) == (2, 0, 0.0, 0)
    assert pkg.acars_settings(pkg.acars_cfg(sync_errors=pkg.ACARS_SYNC_EXACT)).sync_errors == pkg.ACARS_SYNC_EXACT
    assert pkg.acars_cfg(sync_errors=0).sync_errors == 0 == pkg.acars_cfg(None).sync_errors  # (0 is the default in Python as in C)


def test_templates_within_one_float32_step_of_the_formula(pkg):
    h1, h2 = pkg.acars_templates()
    rho = np.arange(20, dtype=np.float64)
    for got, want in ((h1, np.sin(np.pi * rho / 20)), (h2, np.sin(2 * np.pi * rho / 20))):
        assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    m1, m2 = templates()
    assert h1.tobytes() == m1.tobytes() and h2.tobytes() == m2.tobytes()


def test_crc_is_kermit_and_not_the_other_bit_order(pkg):
    """0x2189 is the catalogue's check value of CRC-16/KERMIT; the bit-by-bit register of the model gives it, the same polynomial
    shifted the other way (XMODEM, 0x31C3) does not, and a frame's bytes with their BCS behind them give 0."""
    assert pkg.acars_crc(b"123456789") == 0x2189 == crc_kermit(b"123456789")
    assert crc_other_order(b"123456789") == 0x31C3 != 0x2189
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 17, 240):
        data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        assert pkg.acars_crc(data) == crc_kermit(data)
        if n:
            assert pkg.acars_crc(data) != crc_other_order(data) or n < 2
    f = frame_bytes(text="CHECK")
    assert pkg.acars_crc(bytes(f)) == 0 and pkg.acars_crc(bytes(f[:-2])) == f[-2] | f[-1] << 8
    assert pkg.lib().mi_acars_crc(None, 3) == 0xFFFFFFFF
    pat = sync_pattern()
    assert len(pat) == 39 and pat.sum() > 8  # (a fresh state's zeros are far from it)


# ---------------- the twin against the model ----------------

@pytest.mark.parametrize("cuts", [(12,), (5, 7), (1,) * 12, (1, 4, 1, 4, 2)])
def test_twin_equals_model_on_every_builder(pkg, cuts):
    names, plane, _, _, _ = builders()
    state, done = fresh_state(len(names)), 0
    for i, (n, want) in enumerate(zip(cuts, model_calls(cuts))):
        state = check_twin_call(pkg, f"cuts {cuts}, call {i}", None, np.ones(len(names)), plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], n, state, want, pad=i % 2)
        done += n
    whole = model_calls((12,))[0]
    key = lambda fs: sorted((int(f["row"]), int(f["batch"]), int(f["third"]), bytes(f["bytes"])) for f in fs)  # noqa: E731
    assert key(np.concatenate([c[0] for c in model_calls(cuts)])) == key(whole[0]) and state.tobytes() == whole[4].tobytes()


@pytest.mark.parametrize("rows,nb", [(1, 1), (1, 4), (5, 1), (5, 4)])
def test_twin_equals_model_at_small_geometries_with_a_disabled_row_and_a_cap(pkg, rows, nb):
    names, plane, _, _, _ = builders()
    r0 = names.index("start at third 19")
    sub = np.ascontiguousarray(plane[r0:r0 + rows, :nb * WAVE_BATCH])
    en = np.ones(rows, np.uint8)
    if rows > 1:
        en[2] = 0
    st = fresh_state(rows)
    st["x"][:] = np.random.default_rng(3).normal(0, 0.1, (rows, HISTORY)).astype(np.float32)
    want = acars_model(sub, st, en)
    check_twin_call(pkg, f"{rows} x {nb}", None, en, sub, nb, st, want, pad=1)
    if nb == 4 and rows == 5:
        assert len(want[0]) == 4
        check_twin_call(pkg, "a cap of 2", None, en, sub, nb, st, want, cap=2)


@pytest.mark.parametrize("kw", [dict(keep_bad=True), dict(sync_errors=0), dict(sync_errors=4), dict(hold_timing=True), dict(min_quality=1.0)])
def test_twin_equals_model_under_every_setting(pkg, kw):
    names, plane, _, _, _ = builders()
    want = model_calls((12,), **kw)[0]
    cfg = pkg.acars_cfg(**{k: (v or pkg.ACARS_SYNC_EXACT) if k == "sync_errors" else v for k, v in kw.items()})
    check_twin_call(pkg, str(kw), cfg, np.ones(len(names)), plane, 12, fresh_state(len(names)), want)


# ---------------- every timing move, one by one ----------------

def bits_taken(st):
    return 8 * (st["nbytes"].astype(np.int64) + np.maximum(st["tail"].astype(np.int64) - 1, 0)) + st["nbits"]


def check_tracker_moves(what, cases, before, after, frames, hold=False):
    """what every seeded row of tracker_cases() must have done in its one batch"""
    took = bits_taken(after) - bits_taken(before)
    for r, (name, u, _, _, _, v, nbits, nframes) in enumerate(cases):
        mine = frames[frames["row"] == r]
        if hold:
            if nframes:  # one bit was missing: slot 0 on hypothesis u gives it, and the row is idle
                assert after["phase"][r] != FRAME, f"{what}, {name}"
            else:
                assert after["phase"][r] == FRAME and after["u"][r] == u and took[r] == 300, f"{what}, {name}: hold_timing moved"
            continue
        assert len(mine) == nframes, f"{what}, {name}: frames"
        if nframes:  # the bit taken again was the frame's last: a record with a valid checksum, and the row idle
            assert after["phase"][r] != FRAME and mine[0]["crc_ok"] == 1 and (mine[0]["tau_sync"], mine[0]["tau_end"]) == (u, v) and mine[0]["end_batch"] == 0
            assert frame_fields(mine[0])["text"] == "TRK" and (mine[0]["batch"], mine[0]["third"]) == (6, 4321)
        else:
            assert after["phase"][r] == FRAME and after["u"][r] == v and took[r] == nbits, f"{what}, {name}: u {after['u'][r]}, {took[r]} bits"


def test_every_timing_move_from_a_seeded_state(pkg):
    """u - 1 and u + 1, both wraps between 19 and 0, the slot passed over (0 -> 1), the carried bit taken again (1 -> 0) where it
    ends nothing, a byte and the frame, the neighbours' exact tie and the tie of all: the model does what the header says, and the
    twin equals it byte for byte; under hold_timing nothing moves"""
    names, st, plane, cases = tracker_cases()
    assert {(c[1], c[5]) for c in cases} >= {(10, 9), (10, 11), (0, 19), (19, 0), (0, 1), (1, 0), (10, 10)}
    want = acars_model(plane, st)
    tie = names.index("the neighbours tie above u")
    assert want[2][tie, 0, 9] == want[2][tie, 0, 11] > want[2][tie, 0, 10] == 0
    check_tracker_moves("model", cases, st, want[4], want[0])
    byte = names.index("1 -> 0, the bit retaken ends a byte")
    assert want[4]["nbytes"][byte] >= 6 and want[4]["bytes"][byte][5] == frame_bytes(text="TRK", address=".TRACK1", label="5Z", block_id="9")[5]
    check_twin_call(pkg, "tracker", None, np.ones(len(names)), plane, 1, st, want)
    held = acars_model(plane, st, hold_timing=True)
    check_tracker_moves("model, hold_timing", cases, st, held[4], held[0], hold=True)
    check_twin_call(pkg, "tracker, hold_timing", pkg.acars_cfg(hold_timing=True), np.ones(len(names)), plane, 1, st, held)


def check_drift(what, states, frames):
    """states: the blob after each of the 8 batches; frames: all records"""
    for r, (name, _, _, path) in enumerate(DRIFTS):
        got = [int(st["u"][r]) if st["phase"][r] == FRAME else -1 for st in states]
        assert got == path, f"{what}, {name}: u went {got}"
        mine = frames[frames["row"] == r]
        assert len(mine) == 1 and mine[0]["crc_ok"] == 1 and (mine[0]["tau_sync"], mine[0]["tau_end"]) == (path[0], path[-2]) and \
            frame_fields(mine[0])["text"] == LONG_TEXT, f"{what}, {name}"


def test_the_walker_follows_a_drifting_clock_through_both_wraps(pkg):
    plane = drift_rows()
    calls = run_in_calls(plane, (1,) * DRIFT_BATCHES)
    check_drift("model", [c[4] for c in calls], np.concatenate([c[0] for c in calls]))
    state = fresh_state(2)
    for b, want in enumerate(calls):
        state = check_twin_call(pkg, f"drift, batch {b}", None, [1, 1], plane[:, b * WAVE_BATCH:(b + 1) * WAVE_BATCH], 1, state, want)
    held = acars_model(plane, hold_timing=True)
    assert len(held[0]) == 0  # (without the moves a drift of seven thirds loses both frames)


# ---------------- every builder does its job ----------------

def test_the_frames_found_are_the_frames_sent(pkg):
    names, plane, tail, found, kept = builders()
    frames, _, _, first, _, state = pkg.acars_plan_host(np.ones(len(names)), plane)
    bad, _, _, bfirst, _, _ = pkg.acars_plan_host(np.ones(len(names)), plane, pkg.acars_cfg(keep_bad=True))
    for r, name in enumerate(names):
        got = frames[first[r]:first[r + 1]]
        assert [frame_fields(f) for f in got] == found[r], name
        assert [pkg.acars_frame_text(f) for f in got] == [{k: v for k, v in f.items() if k != "end"} for f in found[r]], name
        assert all(f["crc_ok"] == 1 and f["row"] == r for f in got)
        more = bad[bfirst[r]:bfirst[r + 1]]
        assert len([f for f in more if not f["crc_ok"]]) == len(kept[r]), name
    st = state.view(STATE)
    assert [names[r] for r in range(len(names)) if st["phase"][r] == FRAME] == [CUT_ROW]
    by = dict(zip(names, range(len(names))))
    a, b = frames[first[by["a clean frame"]]], frames[first[by["the same inverted"]]]
    assert a["bytes"].tobytes() == b["bytes"].tobytes() and a["third"] == b["third"] and a["tau_sync"] == b["tau_sync"]
    f = frames[first[by["the longest frame"]]]
    assert f["nbytes"] == MAX_BYTES and frame_fields(f)["text"] == LONG_TEXT and f["end"] == ETX
    assert frames[first[by["an empty text"]]]["nbytes"] == 13 and frames[first[by["ETB"]]]["end"] == ETB
    assert frames[first[by["a parity error under a matching BCS"]]]["parity_errors"] == 1
    assert frames[first[by["a frame that starts in the last bits of a batch"]]]["third"] >= 3 * WAVE_BATCH - 60
    assert {int(frames[first[by[f"start at third {s}"]]]["tau_end"]) for s in range(20)} >= set(range(4, 20))
    assert NOISE_SNR_DB == MIN_SNR_DB + 3 and TRACK_LIMIT_PPM > 0
    # the frame cut by the end of the plane ends in the next call, out of the state
    r = by[CUT_ROW]
    more, _, _, _, _, after = pkg.acars_plan_host([1], tail[r:r + 1], state=state.view(STATE)[r:r + 1])
    assert len(more) == 1 and more[0]["batch"] == NB - 3 and len(frame_fields(more[0])["text"]) == 200 and after.view(STATE)["phase"][0] != FRAME


def test_state_blob_round_trip_and_its_refusals(pkg):
    names, plane, _, _, _ = builders()
    r = names.index(CUT_ROW)
    _, _, _, _, _, state = pkg.acars_plan_host([1], plane[r:r + 1])
    st = state.view(STATE)
    assert st["phase"][0] == FRAME and st["nbytes"][0] > 12 and st["crc"][0] == crc_kermit(bytes(st["bytes"][0][:int(st["nbytes"][0])]))
    again = pkg.acars_plan_host([1], np.zeros((1, WAVE_BATCH), np.float32), state=state)  # the blob as it came goes in again
    assert again[5].view(STATE)["batch"][0] == NB + 1
    for field, value in (("phase", 2), ("u", 20), ("prev", 2), ("nbits", 8), ("cur", 255), ("tail", 3), ("nbytes", 240), ("crc", int(st["crc"][0]) ^ 1),
                         ("parity_errors", 77), ("start_third", 6000), ("tau_sync", 20), ("mismatches", 5), ("end", 3), ("zero", 1)):
        bad = st.copy()
        bad[0][field] = value
        rc = raw_plan(pkg, None, [1], np.zeros((1, WAVE_BATCH), np.float32), 1, bad.view(np.uint8), 1)[0]
        assert rc == pkg.MI_ERR_INVALID and b"malformed state blob" in pkg.lib().mi_last_error(), field
    for field, index, value in (("hist", 3, 1 << 38), ("bytes", RAW - 1, 1)):
        bad = st.copy()
        bad[0][field][index] = value
        assert raw_plan(pkg, None, [1], np.zeros((1, WAVE_BATCH), np.float32), 1, bad.view(np.uint8), 1)[0] == pkg.MI_ERR_INVALID, field
    idle = fresh_state(1)
    idle["nbytes"] = 1
    assert raw_plan(pkg, None, [1], np.zeros((1, WAVE_BATCH), np.float32), 1, idle.view(np.uint8), 1)[0] == pkg.MI_ERR_INVALID
