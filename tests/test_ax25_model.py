"""The packet stage's host twin (mi_ax25_plan_host) against the numpy / Python restatement in ax25_model.py, as bytes: tone bits,
frames, prefix, counts and state, on every builder, at every cut; the helpers (CRC, templates, TNC2 text); the ordering rule and
the capacity bound from seeded states.  No GPU."""
import functools

import numpy as np
import pytest

import ax25_model as m
from ax25_model import FRAME_REC, NB, WAVE_BATCH, ax25_model, fresh_state


@functools.lru_cache(maxsize=None)
def builders():
    """(names, plane, found, loose, the model over the whole plane from a fresh state) -- computed once"""
    names, plane, found, loose = m.stacked()
    return names, plane, found, loose, ax25_model(plane)


def sent(frames, first, r):
    return [bytes(f["bytes"][:f["nbytes"]]) for f in frames[first[r]:first[r + 1]]]


def same(what, twin, want):
    frames, bits, first, count, state = twin
    w_frames, w_bits, w_first, w_state = want
    assert frames.tobytes() == w_frames.tobytes(), f"{what}: frames\n{frames[['row', 'batch', 'third', 'lane', 'nbytes']]}\nwant\n{w_frames[['row', 'batch', 'third', 'lane', 'nbytes']]}"
    assert bits.tobytes() == w_bits.tobytes(), f"{what}: tone bits, first at {np.argwhere(bits != w_bits)[:3]}"
    assert np.array_equal(first, w_first) and tuple(count) == (len(w_frames),) * 2, f"{what}: prefix or counts"
    assert state.tobytes() == w_state.tobytes(), f"{what}: state blob"


def test_the_model_finds_what_the_builders_send():
    names, plane, found, loose, whole = builders()
    frames, _, first, state = whole
    for r, name in enumerate(names):
        assert sent(frames, first, r) == found[r], name
    loose_run = ax25_model(plane[[names.index("a bad callsign byte")]], strict=False)
    assert sent(loose_run[0], loose_run[2], 0) == loose[names.index("a bad callsign byte")] and loose_run[0][0]["naddr"] == 0
    lanes = {n: int(frames[first[names.index(n)]]["lane"]) // 10 for n in ("space 6 dB down", "space 6 dB up")}
    print("slicers of the tilted frames:", lanes)
    assert (state["batch"] == NB).all()


def test_which_slicers_decode_the_tilted_frames(pkg):
    """Each slicer alone (the other two gains out of reach) on the tilted builders.  Space 6 dB down and 6 dB up on noise-free audio
    decode on every slicer -- the detector is far from its threshold there, which is printed, not asserted.  What the
    three slicers are for is asserted on two rows: the space tone down by the measured tilt near the noise limit is lost on the flat
    slicer and kept on the other two, and a space tone 26 dB up is lost on slicer 2 and kept on the other two; the default handle
    finds all four."""
    names, plane, found, _, _ = builders()
    off = 1e30
    for name in ("space 6 dB down", "space 6 dB up", m.TILT_DOWN, m.TILT_UP):
        r = names.index(name)
        alone = []
        for gain in ((1.0, off, off), (off, m.DEFAULT_GAIN[1], off), (off, off, m.DEFAULT_GAIN[2])):
            frames, _, first, _, _ = pkg.ax25_plan_host([1], plane[r:r + 1], pkg.ax25_cfg(gain=gain))
            alone.append(sent(frames, first, 0) == found[r])
        print(f"{name}: slicers alone {alone}")
        frames, _, first, _, _ = pkg.ax25_plan_host([1], plane[r:r + 1])
        assert sent(frames, first, 0) == found[r] and any(alone), name
        if name in m.SLICERS_ALONE:
            assert alone == m.SLICERS_ALONE[name], name


@pytest.mark.parametrize("cuts", [(48,), (20, 28), (1,) * 48])
@pytest.mark.parametrize("rows", [1, 5])
def test_twin_equals_model_on_every_builder(pkg, rows, cuts):
    """the twin over every builder's row in groups of `rows`, the 48 batches cut as `cuts`: every call's frames, bits, prefix, counts
    and state equal those of the model run in the same calls, for every group, and the calls' frames and the final state equal the
    whole-plane model's"""
    names, plane, found, _, whole = builders()
    for g0 in range(0, len(names), rows):
        rws = slice(g0, min(g0 + rows, len(names)))
        n = rws.stop - rws.start
        en = np.ones(n, np.uint8)
        want_calls = m.run_in_calls(plane[rws], cuts)
        state, done, got = fresh_state(n), 0, []
        for i, c in enumerate(cuts):
            twin = pkg.ax25_plan_host(en, plane[rws, done * WAVE_BATCH:(done + c) * WAVE_BATCH], None, state)
            same(f"rows {rws}, call {i}", twin, want_calls[i])
            fr = twin[0].copy()
            fr["end_batch"] += done
            got.append(fr)
            state, done = twin[4], done + c
        got = np.concatenate(got)
        got = got[np.argsort(got["row"], kind="stable")]
        w = whole[0][(whole[0]["row"] >= rws.start) & (whole[0]["row"] < rws.stop)].copy()
        w["row"] -= rws.start
        assert got.tobytes() == w.tobytes(), f"rows {rws}, cuts {cuts}: frames"
        assert state.tobytes() == whole[3][rws].tobytes(), f"rows {rws}, cuts {cuts}: state"


@pytest.mark.parametrize("cuts", [(48,), (20, 28), (1,) * 48])
def test_twin_equals_model_without_strict(pkg, cuts):
    """the bad callsign byte's row, beside a well-formed one, under MI_AX25_STRICT_OFF: the twin equals the model call by call, and
    the malformed frame is one record with naddr 0 whose bytes are the ones sent; under strict the twin drops it"""
    names, plane, found, loose, _ = builders()
    r = names.index("a bad callsign byte")
    rws = [r, names.index("a short UI frame")]
    cfg = pkg.ax25_cfg(strict=False)
    want_calls = m.run_in_calls(plane[rws], cuts, strict=False)
    state, done, got = fresh_state(2), 0, []
    for i, c in enumerate(cuts):
        twin = pkg.ax25_plan_host([1, 1], plane[rws, done * WAVE_BATCH:(done + c) * WAVE_BATCH], cfg, state)
        same(f"strict off, call {i}", twin, want_calls[i])
        got.append(twin[0])
        state, done = twin[4], done + c
    got = np.concatenate(got)
    bad = got[got["row"] == 0]
    assert len(bad) == 1 and bad[0]["naddr"] == 0 and [bytes(bad[0]["bytes"][:bad[0]["nbytes"]])] == loose[r] and (got[got["row"] == 1]["naddr"] == 2).all()
    frames, _, first, _, _ = pkg.ax25_plan_host([1, 1], plane[rws])
    assert sent(frames, first, 0) == [] and sent(frames, first, 1) == found[rws[1]]


def test_the_40_start_thirds(pkg):
    plane, f = m.start_thirds()
    want = ax25_model(plane)
    same("start thirds", pkg.ax25_plan_host(np.ones(40), plane), want)
    assert [sent(want[0], want[2], r) for r in range(40)] == [[f]] * 40
    print("lanes by start third:", [int(x) for x in want[0]["lane"]])


def test_a_disabled_row_padded_strides_and_capped_sentinel_filled_outputs(pkg):
    import ctypes as C
    names, plane, _, _, _ = builders()
    rows, nb, pad = 6, 6, 7 * 4
    en = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    wide = np.full((rows, nb * WAVE_BATCH + pad), np.float32(0.25))
    wide[:, :nb * WAVE_BATCH] = plane[:rows, :nb * WAVE_BATCH]
    st = fresh_state(rows)
    st["x"] = np.random.default_rng(5).normal(0, 0.1, (rows, 14)).astype(np.float32)
    st["batch"][1] = 3
    m.seed_lane(st[1], 7, m.ui_frame(**m.SHORT), 9, 0)  # a disabled row inside a frame: every byte stays
    want = ax25_model(wide[:, :nb * WAVE_BATCH], st, en)
    assert len(want[0]) >= 3
    same("a disabled row, padded", pkg.ax25_plan_host(en, wide, None, st, nbatches=nb), want)
    assert want[3][1].tobytes() == st[1].tobytes() and want[3][4].tobytes() == st[4].tobytes()
    cap = 2
    frames = np.full(cap + 3, 0xA5, np.uint8).repeat(FRAME_REC.itemsize).view(FRAME_REC)
    first, count, blob = np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32), st.copy()
    cfg = pkg.ax25_cfg()
    assert pkg.lib().mi_ax25_plan_host(C.byref(cfg), en.ctypes.data, rows, nb, wide.ctypes.data, wide.shape[1], blob.ctypes.data, None, frames.ctypes.data,
                                       cap, first.ctypes.data, count.ctypes.data) == pkg.MI_OK
    assert tuple(count) == (len(want[0]), cap) and frames[:cap].tobytes() == want[0][:cap].tobytes() and (frames[cap:].view(np.uint8) == 0xA5).all()
    assert blob.tobytes() == want[3].tobytes() and np.array_equal(first, want[2])


def test_the_ordering_rule_branch_by_branch(pkg):
    names, st, plane, expect = m.ordering_cases()
    want = ax25_model(plane, st)
    same("ordering", pkg.ax25_plan_host(np.ones(len(names)), plane, None, st), want)
    assert [int(want[2][r + 1] - want[2][r]) for r in range(len(names))] == expect, list(zip(names, np.diff(want[2])))
    assert int(want[0][0]["lane"]) == 0 and int(want[0][1]["lane"]) == 0, "the lower lane of two is the record"


@pytest.mark.parametrize("nb", [1, 2])
def test_the_capacity_bound_is_reached(pkg, nb):
    st, plane = m.capacity_case(nb)
    want = ax25_model(plane, st)
    assert len(want[0]) == m.max_frames(nb) == pkg.ax25_max_frames(nb) == 1 + 150 * nb // 143
    same(f"capacity, {nb} batches", pkg.ax25_plan_host([1], plane, None, st), want)
    assert (want[0]["nbytes"] == 17).all()


def test_crc_and_templates(pkg):
    assert pkg.ax25_crc(b"123456789") == 0x906E == m.crc_x25(b"123456789")
    assert pkg.ax25_crc(b"") == 0 and pkg.lib().mi_ax25_crc(None, 3) == 0xFFFFFFFF
    f = m.ui_frame(**m.SHORT)
    assert m.crc_register(m.bits_of(f)) == 0xF0B8 == pkg.AX25_RESIDUE and pkg.ax25_crc(bytes(f)) == 0xF0B8 ^ 0xFFFF
    assert m.FLAG_RESIDUE == pkg.AX25_FLAG_RESIDUE
    rng = np.random.default_rng(3)
    for n in (1, 2, 17, 330):
        data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        assert pkg.ax25_crc(data) == m.crc_x25(data)
    t = pkg.ax25_templates()
    rho = np.arange(40, dtype=np.float64)
    for i, (fn, hz) in enumerate(((np.cos, 1200.0), (np.sin, 1200.0), (np.cos, 2200.0), (np.sin, 2200.0))):
        exact = fn(2 * np.pi * hz * rho / 48000.0)
        assert (np.abs(t[i].astype(np.float64) - exact) <= np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)).all(), i
    d = pkg.ax25_settings()
    assert tuple(d.gain) == tuple(np.float32(g) for g in m.DEFAULT_GAIN) and d.strict == 1
    assert abs(d.gain[1] ** 2 / d.gain[2] - 1) < 1e-3, "gain[1] is the geometric mean of gain[0] = 1 and gain[2]"


def test_the_tnc2_line(pkg):
    def rec(f):
        r = np.zeros((), FRAME_REC)
        r["nbytes"] = len(f)
        r["bytes"][:len(f)] = f
        return r

    f0 = m.ui_frame(src="N0CALL", src_ssid=7, dst="APRS", info=b"hi\x01there\x7f")
    assert pkg.ax25_frame_text(rec(f0)) == "N0CALL-7>APRS:hi.there." == m.tnc2(rec(f0))
    f1 = m.ui_frame(src="AB1CD", dst="APZ", dst_ssid=3, digis=[("WIDE1", 1, False)], info=b"x")
    assert pkg.ax25_frame_text(rec(f1)) == "AB1CD>APZ-3,WIDE1-1:x" == m.tnc2(rec(f1))
    f8 = m.ui_frame(**m.LONGEST)
    line = pkg.ax25_frame_text(rec(f8))
    assert line == m.tnc2(rec(f8)) and line.startswith("LONG-15>APZ123,DIGI1-1,DIGI2-2*,DIGI3-3,DIGI4-4,DIGI5-5,DIGI6-6,DIGI7-7,DIGI8-8:") and len(line) < pkg.AX25_TEXT_BYTES
    bad = m.ui_frame(src="n0call", info=b"x")
    with pytest.raises(pkg.MiError) as e:
        pkg.ax25_frame_text(rec(bad))
    assert e.value.code == pkg.MI_ERR_INVALID and "address field is not well formed" in str(e.value)


def test_ten_minutes_of_noise_and_of_voice_give_no_record(pkg):
    """4800 batches each through the twin under strict.  (The frame check alone admits about one false frame in 2^16 candidates
    of whole bytes; tools/ax25_classes.py counts what strict off gives.)"""
    n = 4800 * WAVE_BATCH
    for what, x in (("noise", np.random.default_rng(11).normal(0, 0.1, n)), ("voice", m.voice_like(n, 12))):
        frames = pkg.ax25_plan_host([1], x.astype(np.float32)[None, :])[0]
        assert len(frames) == 0, (what, frames[["batch", "lane", "nbytes"]])
