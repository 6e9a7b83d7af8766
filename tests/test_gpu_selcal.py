"""The SELCAL decoder stage on the GPU (mi_selcal_*, csrc/selcal.hip) against the numpy restatement in selcal_model.py and against its
host twin mi_selcal_plan_host.

Every comparison is bit for bit: window records, codes, prefix, counts and the state blob travel and are compared as bytes -- the order
of the energy's sum, the recurrence, the tie rules and the decoder's table are part of the definition.  Every destination buffer is
filled with a sentinel before a call and is longer than the capacity the stage is told; what it must not write must still hold the
sentinel afterwards."""
import numpy as np
import pytest

from selcal_model import (CODE_REC, E2E_CODE, HISTORY, MODE_16, MODE_32, MODE_CUSTOM, NB, NONE8, WAVE_BATCH, WINDOW_REC, code_row, e2e_setup, fresh_state,
                          selcal_model, short_codes, SHORT)
from test_selcal_model import CUSTOM2, builders

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity


class Dest:
    """destination buffers for `cap` codes and rows * 2 nb window records, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, nb, cap, windows=True):
        import torch
        self.cap = cap
        self.codes = torch.full(((cap + GUARD) * CODE_REC.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.windows = torch.full(((rows * 2 * nb + GUARD) * WINDOW_REC.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda") if windows else None
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def selcal_call(sc, d_plane, row_stride, nb, dest, stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    sc.process_device(d_plane.data_ptr(), row_stride, nb, dest.codes.data_ptr(), dest.row_first.data_ptr(), dest.count.data_ptr(),
                      d_windows=None if dest.windows is None else dest.windows.data_ptr(), hip_stream=s)
    return sc.download(s)


def check(what, got, dest, rows, nb, en, want):
    codes, win, row_first, count = got
    w_codes, w_win, w_first, _ = want
    total, k = len(w_codes), min(len(w_codes), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, w_first), f"{what}: row_first_code"
    assert codes.tobytes() == w_codes[:k].tobytes(), f"{what}: codes\n{codes}\nwant\n{w_codes[:k]}"
    d_codes = dest.codes.cpu().numpy()
    assert d_codes[:k * CODE_REC.itemsize].tobytes() == w_codes[:k].tobytes(), f"{what}: codes on the device"
    assert (d_codes[k * CODE_REC.itemsize:] == SENT_BYTE).all(), f"{what}: something was written behind code {k}"
    if dest.windows is None:
        assert win is None
    else:
        on = np.asarray(en, bool)
        bad = np.argwhere(win[on].view(np.uint8).reshape(-1, 2 * nb, 24) != w_win[on].view(np.uint8).reshape(-1, 2 * nb, 24))
        assert win[on].tobytes() == w_win[on].tobytes(), f"{what}: window records, first at {bad[:3]}"
        d_win = dest.windows.cpu().numpy()
        assert (win[~on].view(np.uint8) == SENT_BYTE).all() and (d_win[rows * 2 * nb * 24:] == SENT_BYTE).all(), f"{what}: windows that must not be written"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def run_calls(pkg, plane, cuts, what, cfg=None, model_kw=None, masks=None, cap=0, windows=True, pads=(0,), stream=None, twin_at=None, state=None):
    """One handle over consecutive calls of the lengths `cuts`, call i over a plane laid out for pads[i % len] more batches than the call:
    window records, codes and the state after every call against the model, and the host twin run from the same blob against both.
    masks: the enabled rows of each call (set_rows in between).  twin_at: that call is made by the host twin from the device's state
    blob, whose state goes back to the device.  Returns (codes of all calls, state)."""
    import torch
    rows = plane.shape[0]
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    sc = pkg.Selcal(masks[0], max_batches=max(cuts), cfg=cfg, max_codes=cap)
    if state is None:
        state = fresh_state(rows)
    else:
        sc.set_state(state)
    done, all_codes = 0, []
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            sc.set_rows(en)
        lay = n + pads[i % len(pads)]
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.25))  # behind the call: a level that would name no pair but change E
        w[:, :n * WAVE_BATCH] = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = selcal_model(w[:, :n * WAVE_BATCH], state, en, **(model_kw or {}))
        before = sc.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin = pkg.selcal_plan_host(en, w, cfg, before, nbatches=n)
        on = np.asarray(en, bool)
        assert twin[0].tobytes() == want[0].tobytes() and twin[1][on].tobytes() == want[1][on].tobytes() and twin[4].tobytes() == want[3].tobytes(), \
            f"{what}, call {i}: the twin and the model differ"
        if i == twin_at:
            sc.set_state(twin[4])
        else:
            room = cap or rows * pkg.selcal_max_codes(max(cuts), cfg)
            dest = Dest(rows, n, room, windows)
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_w = to_dev(w)
            else:
                d_w = to_dev(w)
            got = selcal_call(sc, d_w, lay * WAVE_BATCH, n, dest, None if stream is None else stream.cuda_stream)
            check(f"{what}, call {i} at batch {done}", got, dest, rows, n, en, want)
        assert sc.state().tobytes() == want[3].tobytes(), f"{what}, call {i}: state blob after"
        state, done = want[3], done + n
        all_codes.append(want[0])
    sc.close()
    return np.concatenate(all_codes), state


def tiled(plane, rows):
    return plane[np.arange(rows) % plane.shape[0]]


@gpu
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_device_equals_model_and_twin(pkg, rows):
    """Calls of 1 and 4 batches (and the rest of the 24) on one handle over every builder's row: one block, a few, and -- at 70 rows,
    the 27 builders tiled -- many; codes whose pulses begin in one call and end in another; windows that begin in the carried samples."""
    plane = builders(MODE_16)[1]
    plane = tiled(plane, rows) if rows == 70 else plane[8:8 + rows]
    codes, state = run_calls(pkg, plane, (1, 4, 1, 4, 14), f"{rows} rows")
    assert len(codes) >= rows * 15 // 27 and state["window"][0] == 48


@gpu
@pytest.mark.parametrize("cuts", [(24,), (11, 13), (1,) * 24])
def test_24_batches_and_their_cuts_at_70_rows(pkg, cuts):
    """1680 blocks in one launch, the same cut in two, and twenty-four calls of one batch: every cut decodes the same codes into the
    same state"""
    plane = tiled(builders(MODE_16)[1], 70)
    codes, state = run_calls(pkg, plane, cuts, f"cuts {cuts}")
    whole = selcal_model(plane)
    key = lambda cs: sorted((int(c["row"]), int(c["seq"]), bytes(c["tone"]), int(c["last_window"]), int(c["run1"]), int(c["gap"])) for c in cs)  # noqa: E731
    assert key(codes) == key(whole[0]) and len(codes) == 48
    assert state.tobytes() == whole[3].tobytes()


@gpu
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg):
    """rows 1 and 3 sit the second of four calls out -- no record, every byte of their state stays, carried samples included --; the
    third call is made by the host twin from the device's blob and handed back with set_state; the fourth goes on from it.  The blob
    the handle starts from has a window counter about to wrap.  An impossible decoder state is refused."""
    plane = builders(MODE_16)[1][4:9]
    masks = [np.ones(5, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(5, np.uint8), np.ones(5, np.uint8)]
    st = fresh_state(5)
    st["window"], st["seq"] = 0xFFFFFFF8, 3
    st["x"][:] = np.random.default_rng(9).normal(0, 0.05, (5, HISTORY)).astype(np.float32)
    codes, state = run_calls(pkg, plane, (5, 6, 6, 7), "set_rows", masks=masks, twin_at=2, state=st)
    assert len(codes) >= 3 and state["window"][0] == 40
    sc = pkg.Selcal([1], max_batches=2)
    for field, value in (("phase", 6), ("run1", 1), ("zero", 1)):
        bad = fresh_state(1)
        bad[0][field] = value
        with pytest.raises(pkg.MiError) as e:
            sc.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID and "state" in str(e.value)
    sc.close()


@gpu
@pytest.mark.parametrize("windows", [True, False])
def test_capped_codes_padded_unequal_strides_and_a_side_stream(pkg, windows):
    """a code buffer shorter than the call's codes is left untouched beyond its cap, with and without d_windows; the planes are laid
    out for three and for one batch more than the call; everything is enqueued on a side stream with no synchronisation before
    download"""
    import torch
    plane = builders(MODE_16)[1][:12]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    codes, _ = run_calls(pkg, plane, (11, 13), f"cap 3, windows {windows}", cap=3, windows=windows, pads=(3, 1), stream=side)
    assert len(codes) > 3


@gpu
def test_both_table_modes_and_a_custom_table_of_two(pkg):
    plane32 = builders(MODE_32)[1]
    codes, _ = run_calls(pkg, plane32, (9, 15), "SELCAL 32", cfg=pkg.selcal_cfg(MODE_32), model_kw=dict(mode=MODE_32))
    assert len(codes) == 20
    two = np.stack([code_row((0, 1), None, np.array(CUSTOM2), seed=3), np.zeros(NB * WAVE_BATCH)]).astype(np.float32)
    kw = dict(mode=MODE_CUSTOM, freq=CUSTOM2)
    assert (selcal_model(two, **kw)[1]["third"] == NONE8).all()
    run_calls(pkg, two, (24,), "two tones", cfg=pkg.selcal_cfg(MODE_CUSTOM, freq=CUSTOM2), model_kw=kw)
    codes, _ = run_calls(pkg, short_codes(), (18,), "min_run 2", cfg=pkg.selcal_cfg(MODE_16, **SHORT), model_kw=SHORT)  # several codes a row and call
    assert len(codes) >= 6 and np.bincount(codes["row"]).max() == 3


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    sc = pkg.Selcal([1, 1, 0], max_batches=nb)
    dest = Dest(rows, nb, rows)
    plane = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_plane=plane.data_ptr(), row_stride=nb * WAVE_BATCH, d_codes=dest.codes.data_ptr(), d_windows=None, d_first=dest.row_first.data_ptr(),
             d_count=dest.count.data_ptr()):
        sc.process_device(d_plane, row_stride, nbatches, d_codes, d_first, d_count, d_windows=d_windows, hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_codes=None), dict(d_plane=None), dict(d_first=None), dict(d_count=None),
                dict(d_plane=plane.data_ptr() + 4), dict(d_codes=dest.codes.data_ptr() + 4), dict(d_windows=dest.windows.data_ptr() + 4),
                dict(row_stride=nb * WAVE_BATCH + 2), dict(row_stride=WAVE_BATCH), dict(d_first=dest.row_first.data_ptr() + 2)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        sc.download(s)  # nothing was enqueued yet
    call()
    codes, win, first, count = sc.download(s)
    assert tuple(count) == (0, 0) and list(first) == [0, 0, 0, 0] and win is None and len(codes) == 0
    with pytest.raises(pkg.MiError) as e:  # windows asked for after a call that stored none
        sc._nwin = 2 * nb
        sc.download(s)
    assert e.value.code == pkg.MI_ERR_INVALID
    sc.set_timing(True)
    call()
    assert len(sc.last_launch_ms()) == 5
    sc.close()


@gpu
def test_behind_the_demodulator_and_the_voice_band(pkg):
    """An AM carrier with a call on it, about 4 s of u8 I/Q built in numpy, through the demodulator and the stage: the text of the one
    code equals what was sent, records and state equal the model over the audio the demodulator returned; and the same plane through
    the voice band stage at (300, 3400) still decodes."""
    import torch
    dev, chans, iq, nb = e2e_setup(pkg)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
    wo, axc, _, _ = d.process([iq], nb)
    d.close()
    print("flags:", bytes(axc[0][0]).decode())
    assert (axc[0][0][7:] == ord("*")).all(), "the squelch is not open when the call begins"
    plane = np.ascontiguousarray(wo[0][:, :nb * WAVE_BATCH])
    s = torch.cuda.current_stream().cuda_stream
    d_plane = to_dev(plane)
    sc = pkg.Selcal([1], max_batches=nb)
    dest = Dest(1, nb, sc.max_codes)
    got = selcal_call(sc, d_plane, nb * WAVE_BATCH, nb, dest)
    want = selcal_model(plane)
    check("behind the demodulator", got, dest, 1, nb, [1], want)
    assert sc.state().tobytes() == want[3].tobytes()
    assert [pkg.selcal_code_text(c["tone"]) for c in got[0]] == [E2E_CODE]
    vb = pkg.Vband([1], rows_cfg=[(300, 3400)], max_batches=nb)
    d_out = torch.zeros_like(d_plane)
    vb.process_device(d_plane.data_ptr(), nb * WAVE_BATCH, nb, d_out.data_ptr(), nb * WAVE_BATCH, hip_stream=s)
    sc2 = pkg.Selcal([1], max_batches=nb)
    dest2 = Dest(1, nb, sc2.max_codes)
    got2 = selcal_call(sc2, d_out, nb * WAVE_BATCH, nb, dest2)  # (no host synchronisation between the two stages)
    check("behind the voice band stage", got2, dest2, 1, nb, [1], selcal_model(d_out.cpu().numpy()))
    assert [pkg.selcal_code_text(c["tone"]) for c in got2[0]] == [E2E_CODE]
    for h in (sc, sc2, vb):
        h.close()
