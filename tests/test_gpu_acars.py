"""The ACARS decoder stage on the GPU (mi_acars_*, csrc/acars.hip) against the numpy restatement in acars_model.py and against its
host twin mi_acars_plan_host.

Every comparison is bit for bit: change bits, Q, frames, prefix, counts and the state blob travel and are compared as bytes.  Every
destination buffer is filled with a sentinel before a call and is longer than the capacity the stage is told; what it must not write
must still hold the sentinel afterwards."""
import numpy as np
import pytest

from acars_model import (CUT_ROW, E2E_FRAME, FRAME, FRAME_REC, NB, NTAU, NWORDS, WAVE_BATCH, acars_model, e2e_setup, frame_fields, fresh_state, drift_rows, DRIFT_BATCHES, tracker_cases)
from test_acars_model import builders, check_drift, check_tracker_moves

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity


class Dest:
    """destination buffers for `cap` frames and the rows * nb blocks' bits and Q, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, nb, cap):
        import torch
        self.cap = cap
        self.frames = torch.full(((cap + GUARD) * FRAME_REC.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.bits = torch.full((rows * nb * NTAU * NWORDS + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.q = torch.full((rows * nb * NTAU + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def acars_call(ac, d_plane, row_stride, nb, dest, stream=None, scratch=False):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    ac.process_device(d_plane.data_ptr(), row_stride, nb, dest.frames.data_ptr(), dest.row_first.data_ptr(), dest.count.data_ptr(),
                      d_bits=None if scratch else dest.bits.data_ptr(), d_q=None if scratch else dest.q.data_ptr(), hip_stream=s)
    return ac.download(s)


def check(what, got, dest, rows, nb, en, want, scratch=False):
    frames, row_first, count = got
    w_frames, w_bits, w_q, w_first, _ = want
    total, k = len(w_frames), min(len(w_frames), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, w_first), f"{what}: row_first_frame"
    assert frames.tobytes() == w_frames[:k].tobytes(), f"{what}: frames\n{frames}\nwant\n{w_frames[:k]}"
    d_frames = dest.frames.cpu().numpy()
    assert d_frames[:k * FRAME_REC.itemsize].tobytes() == w_frames[:k].tobytes(), f"{what}: frames on the device"
    assert (d_frames[k * FRAME_REC.itemsize:] == SENT_BYTE).all(), f"{what}: something was written behind frame {k}"
    bits, q = dest.bits.cpu().numpy().view(np.uint32), dest.q.cpu().numpy()
    if scratch:
        assert (bits == 0xA5A5A5A5).all() and (q == SENT32).all(), f"{what}: bits or Q written though the call gave none"
    else:
        on = np.asarray(en, bool)
        g_bits, g_q = bits[:rows * nb * NTAU * NWORDS].reshape(rows, nb, NTAU, NWORDS), q[:rows * nb * NTAU].view(np.float32).reshape(rows, nb, NTAU)
        bad = np.argwhere(g_bits[on] != w_bits[on])
        assert not len(bad), f"{what}: change bits, first at {bad[:3]}"
        assert g_q[on].tobytes() == w_q[on].tobytes(), f"{what}: Q, first at {np.argwhere(g_q[on].view(np.uint32) != w_q[on].view(np.uint32))[:3]}"
        assert (g_bits[~on] == 0xA5A5A5A5).all() and (bits[rows * nb * NTAU * NWORDS:] == 0xA5A5A5A5).all() and (q[rows * nb * NTAU:] == SENT32).all(), \
            f"{what}: bits or Q that must not be written"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def run_calls(pkg, plane, cuts, what, cfg=None, model_kw=None, masks=None, cap=0, pads=(0,), stream=None, twin_at=None, state=None, scratch=False):
    """One handle over consecutive calls of the lengths `cuts`, call i over a plane laid out for pads[i % len] more batches than the
    call: bits, Q, frames and the state after every call against the model, and the host twin run from the same blob against both.
    masks: the enabled rows of each call (set_rows in between).  twin_at: that call is made by the host twin from the device's state
    blob, whose state goes back to the device.  Returns (frames of all calls, state)."""
    import torch
    rows = plane.shape[0]
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    ac = pkg.Acars(masks[0], max_batches=max(cuts), cfg=cfg, max_frames=cap)
    if state is None:
        state = fresh_state(rows)
    else:
        ac.set_state(state)
    done, all_frames = 0, []
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            ac.set_rows(en)
        lay = n + pads[i % len(pads)]
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.25))  # behind the call: a level that must not be read
        w[:, :n * WAVE_BATCH] = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = acars_model(w[:, :n * WAVE_BATCH], state, en, **(model_kw or {}))
        before = ac.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin = pkg.acars_plan_host(en, w, cfg, before, nbatches=n)
        assert twin[0].tobytes() == want[0].tobytes() and twin[1].tobytes() == want[1].tobytes() and twin[2].tobytes() == want[2].tobytes() and \
            twin[5].tobytes() == want[4].tobytes(), f"{what}, call {i}: the twin and the model differ"
        if i == twin_at:
            ac.set_state(twin[5])
        else:
            room = cap or rows * pkg.acars_max_frames(max(cuts))
            dest = Dest(rows, n, room)
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_w = to_dev(w)
            else:
                d_w = to_dev(w)
            got = acars_call(ac, d_w, lay * WAVE_BATCH, n, dest, None if stream is None else stream.cuda_stream, scratch)
            check(f"{what}, call {i} at batch {done}", got, dest, rows, n, en, want, scratch)
        assert ac.state().tobytes() == want[4].tobytes(), f"{what}, call {i}: state blob after"
        state, done = want[4], done + n
        all_frames.append(want[0])
    ac.close()
    return np.concatenate(all_frames), state


def tiled(plane, rows):
    return plane[np.arange(rows) % plane.shape[0]]


def key(frames):
    return sorted((int(f["row"]), int(f["batch"]), int(f["third"]), bytes(f["bytes"])) for f in frames)


@gpu
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_device_equals_model_and_twin(pkg, rows):
    """Calls of 1 and 4 batches (and the rest of the 12) on one handle: over the longest frame's row at 1 row, over it and its four
    neighbours at 5, and over every builder's row, tiled, at 70 -- one block, a few, many; frames that begin in one call and end in
    another; bits that begin in the carried samples."""
    names, plane, _, found, _ = builders()
    first = names.index("the longest frame")
    plane = tiled(plane, rows) if rows == 70 else plane[first:first + rows]
    frames, state = run_calls(pkg, plane, (1, 4, 1, 4, 2), f"{rows} rows")
    assert len(frames) >= rows * 2 // 3 and state["batch"][0] == NB


@gpu
@pytest.mark.parametrize("cuts", [(12,), (5, 7), (1,) * 12])
def test_12_batches_and_their_cuts_at_70_rows(pkg, cuts):
    """840 blocks in one launch, the same cut in two where a frame's SOH lies across the calls, and twelve calls of one batch: every
    cut decodes the same frames into the same state"""
    names, plane, _, found, _ = builders()
    plane = tiled(plane, 70)
    frames, state = run_calls(pkg, plane, cuts, f"cuts {cuts}")
    whole = acars_model(plane)
    assert key(frames) == key(whole[0]) and len(frames) == sum(len(found[r % len(names)]) for r in range(70))
    assert state.tobytes() == whole[4].tobytes()


@gpu
def test_set_rows_between_calls_the_host_twin_and_a_frame_across_planes(pkg):
    """rows 1 and 3 sit the second of four calls out -- no record, every byte of their state stays --; the third call is made by the
    host twin from the device's blob and handed back with set_state; the fourth goes on from it.  The blob the handle starts from has a
    batch counter about to wrap.  Then the frame cut by the end of the plane: it stays in the state and ends in the next call.  An
    impossible walker state is refused."""
    names, plane, tail, found, _ = builders()
    masks = [np.ones(5, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(5, np.uint8), np.ones(5, np.uint8)]
    st = fresh_state(5)
    st["batch"] = 0xFFFFFFFD
    st["x"][:] = np.random.default_rng(9).normal(0, 0.05, (5, 6)).astype(np.float32)
    frames, state = run_calls(pkg, plane[:5], (2, 3, 3, 4), "set_rows", masks=masks, twin_at=2, state=st, cfg=pkg.acars_cfg(keep_bad=True),
                              model_kw=dict(keep_bad=True))
    assert len(frames) >= 3 and state["batch"][0] == 9
    r = names.index(CUT_ROW)
    both = np.concatenate([plane[r:r + 1], tail[r:r + 1]], axis=1)
    frames, state = run_calls(pkg, both, (NB, tail.shape[1] // WAVE_BATCH), "a frame across planes")
    assert len(frames) == 1 and frames[0]["batch"] == NB - 3 and frames[0]["end_batch"] == 3 and frame_fields(frames[0])["text"] != ""
    ac = pkg.Acars([1], max_batches=2)
    for field, value in (("phase", 2), ("u", 1), ("zero", 1), ("hist", 1 << 38)):
        bad = fresh_state(1)
        bad[0][field] = value
        with pytest.raises(pkg.MiError) as e:
            ac.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID and "state" in str(e.value)
    ac.close()


@gpu
@pytest.mark.parametrize("scratch", [False, True])
def test_capped_frames_padded_unequal_strides_and_a_side_stream(pkg, scratch):
    """a frame buffer shorter than the call's frames is left untouched beyond its cap, with the bits and Q in the caller's buffers
    and in the handle's; the planes are laid out for three and for one batch more than the call; everything is enqueued on a side
    stream with no synchronisation before download"""
    import torch
    plane = builders()[1][:12]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    frames, _ = run_calls(pkg, plane, (5, 7), f"cap 3, scratch {scratch}", cap=3, pads=(3, 1), stream=side, scratch=scratch)
    assert len(frames) > 3


@gpu
def test_settings_on_the_device(pkg):
    """keep_bad, an exact sync, hold_timing and a quality floor, each against the model"""
    names, plane, _, _, kept = builders()
    rows = [names.index(n) for n in ("one flipped bit in the text", "a frame in noise", "a fast clock at half the tracking limit", "amplitude 1e-3")]
    for cfg, kw in ((pkg.acars_cfg(keep_bad=True), dict(keep_bad=True)), (pkg.acars_cfg(sync_errors=pkg.ACARS_SYNC_EXACT), dict(sync_errors=0)),
                    (pkg.acars_cfg(hold_timing=True), dict(hold_timing=True)), (pkg.acars_cfg(min_quality=1.0), dict(min_quality=1.0))):
        frames, _ = run_calls(pkg, plane[rows], (NB,), f"settings {kw}", cfg=cfg, model_kw=kw)
        assert (len(frames) == 4) == ("keep_bad" in kw) and (int(frames["row"].max()) < 3) == ("min_quality" in kw)


@gpu
@pytest.mark.parametrize("hold", [False, True])
def test_every_timing_move_from_a_seeded_state(pkg, hold):
    """The rows of tracker_cases() from their seeded blob (set_state) through one batch on the device: u - 1, u + 1, the wraps 0 -> 19
    and 19 -> 0, the slot passed over, the carried bit taken again -- ending nothing, a byte, and the frame, whose record the walk
    stores from there --, the neighbours' tie and the tie of all.  Bits, Q, frames and state equal the model and the twin, and the
    moves are the ones named; under hold_timing none is made."""
    names, st, plane, cases = tracker_cases()
    kw = dict(hold_timing=True) if hold else {}
    frames, after = run_calls(pkg, plane, (1,), f"tracker, hold {hold}", cfg=pkg.acars_cfg(**kw), model_kw=kw, state=st)
    check_tracker_moves(f"device, hold {hold}", cases, st, after, frames, hold=hold)


@gpu
def test_the_walker_follows_a_drifting_clock_through_both_wraps(pkg):
    """the longest frame 150 ppm fast and slow, a batch a call: the state after every call equals the model's, whose u goes 5 .. 0, 19
    and 16 .. 19, 0 .. 2"""
    plane = drift_rows()
    ac = pkg.Acars([1, 1], max_batches=1)
    states, frames, state = [], [], fresh_state(2)
    for b in range(DRIFT_BATCHES):
        blk = np.ascontiguousarray(plane[:, b * WAVE_BATCH:(b + 1) * WAVE_BATCH])
        want = acars_model(blk, state)
        dest = Dest(2, 1, ac.max_frames)
        check(f"drift, batch {b}", acars_call(ac, to_dev(blk), WAVE_BATCH, 1, dest), dest, 2, 1, [1, 1], want)
        state = ac.state().view(want[4].dtype)
        assert state.tobytes() == want[4].tobytes(), f"drift, batch {b}: state"
        states.append(state)
        frames.append(want[0])
    ac.close()
    check_drift("device", states, np.concatenate(frames))


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    ac = pkg.Acars([1, 1, 0], max_batches=nb)
    dest = Dest(rows, nb, rows)
    plane = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_plane=plane.data_ptr(), row_stride=nb * WAVE_BATCH, d_frames=dest.frames.data_ptr(), d_bits=None, d_q=None,
             d_first=dest.row_first.data_ptr(), d_count=dest.count.data_ptr()):
        ac.process_device(d_plane, row_stride, nbatches, d_frames, d_first, d_count, d_bits=d_bits, d_q=d_q, hip_stream=s)

    null, count, short, align = "NULL argument", "nbatches outside 1 .. max_batches", "a row stride is shorter than the call", \
        "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; frame records 8-byte aligned"
    for bad, words in ((dict(nbatches=0), count), (dict(nbatches=nb + 1), count), (dict(d_frames=None), null), (dict(d_plane=None), null),
                       (dict(d_first=None), null), (dict(d_count=None), null), (dict(d_plane=plane.data_ptr() + 4), align),
                       (dict(d_frames=dest.frames.data_ptr() + 4), align), (dict(d_bits=dest.bits.data_ptr() + 2), align),
                       (dict(d_q=dest.q.data_ptr() + 2), align), (dict(row_stride=nb * WAVE_BATCH + 2), align), (dict(row_stride=WAVE_BATCH), short),
                       (dict(d_first=dest.row_first.data_ptr() + 2), align)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID and words in str(e.value), (bad, str(e.value))
    with pytest.raises(pkg.MiError) as e:
        ac.download(s)  # nothing was enqueued yet
    assert "no mi_acars_process_device call" in str(e.value)
    call()
    frames, first, count = ac.download(s)
    assert tuple(count) == (0, 0) and list(first) == [0, 0, 0, 0] and len(frames) == 0
    ac.set_timing(True)
    call()
    assert len(ac.last_launch_ms()) == 5
    ac.close()


@gpu
def test_behind_the_demodulator(pkg):
    """An AM carrier with one burst on it, 1.75 s of u8 I/Q built in numpy, through the demodulator and the stage: the frame sent is the
    frame found, and bits, Q, record and state equal the model over the audio the demodulator returned."""
    dev, chans, iq, nb = e2e_setup(pkg)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
    wo, axc, _, _ = d.process([iq], nb)
    d.close()
    assert (axc[0][0][4:] == ord("*")).all(), "the squelch is not open when the burst begins"
    plane = np.ascontiguousarray(wo[0][:, :nb * WAVE_BATCH])
    d_plane = to_dev(plane)
    ac = pkg.Acars([1], max_batches=nb)
    dest = Dest(1, nb, ac.max_frames)
    got = acars_call(ac, d_plane, nb * WAVE_BATCH, nb, dest)
    want = acars_model(plane)
    check("behind the demodulator", got, dest, 1, nb, [1], want)
    assert ac.state().tobytes() == want[4].tobytes()
    sent = {k: "".join(ch if 0x20 <= ord(ch) <= 0x7E else "." for ch in v) for k, v in E2E_FRAME.items() if isinstance(v, str)}
    assert [pkg.acars_frame_text(f) for f in got[0]] == [sent]
    assert got[0][0]["crc_ok"] == 1 and got[0][0]["end"] == E2E_FRAME["end"] and ac.state().view(pkg.ACARS_STATE_DTYPE)["phase"][0] != FRAME
    ac.close()
