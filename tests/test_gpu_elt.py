"""The ELT detector stage on the GPU (mi_elt_*, csrc/elt.hip) against the numpy restatement in elt_model.py and against its host twin
mi_elt_plan_host.

Every comparison is bit for bit: frame records, events, prefix, counts and the state blob travel and are compared as bytes -- the order
of the energy's sum, the recurrence, the tie rule and the walker's rules are part of the definition.  Every destination buffer is filled
with a sentinel before a call and is longer than the capacity the stage is told; what it must not write must still hold the sentinel
afterwards."""
import numpy as np
import pytest

from elt_model import (BOUND_NB, DOWN, END, EVENT_REC, FRAME_REC, FRAMES, HISTORY, HOP, NB, ONSET, WAVE_BATCH, bound_cases, carried_edge_state, e2e_setup, elt_model, fresh_state,
                       refused_states, stacked, start_offsets, state_of)
from test_elt_model import CAP, bound_plane, capacity_rows

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity


class Dest:
    """destination buffers for `cap` events and rows * 25 nb frame records, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, nb, cap, frames=True):
        import torch
        self.cap = cap
        self.events = torch.full(((cap + GUARD) * EVENT_REC.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.frames = torch.full(((rows * FRAMES * nb + GUARD) * FRAME_REC.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda") if frames else None
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def elt_call(el, d_plane, row_stride, nb, dest, stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    el.process_device(d_plane.data_ptr(), row_stride, nb, dest.events.data_ptr(), dest.row_first.data_ptr(), dest.count.data_ptr(),
                      d_frames=None if dest.frames is None else dest.frames.data_ptr(), hip_stream=s)
    return el.download(s)


def check(what, got, dest, rows, nb, en, want):
    events, fr, row_first, count = got
    w_events, w_fr, w_first, _ = want
    total, k = len(w_events), min(len(w_events), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, w_first), f"{what}: row_first_event"
    assert events.tobytes() == w_events[:k].tobytes(), f"{what}: events\n{events}\nwant\n{w_events[:k]}"
    d_events = dest.events.cpu().numpy()
    assert d_events[:k * 32].tobytes() == w_events[:k].tobytes(), f"{what}: events on the device"
    assert (d_events[k * 32:] == SENT_BYTE).all(), f"{what}: something was written behind event {k}"
    if dest.frames is None:
        assert fr is None
    else:
        on = np.asarray(en, bool)
        bad = np.argwhere(fr[on].view(np.uint8).reshape(-1, FRAMES * nb, 16) != w_fr[on].view(np.uint8).reshape(-1, FRAMES * nb, 16))
        assert fr[on].tobytes() == w_fr[on].tobytes(), f"{what}: frame records, first at {bad[:3]}"
        d_fr = dest.frames.cpu().numpy()
        assert (fr[~on].view(np.uint8) == SENT_BYTE).all() and (d_fr[rows * FRAMES * nb * 16:] == SENT_BYTE).all(), f"{what}: frames that must not be written"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def run_calls(pkg, plane, cuts, what, cfg=None, model_kw=None, masks=None, cap=0, frames=True, pads=(0,), stream=None, twin_at=(), state=None):
    """One handle over consecutive calls of the lengths `cuts`, call i over a plane laid out for pads[i % len] more batches than the call:
    frame records, events and the state after every call against the model, and the host twin run from the same blob against both.
    masks: the enabled rows of each call (set_rows in between).  twin_at: those calls are made by the host twin from the device's state
    blob, whose state goes back to the device.  Returns (events of all calls, state)."""
    import torch
    rows = plane.shape[0]
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    el = pkg.Elt(masks[0], max_batches=max(cuts), cfg=cfg, max_events=cap)
    if state is None:
        state = fresh_state(rows)
    else:
        el.set_state(state)
    done, all_events = 0, []
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            el.set_rows(en)
        lay = n + pads[i % len(pads)]
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.25))  # behind the call: a level that would change every E it reached
        w[:, :n * WAVE_BATCH] = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = elt_model(w[:, :n * WAVE_BATCH], state, en, **(model_kw or {}))
        before = el.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin = pkg.elt_plan_host(en, w, cfg, before, nbatches=n)
        on = np.asarray(en, bool)
        assert twin[0].tobytes() == want[0].tobytes() and twin[1][on].tobytes() == want[1][on].tobytes() and twin[4].tobytes() == want[3].tobytes(), \
            f"{what}, call {i}: the twin and the model differ"
        if i in twin_at:
            el.set_state(twin[4])
        else:
            room = cap or rows * pkg.elt_max_events(max(cuts), cfg)
            dest = Dest(rows, n, room, frames)
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_w = to_dev(w)
            else:
                d_w = to_dev(w)
            got = elt_call(el, d_w, lay * WAVE_BATCH, n, dest, None if stream is None else stream.cuda_stream)
            check(f"{what}, call {i} at batch {done}", got, dest, rows, n, en, want)
        assert el.state().tobytes() == want[3].tobytes(), f"{what}, call {i}: state blob after"
        state, done = want[3], done + n
        all_events.append(want[0])
    el.close()
    return np.concatenate(all_events), state


def tiled(plane, rows):
    return plane[np.arange(rows) % plane.shape[0]]


@gpu
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_device_equals_model_and_twin(pkg, rows):
    """Calls of 1 and 4 batches (and the rest of the 48) on one handle over the builders' rows: one block, a few, and -- at 70 rows, the
    builders tiled -- many; sweeps and chains that begin in one call and end in another; frames that begin in the carried samples; one
    sounding block among closed ones (the lone samples), silence, -0.0 and subnormals."""
    plane = stacked()[1]
    plane = tiled(plane, rows) if rows == 70 else plane[10:10 + rows]
    events, state = run_calls(pkg, plane, (1, 4, 1, 4, 38), f"{rows} rows")
    assert len(events) >= 2 * (rows // 5 + 1) and state["frame"][0] == FRAMES * NB


@gpu
@pytest.mark.parametrize("cuts", [(48,), (5, 43), (1,) * 48])
def test_48_batches_and_their_cuts(pkg, cuts):
    """every builder in one launch of 48 batches, the same cut in two, and forty-eight calls of one batch: every cut raises the same
    alarms and leaves the same state"""
    plane = stacked()[1]
    events, state = run_calls(pkg, plane, cuts, f"cuts {cuts[:2]}")
    whole = elt_model(plane)
    key = lambda es: sorted((int(e["row"]), int(e["seq"]), int(e["kind"]), int(e["frame"]), int(e["sweeps"])) for e in es)  # noqa: E731
    assert key(events) == key(whole[0]) and len(events) >= 15
    assert state.tobytes() == whole[3].tobytes()


@gpu
def test_the_80_start_offsets_and_the_capacity_bound(pkg):
    """a beacon beginning at every sample offset modulo 80, a row each; and the row that emits END, ONSET, END in one call of two
    batches, which is all its slots"""
    events, _ = run_calls(pkg, start_offsets(), (7, 13), "start offsets")
    assert len(events) == HOP and (events["kind"] == ONSET).all()
    plane, cuts = capacity_rows()
    events, _ = run_calls(pkg, plane, cuts, "capacity", cfg=pkg.elt_cfg(**CAP), model_kw=CAP)
    assert list(events["kind"]) == [ONSET, END, ONSET, END] and list(events["batch"][1:]) == [0, 1, 1]


@gpu
@pytest.mark.parametrize("case", bound_cases(), ids=[c[0] for c in bound_cases()])
def test_both_sides_of_every_settings_bound(pkg, case):
    """the walker on the device on audio whose sweeps sit exactly on a setting and one beyond it (test_elt_model.py asserts what the
    model measures for each signal): device = model = twin in every byte, and what must and must not be raised"""
    name, signal, kw, kinds, first_frame = case
    events, _ = run_calls(pkg, bound_plane(signal), (7, BOUND_NB - 7), name, cfg=pkg.elt_cfg(**kw), model_kw=kw)
    assert [int(e["kind"]) for e in events] == kinds and (first_frame is None or events[0]["first_frame"] == first_frame), events


@gpu
def test_one_carried_sample_at_either_end_of_the_lead(pkg):
    """one batch of silence behind a state with a single carried sample: the newest one, which frames 0 .. 2 see, and the oldest that
    weighs, which frame 0 sees; then the three oldest, which no frame may see"""
    zero = np.zeros((2, WAVE_BATCH), np.float32)
    edge = carried_edge_state()
    want = elt_model(zero, edge)
    assert list(np.flatnonzero(want[1]["energy"][0])) == [0, 1, 2] and list(np.flatnonzero(want[1]["energy"][1])) == [0]
    run_calls(pkg, zero, (1,), "carried edges", state=edge)
    edge["x"][1, 3], edge["x"][1, :3] = 0.0, 0.5
    assert not elt_model(zero, edge)[1]["energy"][1].any()
    run_calls(pkg, zero, (1,), "carried samples that must not count", state=edge)


@gpu
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg):
    """rows 1 and 3 sit the second call out -- no record, every byte of their state stays, carried samples included --; three calls are
    made by the host twin from the device's blob and handed back with set_state: one that ends mid-sweep, one that ends between sweeps
    (behind six sweeps then silence) and one while alarmed; the device goes on from each.  The blob the handle starts from has a frame
    counter about to wrap.  States the walker cannot be in are refused."""
    plane = stacked()[1][[1, 2, 10, 11, 12]]
    ones = np.ones(5, np.uint8)
    masks = [ones, np.array([1, 0, 1, 0, 1], np.uint8), ones, ones, ones, ones, ones]
    st = fresh_state(5)
    st["frame"], st["seq"] = 0xFFFFFF80, 3
    st["x"][:] = np.random.default_rng(9).normal(0, 0.05, (5, HISTORY)).astype(np.float32)
    cuts = (5, 6, 3, 6, 7, 4, 17)
    want = np.cumsum(cuts)
    events, state = run_calls(pkg, plane, cuts, "set_rows", masks=masks, twin_at=(2, 4, 5), state=st)
    assert len(events) >= 6 and state["frame"][0] == (0xFFFFFF80 + FRAMES * NB) & 0xFFFFFFFF and want[-1] == NB
    el = pkg.Elt([1], max_batches=2)
    good, bad = refused_states()
    for name, fields in good:
        el.set_state(state_of(1, 0, fields))
    for name, fields in bad:
        with pytest.raises(pkg.MiError) as e:
            el.set_state(state_of(1, 0, fields))
        assert e.value.code == pkg.MI_ERR_INVALID and "ELT stage state" in str(e.value), name
    el.close()


@gpu
@pytest.mark.parametrize("frames", [True, False])
def test_capped_events_padded_unequal_strides_and_a_side_stream(pkg, frames):
    """an event buffer shorter than the call's events is left untouched beyond its cap, with and without d_frames; the planes are laid
    out for three and for one batch more than the call; everything is enqueued on a side stream with no synchronisation before
    download"""
    import torch
    plane = stacked()[1][:14]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    events, _ = run_calls(pkg, plane, (21, 27), f"cap 3, frames {frames}", cap=3, frames=frames, pads=(3, 1), stream=side)
    assert len(events) > 3


@gpu
def test_more_blocks_than_a_grid_s_first_wave_of_workgroups(pkg):
    """2100 rows of 2 batches: 4200 blocks, more than the device holds at once (256 CUs x 16), most of them closed; every 16th row sounds"""
    base = stacked()[1]
    rows = 2100
    plane = np.zeros((rows, 2 * WAVE_BATCH), np.float32)
    plane[::16] = tiled(base, len(range(0, rows, 16)))[:, 6 * WAVE_BATCH:8 * WAVE_BATCH]
    run_calls(pkg, plane, (2,), "2100 rows")


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    el = pkg.Elt([1, 1, 0], max_batches=nb)
    dest = Dest(rows, nb, rows * 3)
    plane = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_plane=plane.data_ptr(), row_stride=nb * WAVE_BATCH, d_events=dest.events.data_ptr(), d_frames=None, d_first=dest.row_first.data_ptr(),
             d_count=dest.count.data_ptr()):
        el.process_device(d_plane, row_stride, nbatches, d_events, d_first, d_count, d_frames=d_frames, hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_events=None), dict(d_plane=None), dict(d_first=None), dict(d_count=None),
                dict(d_plane=plane.data_ptr() + 4), dict(d_events=dest.events.data_ptr() + 4), dict(d_frames=dest.frames.data_ptr() + 4),
                dict(row_stride=nb * WAVE_BATCH + 2), dict(row_stride=WAVE_BATCH), dict(d_first=dest.row_first.data_ptr() + 2)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        el.download(s)  # nothing was enqueued yet
    call()
    events, fr, first, count = el.download(s)
    assert tuple(count) == (0, 0) and list(first) == [0, 0, 0, 0] and fr is None and len(events) == 0
    with pytest.raises(pkg.MiError) as e:  # frames asked for after a call that stored none
        el._nframes = FRAMES * nb
        el.download(s)
    assert e.value.code == pkg.MI_ERR_INVALID
    el.set_timing(True)
    call()
    assert len(el.last_launch_ms()) == 5
    el.close()


@gpu
def test_behind_the_demodulator(pkg):
    """An AM carrier modulated 80 % by the 3 Hz beacon, 4 s of u8 I/Q built in numpy (the device generator cannot modulate by audio),
    through the demodulator and the stage: one ONSET, downward, within the first 24 batches; records and state equal the model over the
    audio the demodulator returned."""
    dev, chans, iq, nb = e2e_setup(pkg)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
    wo, axc, _, _ = d.process([iq], nb)
    d.close()
    print("flags:", bytes(axc[0][0]).decode())
    plane = np.ascontiguousarray(wo[0][:, :nb * WAVE_BATCH])
    d_plane = to_dev(plane)
    el = pkg.Elt([1], max_batches=nb)
    dest = Dest(1, nb, el.max_events)
    got = elt_call(el, d_plane, nb * WAVE_BATCH, nb, dest)
    want = elt_model(plane)
    check("behind the demodulator", got, dest, 1, nb, [1], want)
    assert el.state().tobytes() == want[3].tobytes()
    print([pkg.elt_event_text(e) for e in got[0]], "tonal share", (got[1]["bin"] != 0xFF).mean())
    assert list(got[0]["kind"]) == [ONSET] and got[0]["dir"][0] == DOWN and got[0]["batch"][0] < 24
    el.close()
