"""The SAME decoder stage on the GPU (mi_same_*, csrc/same.hip) against the numpy restatement in same_model.py and against its host
twin mi_same_plan_host.

Every comparison is bit for bit: bits, Q, messages, prefix, counts and the state blob travel and are compared as bytes.  Every
destination buffer is filled with a sentinel before a call and is longer than the capacity the stage is told; what it must not write
must still hold the sentinel afterwards."""
import numpy as np
import pytest

from same_model import (BURST, HEADER, HEADER_TEXT, MSG_REC, NB, NTAU, NWORDS, WAVE_BATCH, builders, fresh_state, message_fields, modulate, same_model,
                        timing_cases, train, START_CFG, start_unit_rows, tie_cases, tie_start_unit, EOM)
from test_same_model import check_expected, check_start_units, check_timing_moves

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity


class Dest:
    """destination buffers for `cap` messages and the rows * nb blocks' bits and Q, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, nb, cap):
        import torch
        self.cap = cap
        self.msgs = torch.full(((cap + GUARD) * MSG_REC.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.bits = torch.full((rows * nb * NTAU * NWORDS + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.q = torch.full((rows * nb * NTAU + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def same_call(sa, d_plane, row_stride, nb, dest, stream=None, scratch=False):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    sa.process_device(d_plane.data_ptr(), row_stride, nb, dest.msgs.data_ptr(), dest.row_first.data_ptr(), dest.count.data_ptr(),
                      d_bits=None if scratch else dest.bits.data_ptr(), d_q=None if scratch else dest.q.data_ptr(), hip_stream=s)
    return sa.download(s)


def check(what, got, dest, rows, nb, en, want, scratch=False):
    msgs, row_first, count = got
    w_msgs, w_bits, w_q, w_first, _ = want
    total, k = len(w_msgs), min(len(w_msgs), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, w_first), f"{what}: row_first_message"
    assert msgs.tobytes() == w_msgs[:k].tobytes(), f"{what}: messages\n{msgs}\nwant\n{w_msgs[:k]}"
    d_msgs = dest.msgs.cpu().numpy()
    assert d_msgs[:k * MSG_REC.itemsize].tobytes() == w_msgs[:k].tobytes(), f"{what}: messages on the device"
    assert (d_msgs[k * MSG_REC.itemsize:] == SENT_BYTE).all(), f"{what}: something was written behind message {k}"
    bits, q = dest.bits.cpu().numpy().view(np.uint32), dest.q.cpu().numpy()
    if scratch:
        assert (bits == 0xA5A5A5A5).all() and (q == SENT32).all(), f"{what}: bits or Q written though the call gave none"
    else:
        on = np.asarray(en, bool)
        g_bits, g_q = bits[:rows * nb * NTAU * NWORDS].reshape(rows, nb, NTAU, NWORDS), q[:rows * nb * NTAU].view(np.float32).reshape(rows, nb, NTAU)
        bad = np.argwhere(g_bits[on] != w_bits[on])
        assert not len(bad), f"{what}: bits, first at {bad[:3]}"
        assert g_q[on].tobytes() == w_q[on].tobytes(), f"{what}: Q, first at {np.argwhere(g_q[on].view(np.uint32) != w_q[on].view(np.uint32))[:3]}"
        assert (g_bits[~on] == 0xA5A5A5A5).all() and (bits[rows * nb * NTAU * NWORDS:] == 0xA5A5A5A5).all() and (q[rows * nb * NTAU:] == SENT32).all(), \
            f"{what}: bits or Q that must not be written"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def run_calls(pkg, plane, cuts, what, cfg=None, model_kw=None, masks=None, cap=0, pads=(0,), stream=None, twin_at=None, state=None, scratch=False):
    """One handle over consecutive calls of the lengths `cuts`, call i over a plane laid out for pads[i % len] more batches than the
    call: bits, Q, messages and the state after every call against the model, and the host twin run from the same blob against both.
    masks: the enabled rows of each call (set_rows in between).  twin_at: that call is made by the host twin from the device's state
    blob, whose state goes back to the device.  Returns (messages of all calls, state)."""
    import torch
    rows = plane.shape[0]
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    sa = pkg.Same(masks[0], max_batches=max(cuts), cfg=cfg, max_messages=cap)
    if state is None:
        state = fresh_state(rows)
    else:
        sa.set_state(state)
    done, all_msgs = 0, []
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            sa.set_rows(en)
        lay = n + pads[i % len(pads)]
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.25))  # behind the call: a level that must not be read
        w[:, :n * WAVE_BATCH] = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = same_model(w[:, :n * WAVE_BATCH], state, en, **(model_kw or {}))
        before = sa.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin = pkg.same_plan_host(en, w, cfg, before, nbatches=n)
        assert twin[0].tobytes() == want[0].tobytes() and twin[1].tobytes() == want[1].tobytes() and twin[2].tobytes() == want[2].tobytes() and \
            twin[5].tobytes() == want[4].tobytes(), f"{what}, call {i}: the twin and the model differ"
        if i == twin_at:
            sa.set_state(twin[5])
        else:
            room = cap or rows * pkg.same_max_messages(max(cuts))
            dest = Dest(rows, n, room)
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_w = to_dev(w)
            else:
                d_w = to_dev(w)
            got = same_call(sa, d_w, lay * WAVE_BATCH, n, dest, None if stream is None else stream.cuda_stream, scratch)
            check(f"{what}, call {i} at batch {done}", got, dest, rows, n, en, want, scratch)
        assert sa.state().tobytes() == want[4].tobytes(), f"{what}, call {i}: state blob after"
        state, done = want[4], done + n
        all_msgs.append(want[0])
    sa.close()
    return np.concatenate(all_msgs), state


def tiled(plane, rows):
    return plane[np.arange(rows) % plane.shape[0]]


def key(msgs):
    return sorted((int(m["row"]), int(m["batch"]), int(m["unit"]), int(m["nbursts"]), bytes(m["bytes"])) for m in msgs)


CUTS = (1, 4, 1, 4, 48, 6)  # 64 batches: calls of 1, 4 and 48


@gpu
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_device_equals_model_and_twin(pkg, rows):
    """Calls of 1, 4 and 48 batches on one handle: over the full alert's row at 1 row, over it and its four neighbours at 5, and over
    every builder's row, tiled, at 70 -- 70 x 48 blocks in one launch; bursts that begin in one call and end in another; bits that
    begin in the carried samples; every message the builders expect."""
    names, plane, expect = builders()
    plane = tiled(plane, rows) if rows == 70 else plane[:rows]
    msgs, state = run_calls(pkg, plane, CUTS, f"{rows} rows")
    whole = same_model(plane)
    assert key(msgs) == key(whole[0]) and state.tobytes() == whole[4].tobytes() and state["batch"][0] == NB
    check_expected(names[:min(rows, len(names))], msgs, expect)


@gpu
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg):
    """rows 1 and 3 sit the second of five calls out -- no record, every byte of their state stays --; the third call, which begins
    in the middle of the first burst, or the fourth, which begins between bursts, is made by the host twin from the device's blob and
    handed back with set_state.  The blob the handle starts from has a batch counter about to wrap.  Impossible states are refused."""
    names, plane, _ = builders()
    masks = [np.ones(5, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(5, np.uint8), np.ones(5, np.uint8), np.ones(5, np.uint8)]
    st = fresh_state(5)
    st["batch"] = 0xFFFFFFFD
    st["x"][:] = np.random.default_rng(9).normal(0, 0.05, (5, 30)).astype(np.float32)
    for twin_at, mid in ((2, "in a burst"), (3, "between bursts")):
        sa_state = st.copy()
        msgs, state = run_calls(pkg, plane[:5], (3, 2, 5, 9, 21), f"set_rows, the twin {mid}", masks=masks, twin_at=twin_at, state=sa_state)
        assert len(msgs) >= 3 and state["batch"][0] == 37
    mid_state = same_model(plane[:5, :5 * WAVE_BATCH], st)[4]
    assert (mid_state["phase"][[0, 2, 4]] == BURST).all(), "the third call begins inside a burst"
    sa = pkg.Same([1], max_batches=2)
    for field, value in (("phase", 2), ("u", 1), ("zero", 1), ("grid", 8), ("an", 3)):
        bad = fresh_state(1)
        bad[0][field] = value
        with pytest.raises(pkg.MiError) as e:
            sa.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID and "state" in str(e.value)
    sa.close()


@gpu
@pytest.mark.parametrize("scratch", [False, True])
def test_capped_messages_padded_unequal_strides_and_a_side_stream(pkg, scratch):
    """a message buffer shorter than the call's messages is left untouched beyond its cap, with the bits and Q in the caller's buffers
    and in the handle's; the planes are laid out for three and for one batch more than the call; everything is enqueued on a side
    stream with no synchronisation before download"""
    import torch
    plane = builders()[1][:12]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    msgs, _ = run_calls(pkg, plane, (30, 18), f"cap 2, scratch {scratch}", cap=2, pads=(3, 1), stream=side, scratch=scratch)
    assert len(msgs) > 4


@gpu
def test_settings_on_the_device(pkg):
    """an exact sync, a short gap, hold_timing, a quality floor, a space gain and max_bad, each against the model"""
    names, plane, _ = builders()
    rows = [names.index(n) for n in ("two bursts only", "a full alert in noise", "+200 ppm", "amplitude 1e-3", "a burst cut off by silence")]
    for cfg, kw in ((pkg.same_cfg(sync_errors=pkg.SAME_SYNC_EXACT), dict(sync_errors=0)), (pkg.same_cfg(gap_batches=3), dict(gap_batches=3)),
                    (pkg.same_cfg(hold_timing=True), dict(hold_timing=True)), (pkg.same_cfg(min_quality=1.0), dict(min_quality=1.0)),
                    (pkg.same_cfg(space_gain=1.5, max_bad=2), dict(space_gain=1.5, max_bad=2))):
        msgs, _ = run_calls(pkg, plane[rows], (NB,), f"settings {kw}", cfg=cfg, model_kw=kw)
        assert (3 not in msgs["row"]) == ("min_quality" in kw), kw


@gpu
@pytest.mark.parametrize("hold", [False, True])
def test_every_timing_move_from_a_seeded_state(pkg, hold):
    """The rows of timing_cases() from their seeded blob (set_state) through one batch on the device: u - 1, u + 1, the wraps 0 -> 15
    and 15 -> 0 with the carried bit taken again and the index passed over.  Bits, Q and state equal the model and the twin, and the
    moves are the ones named; under hold_timing none is made."""
    names, st, plane, moves = timing_cases()
    kw = dict(max_bad=16, hold_timing=hold)
    _, after = run_calls(pkg, plane, (1,), f"timing, hold {hold}", cfg=pkg.same_cfg(**kw), model_kw=kw, state=st)
    check_timing_moves(names, moves, after, hold)


@gpu
def test_a_burst_at_every_start_unit_modulo_48_on_the_device(pkg):
    """the 48 rows of start_unit_rows(), calls of 3 and 7 batches: bits, Q, messages and state equal the model and the twin, and every
    row's header comes out as sent"""
    msgs, _ = run_calls(pkg, start_unit_rows(), (3, 7), "start units", cfg=pkg.same_cfg(**START_CFG), model_kw=START_CFG)
    check_start_units(msgs[np.argsort(msgs["row"], kind="stable")])


@gpu
def test_the_choice_among_hits_on_the_device(pkg):
    """tie_cases() from their seeded blobs: the wave's choice equals the model's and the twin's"""
    for name, st, plane, settings, u in tie_cases():
        kw = settings(same_model(plane, st)[2][0, 0])
        _, after = run_calls(pkg, plane, (1,), name, cfg=pkg.same_cfg(**kw), model_kw=kw, state=st)
        assert after["an"][0] == 1 and after["akind"][0] == EOM and after["astart_unit"][0] == tie_start_unit(u), name


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    sa = pkg.Same([1, 1, 0], max_batches=nb)
    dest = Dest(rows, nb, rows)
    plane = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_plane=plane.data_ptr(), row_stride=nb * WAVE_BATCH, d_msgs=dest.msgs.data_ptr(), d_bits=None, d_q=None,
             d_first=dest.row_first.data_ptr(), d_count=dest.count.data_ptr()):
        sa.process_device(d_plane, row_stride, nbatches, d_msgs, d_first, d_count, d_bits=d_bits, d_q=d_q, hip_stream=s)

    null, count, short, align = "NULL argument", "nbatches outside 1 .. max_batches", "a row stride is shorter than the call", \
        "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; message records 8-byte aligned"
    for bad, words in ((dict(nbatches=0), count), (dict(nbatches=nb + 1), count), (dict(d_msgs=None), null), (dict(d_plane=None), null),
                       (dict(d_first=None), null), (dict(d_count=None), null), (dict(d_plane=plane.data_ptr() + 4), align),
                       (dict(d_msgs=dest.msgs.data_ptr() + 4), align), (dict(d_bits=dest.bits.data_ptr() + 2), align),
                       (dict(d_q=dest.q.data_ptr() + 2), align), (dict(row_stride=nb * WAVE_BATCH + 2), align), (dict(row_stride=WAVE_BATCH), short),
                       (dict(d_first=dest.row_first.data_ptr() + 2), align)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID and words in str(e.value), (bad, str(e.value))
    with pytest.raises(pkg.MiError) as e:
        sa.download(s)  # nothing was enqueued yet
    assert "no mi_same_process_device call" in str(e.value)
    call()
    msgs, first, count = sa.download(s)
    assert tuple(count) == (0, 0) and list(first) == [0, 0, 0, 0] and len(msgs) == 0
    sa.set_timing(True)
    call()
    assert len(sa.last_launch_ms()) == 5
    sa.close()


E2E_BATCHES = 36


def e2e_setup(pkg):
    """One stream, one NFM channel five bins above the centre at fft 512, 2.56 Msps: a carrier frequency-modulated (3 kHz peak) by the
    model's three header bursts, which begin half a second in: (dev, chans, iq uint8, batches)."""
    from common import AGC_EXTRA
    rate, centre = 2560000, 162000000
    dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9)
    chans = [pkg.channel_cfg(centre + 25000, modulation=pkg.MOD_NFM)]
    hop = rate // 16000
    n_audio = E2E_BATCHES * WAVE_BATCH + AGC_EXTRA + 8
    audio = modulate(n_audio, train([HEADER_TEXT] * 3, start=25 * 8000 + 11, amp=0.6)[0]).astype(np.float64)
    n = n_audio * hop
    dphi = 2.0 * np.pi * (25000.0 + 3000.0 * np.repeat(audio, hop)) / rate
    z = 30.0 * np.exp(1j * np.cumsum(dphi)).astype(np.complex64)
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    iq += np.random.default_rng(72).normal(0.0, 1.5, 2 * n).astype(np.float32)
    return dev, chans, np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8), E2E_BATCHES


@gpu
def test_behind_the_demodulator(pkg):
    """An NFM carrier modulated by the model's three header bursts, 4.5 s of u8 I/Q, through the demodulator and the stage: the header
    sent is the header found, voted, with fields_ok, and bits, Q, record and state equal the model over the audio the demodulator
    returned."""
    dev, chans, iq, nb = e2e_setup(pkg)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
    wo, axc, _, _ = d.process([iq], nb)
    d.close()
    plane = np.ascontiguousarray(wo[0][:, :nb * WAVE_BATCH])
    d_plane = to_dev(plane)
    sa = pkg.Same([1], max_batches=nb)
    dest = Dest(1, nb, sa.max_messages)
    got = same_call(sa, d_plane, nb * WAVE_BATCH, nb, dest)
    want = same_model(plane)
    check("behind the demodulator", got, dest, 1, nb, [1], want)
    assert sa.state().tobytes() == want[4].tobytes()
    sa.close()
    assert len(got[0]) == 1, f"squelch flags {bytes(axc[0][0])}"
    m = got[0][0]
    assert (m["kind"], m["nbursts"], m["voted"], m["fields_ok"]) == (HEADER, 3, 1, 1) and bytes(m["bytes"][:m["nbytes"]]) == HEADER_TEXT
    assert pkg.same_message_text(m) == message_fields(HEADER_TEXT)
