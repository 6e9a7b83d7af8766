"""The pager decoder stage on the GPU (mi_pocsag_*, csrc/pocsag.hip) against the numpy restatement in pocsag_model.py and against its
host twin mi_pocsag_plan_host.

Every comparison is bit for bit: bits, Q, messages, prefix, counts and the state blob travel and are compared as bytes.  Every
destination buffer is filled with a sentinel before a call and is longer than the capacity the stage is told; what it must not write
must still hold the sentinel afterwards."""
import numpy as np
import pytest

import pocsag_model as m
from pocsag_model import GEOM, MESSAGE, WAVE_BATCH, fresh_state, pocsag_model
from test_pocsag_model import builders, capacity_case

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity


class Dest:
    """destination buffers for `cap` messages and the rows * nb blocks' bits and Q, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, nb, cap, baud):
        import torch
        _, _, H, _, W = GEOM[baud]
        self.cap, self.block, self.lanes = cap, 2 * H * W, 2 * H
        self.messages = torch.full(((cap + GUARD) * MESSAGE.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.bits = torch.full((rows * nb * self.block + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.q = torch.full((rows * nb * self.lanes + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def pg_call(pg, d_plane, row_stride, nb, dest, stream=None, scratch=False):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    pg.process_device(d_plane.data_ptr(), row_stride, nb, dest.messages.data_ptr(), dest.row_first.data_ptr(), dest.count.data_ptr(),
                      d_bits=None if scratch else dest.bits.data_ptr(), d_q=None if scratch else dest.q.data_ptr(), hip_stream=s)
    return pg.download(s)


def check(what, got, dest, rows, nb, en, want, scratch=False):
    msgs, row_first, count = got
    w_msgs, w_bits, w_q, w_first, _ = want
    total, k = len(w_msgs), min(len(w_msgs), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, w_first), f"{what}: row_first_message"
    assert msgs.tobytes() == w_msgs[:k].tobytes(), f"{what}: messages\n{msgs[['row', 'batch', 'twelfth', 'address', 'nwords']]}\nwant\n{w_msgs[:k][['row', 'batch', 'twelfth', 'address', 'nwords']]}"
    d_msgs = dest.messages.cpu().numpy()
    assert d_msgs[:k * MESSAGE.itemsize].tobytes() == w_msgs[:k].tobytes(), f"{what}: messages on the device"
    assert (d_msgs[k * MESSAGE.itemsize:] == SENT_BYTE).all(), f"{what}: something was written behind message {k}"
    bits, q = dest.bits.cpu().numpy().view(np.uint32), dest.q.cpu().numpy().view(np.uint32)
    if scratch:
        assert (bits == 0xA5A5A5A5).all() and (q == 0xA5A5A5A5).all(), f"{what}: bits or Q written though the call gave none"
    else:
        on = np.asarray(en, bool)
        g_bits, g_q = bits[:rows * nb * dest.block].reshape(w_bits.shape), q[:rows * nb * dest.lanes].reshape(w_q.shape)
        bad = np.argwhere(g_bits[on] != w_bits[on])
        assert not len(bad), f"{what}: bits, first at {bad[:3]}"
        bad = np.argwhere(g_q[on] != w_q[on].view(np.uint32))
        assert not len(bad), f"{what}: Q, first at {bad[:3]}"
        assert (g_bits[~on] == 0xA5A5A5A5).all() and (g_q[~on] == 0xA5A5A5A5).all() and (bits[rows * nb * dest.block:] == 0xA5A5A5A5).all() and \
            (q[rows * nb * dest.lanes:] == 0xA5A5A5A5).all(), f"{what}: bits or Q that must not be written"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def run_calls(pkg, plane, cuts, what, baud=1200, masks=None, cap=0, pads=(0,), stream=None, twin_at=None, state=None, scratch=False):
    """One handle over consecutive calls of the lengths `cuts`, call i over a plane laid out for pads[i % len] more batches than the
    call: bits, Q, messages and the state after every call against the model, and the host twin run from the same blob against both.
    masks: the enabled rows of each call (set_rows in between).  twin_at: that call is made by the host twin from the device's state
    blob, whose state goes back to the device.  Returns (messages of all calls, state)."""
    import torch
    rows = plane.shape[0]
    cfg = pkg.pocsag_cfg(baud=baud)
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    pg = pkg.Pocsag(masks[0], max_batches=max(cuts), cfg=cfg, max_messages=cap)
    if state is None:
        state = fresh_state(rows)
    else:
        pg.set_state(state)
    done, all_msgs = 0, []
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            pg.set_rows(en)
        lay = n + pads[i % len(pads)]
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.25))  # behind the call: a level that must not be read
        w[:, :n * WAVE_BATCH] = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = pocsag_model(w[:, :n * WAVE_BATCH], state, en, baud=baud)
        before = pg.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin = pkg.pocsag_plan_host(en, w, cfg, before, nbatches=n)
        assert twin[0].tobytes() == want[0].tobytes() and twin[1].tobytes() == want[1].tobytes() and twin[2].tobytes() == want[2].tobytes() and \
            twin[5].tobytes() == want[4].tobytes(), f"{what}, call {i}: the twin and the model differ"
        if i == twin_at:
            pg.set_state(twin[5])
        else:
            room = cap or rows * pkg.pocsag_max_messages(max(cuts), baud)
            dest = Dest(rows, n, room, baud)
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_w = to_dev(w)
            else:
                d_w = to_dev(w)
            got = pg_call(pg, d_w, lay * WAVE_BATCH, n, dest, None if stream is None else stream.cuda_stream, scratch)
            check(f"{what}, call {i} at batch {done}", got, dest, rows, n, en, want, scratch)
        assert pg.state().tobytes() == want[4].tobytes(), f"{what}, call {i}: state blob after"
        state, done = want[4], done + n
        all_msgs.append(want[0])
    pg.close()
    return np.concatenate(all_msgs), state


def tiled(plane, rows):
    return plane[np.arange(rows) % plane.shape[0]]


@gpu
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_device_equals_model_and_twin(pkg, rows):
    """1200 baud, calls of 1, 2 and 3 batches on one handle over the first 6 batches: one block, a few, many; messages that begin in
    one call and end in another; bits that begin in the carried samples"""
    _, plane, _ = builders(1200)
    plane = tiled(plane, rows) if rows == 70 else plane[:rows]
    msgs, state = run_calls(pkg, plane, (1, 2, 3), f"{rows} rows")
    assert len(msgs) >= (rows + 1) // 2 and state["batch"][0] == 6


@gpu
@pytest.mark.parametrize("baud,cuts", [(512, (1, 4, 7, 16)), (2400, (1, 2, 3))])
def test_the_other_bauds(pkg, baud, cuts):
    names, plane, sent = builders(baud)
    msgs, _ = run_calls(pkg, plane[:6], cuts, f"{baud} baud", baud=baud)
    assert [sorted(m.found(msgs, r)) for r in range(6)] == [sorted(x) for x in sent[:6]]


@gpu
def test_48_batches_in_one_call_at_512_baud(pkg):
    """a full preamble of 576 bits and two groups, the long page crossing from the first into the second; a third group of IDLE
    closes it, and the silence behind (from batch 35 on) fails the next SYNC: the row is idle again at the end"""
    x, sent = m.full_preamble_512(48)
    msgs, state = run_calls(pkg, x.astype(np.float32)[None], (48,), "48 batches", baud=512)
    assert m.found(msgs) == sent and state["phase"][0] == m.IDLE and state["batch"][0] == 48 and msgs[0]["end_batch"] > 26


@gpu
def test_set_rows_and_the_state_through_the_twin(pkg):
    """rows 1 and 3 sit the second of four calls out -- no record, every byte of their state stays --; the third call is made by the
    host twin from the device's blob in the middle of the messages, and handed back with set_state; the fourth goes on from it.
    Impossible blobs are refused."""
    _, plane, _ = builders(1200)
    masks = [np.ones(5, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(5, np.uint8), np.ones(5, np.uint8)]
    st = fresh_state(5)
    st["x"][:] = np.random.default_rng(9).normal(0, 0.05, (5, 34)).astype(np.float32)
    msgs, state = run_calls(pkg, plane[[5, 0, 1, 3, 4]], (1, 1, 1, 5), "set_rows", masks=masks, twin_at=2, state=st)
    assert len(msgs) >= 3 and state["batch"][0] == 8 and state["batch"][1] == 7
    pg = pkg.Pocsag([1], max_batches=2)
    for field, value, words in (("zero", 1, "the zero field is not 0"), ("phase", 2, "an unknown walker phase"), ("lane", 3, "an idle row with a walker field")):
        bad = fresh_state(1)
        bad[field] = value
        with pytest.raises(pkg.MiError) as e:
            pg.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID and "pager stage state: " in str(e.value) and words in str(e.value), field
    bad = fresh_state(1)
    bad["phase"], bad["lane"], bad["lane_sync"] = 1, 20, 20  # a lane of 512 baud on a handle of 1200
    with pytest.raises(pkg.MiError) as e:
        pg.set_state(bad)
    assert "a lane the baud does not have" in str(e.value)
    pg.close()


@gpu
@pytest.mark.parametrize("scratch", [False, True])
def test_capped_messages_padded_unequal_strides_and_a_side_stream(pkg, scratch):
    """a message buffer shorter than the call's messages is left untouched beyond its cap, with bits and Q in the caller's buffers
    and in the handle's; the planes are laid out for three and for one batch more than the call; everything is enqueued on a side
    stream with no synchronisation before download"""
    import torch
    plane = builders(2400)[1][:8]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    msgs, _ = run_calls(pkg, plane, (3, 5), f"cap 2, scratch {scratch}", baud=2400, cap=2, pads=(3, 1), stream=side, scratch=scratch)
    assert len(msgs) > 4


@gpu
def test_more_blocks_than_a_grid_slot_each_and_the_capacity_bound(pkg):
    """1050 rows of 4 batches, 4200 blocks, one row in sixteen carrying a page and the others silence or noise; then the rows that
    close the most messages a call of 1 and of 2 batches can"""
    names, plane, _ = builders(1200)
    rows = 1050
    big = np.zeros((rows, 4 * WAVE_BATCH), np.float32)
    big[::16] = plane[names.index("a tone-only page"), :4 * WAVE_BATCH]
    big[5::16] = plane[names.index("white noise"), :4 * WAVE_BATCH]
    msgs, _ = run_calls(pkg, big, (4,), "4200 blocks")
    assert len(msgs) == len(range(0, rows, 16))
    for nb in (1, 2):
        st, cplane = capacity_case(nb)
        msgs, _ = run_calls(pkg, cplane, (nb,), f"capacity {nb}", state=st)
        assert len(msgs) == pkg.pocsag_max_messages(nb)


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    pg = pkg.Pocsag([1, 1, 0], max_batches=nb)
    dest = Dest(rows, nb, rows, 1200)
    plane = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_plane=plane.data_ptr(), row_stride=nb * WAVE_BATCH, d_messages=dest.messages.data_ptr(), d_bits=None, d_q=None,
             d_first=dest.row_first.data_ptr(), d_count=dest.count.data_ptr()):
        pg.process_device(d_plane, row_stride, nbatches, d_messages, d_first, d_count, d_bits=d_bits, d_q=d_q, hip_stream=s)

    null, count, short, align = "NULL argument", "nbatches outside 1 .. max_batches", "a row stride is shorter than the call", \
        "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; message records 8-byte aligned"
    for bad, words in ((dict(nbatches=0), count), (dict(nbatches=nb + 1), count), (dict(d_messages=None), null), (dict(d_plane=None), null),
                       (dict(d_first=None), null), (dict(d_count=None), null), (dict(d_plane=plane.data_ptr() + 4), align),
                       (dict(d_messages=dest.messages.data_ptr() + 4), align), (dict(d_bits=dest.bits.data_ptr() + 2), align),
                       (dict(d_q=dest.q.data_ptr() + 2), align), (dict(row_stride=nb * WAVE_BATCH + 2), align), (dict(row_stride=WAVE_BATCH), short),
                       (dict(d_first=dest.row_first.data_ptr() + 2), align), (dict(d_count=dest.count.data_ptr() + 2), align)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID and words in str(e.value), (bad, str(e.value))
    with pytest.raises(pkg.MiError) as e:
        pg.download(s)  # nothing was enqueued yet
    assert "no mi_pocsag_process_device call" in str(e.value)
    call()
    msgs, first, count = pg.download(s)
    assert tuple(count) == (0, 0) and list(first) == [0, 0, 0, 0] and len(msgs) == 0
    pg.set_timing(True)
    call()
    assert len(pg.last_launch_ms()) == 5
    pg.close()


E2E_BATCHES = 8
E2E_PAGE = (0x0B0B3, 3, "behind the NFM demodulator")


def e2e_setup(pkg):
    """One stream, one NFM channel five bins above the centre at fft 512, 2.56 Msps: a carrier keyed +-4.5 kHz by the model's NRZ of one
    page at 1200 baud, bit 1 the lower frequency, which begins a quarter of a second in: (dev, chans, iq uint8, batches)."""
    from common import AGC_EXTRA
    rate, centre = 2560000, 152000000
    dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9)
    chans = [pkg.channel_cfg(centre + 25000, modulation=pkg.MOD_NFM)]
    hop = rate // 16000
    n_audio = E2E_BATCHES * WAVE_BATCH + AGC_EXTRA + 8
    nrz = m.render(m.transmission([(E2E_PAGE[0], E2E_PAGE[1], m.alpha_words(E2E_PAGE[2]))], preamble=64), 12 * 4000 + 50, n_audio, 1200, amp=1.0)
    n = n_audio * hop
    dphi = 2.0 * np.pi * (25000.0 + 4500.0 * np.repeat(nrz, hop)) / rate  # (render: bit 1 is -1, the lower frequency)
    z = 30.0 * np.exp(1j * np.cumsum(dphi)).astype(np.complex64)
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    iq += np.random.default_rng(74).normal(0.0, 1.5, 2 * n).astype(np.float32)
    return dev, chans, np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8), E2E_BATCHES


@gpu
def test_behind_the_demodulator(pkg):
    """An NFM carrier keyed by one page, a second of u8 I/Q built on the host, through mi_demod_process_device and the stage: the
    page sent is the page found, and bits, Q, record and state equal the model over the audio the demodulator returned.  The record's
    `inverted` is the demodulator's sign: a lower radio frequency comes out as negative audio, which is bit 1, polarity as sent."""
    dev, chans, iq, nb = e2e_setup(pkg)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
    wo, _, _, _ = d.process([iq], nb)
    d.close()
    plane = np.ascontiguousarray(wo[0][:, :nb * WAVE_BATCH])
    pg = pkg.Pocsag([1], max_batches=nb)
    dest = Dest(1, nb, pg.max_messages, 1200)
    got = pg_call(pg, to_dev(plane), nb * WAVE_BATCH, nb, dest)
    want = pocsag_model(plane)
    check("behind the demodulator", got, dest, 1, nb, [1], want)
    assert pg.state().tobytes() == want[4].tobytes()
    pg.close()
    print(f"behind the NFM demodulator: {m.found(got[0])}, inverted {got[0]['inverted']}, lanes {got[0]['lane_sync']} -> {got[0]['lane_end']}")
    assert m.found(got[0]) == [E2E_PAGE] and pkg.pocsag_message_text(got[0][0]) == E2E_PAGE[2]
    assert got[0][0]["inverted"] == 0
