"""The packet decoder stage on the GPU (mi_ax25_*, csrc/ax25.hip) against the numpy restatement in ax25_model.py and against its
host twin mi_ax25_plan_host.

Every comparison is bit for bit: tone bits, frames, prefix, counts and the state blob travel and are compared as bytes.  Every
destination buffer is filled with a sentinel before a call and is longer than the capacity the stage is told; what it must not write
must still hold the sentinel afterwards."""
import numpy as np
import pytest

import ax25_model as m
from ax25_model import FRAME_REC, NB, NLANES, NWORDS, WAVE_BATCH, ax25_model, fresh_state
from test_ax25_model import builders, sent

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity
BLOCK = NLANES * NWORDS


class Dest:
    """destination buffers for `cap` frames and the rows * nb blocks' bits, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, nb, cap):
        import torch
        self.cap = cap
        self.frames = torch.full(((cap + GUARD) * FRAME_REC.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.bits = torch.full((rows * nb * BLOCK + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def ax_call(ax, d_plane, row_stride, nb, dest, stream=None, scratch=False):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    ax.process_device(d_plane.data_ptr(), row_stride, nb, dest.frames.data_ptr(), dest.row_first.data_ptr(), dest.count.data_ptr(),
                      d_bits=None if scratch else dest.bits.data_ptr(), hip_stream=s)
    return ax.download(s)


def check(what, got, dest, rows, nb, en, want, scratch=False):
    frames, row_first, count = got
    w_frames, w_bits, w_first, _ = want
    total, k = len(w_frames), min(len(w_frames), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, w_first), f"{what}: row_first_frame"
    assert frames.tobytes() == w_frames[:k].tobytes(), f"{what}: frames\n{frames[['row', 'batch', 'third', 'lane', 'nbytes']]}\nwant\n{w_frames[:k][['row', 'batch', 'third', 'lane', 'nbytes']]}"
    d_frames = dest.frames.cpu().numpy()
    assert d_frames[:k * FRAME_REC.itemsize].tobytes() == w_frames[:k].tobytes(), f"{what}: frames on the device"
    assert (d_frames[k * FRAME_REC.itemsize:] == SENT_BYTE).all(), f"{what}: something was written behind frame {k}"
    bits = dest.bits.cpu().numpy().view(np.uint32)
    if scratch:
        assert (bits == 0xA5A5A5A5).all(), f"{what}: bits written though the call gave none"
    else:
        on = np.asarray(en, bool)
        g_bits = bits[:rows * nb * BLOCK].reshape(w_bits.shape)
        bad = np.argwhere(g_bits[on] != w_bits[on])
        assert not len(bad), f"{what}: tone bits, first at {bad[:3]}"
        assert (g_bits[~on] == 0xA5A5A5A5).all() and (bits[rows * nb * BLOCK:] == 0xA5A5A5A5).all(), f"{what}: bits that must not be written"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def run_calls(pkg, plane, cuts, what, cfg=None, model_kw=None, masks=None, cap=0, pads=(0,), stream=None, twin_at=None, state=None, scratch=False):
    """One handle over consecutive calls of the lengths `cuts`, call i over a plane laid out for pads[i % len] more batches than the
    call: bits, frames and the state after every call against the model, and the host twin run from the same blob against both.
    masks: the enabled rows of each call (set_rows in between).  twin_at: that call is made by the host twin from the device's state
    blob, whose state goes back to the device.  Returns (frames of all calls, state)."""
    import torch
    rows = plane.shape[0]
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    ax = pkg.Ax25(masks[0], max_batches=max(cuts), cfg=cfg, max_frames=cap)
    if state is None:
        state = fresh_state(rows)
    else:
        ax.set_state(state)
    done, all_frames = 0, []
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            ax.set_rows(en)
        lay = n + pads[i % len(pads)]
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.25))  # behind the call: a level that must not be read
        w[:, :n * WAVE_BATCH] = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = ax25_model(w[:, :n * WAVE_BATCH], state, en, **(model_kw or {}))
        before = ax.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin = pkg.ax25_plan_host(en, w, cfg, before, nbatches=n)
        assert twin[0].tobytes() == want[0].tobytes() and twin[1].tobytes() == want[1].tobytes() and twin[4].tobytes() == want[3].tobytes(), \
            f"{what}, call {i}: the twin and the model differ"
        if i == twin_at:
            ax.set_state(twin[4])
        else:
            room = cap or rows * pkg.ax25_max_frames(max(cuts))
            dest = Dest(rows, n, room)
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_w = to_dev(w)
            else:
                d_w = to_dev(w)
            got = ax_call(ax, d_w, lay * WAVE_BATCH, n, dest, None if stream is None else stream.cuda_stream, scratch)
            check(f"{what}, call {i} at batch {done}", got, dest, rows, n, en, want, scratch)
        assert ax.state().tobytes() == want[3].tobytes(), f"{what}, call {i}: state blob after"
        state, done = want[3], done + n
        all_frames.append(want[0])
    ax.close()
    return np.concatenate(all_frames), state


def tiled(plane, rows):
    return plane[np.arange(rows) % plane.shape[0]]


@gpu
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_device_equals_model_and_twin(pkg, rows):
    """Calls of 1 and 4 batches on one handle over the first 24 batches: over the longest frame's row at 1 row, over it and its four
    neighbours at 5, and over every builder's row, tiled, at 70 -- one block, a few, many; frames that begin in one call and end in
    another; bits that begin in the carried samples."""
    names, plane, _, _, _ = builders()
    first = names.index("the longest frame")
    plane = tiled(plane, rows) if rows == 70 else plane[first:first + rows]
    frames, state = run_calls(pkg, plane, (1, 4, 1, 4, 4, 1, 4, 4, 1), f"{rows} rows")
    assert len(frames) >= rows // 2 and state["batch"][0] == 24


@gpu
def test_48_batches_in_one_call(pkg):
    """every builder's row over the whole 48 batches in one launch: what the builders send is what is found"""
    names, plane, found, _, _ = builders()
    frames, state = run_calls(pkg, plane, (NB,), "48 batches")
    first = np.searchsorted(frames["row"], np.arange(len(names) + 1))
    assert [sent(frames, first, r) for r in range(len(names))] == found


@gpu
def test_set_rows_and_the_state_through_the_twin(pkg):
    """rows 1 and 3 sit the second of four calls out -- no record, every byte of their state stays --; the third call is made by the
    host twin from the device's blob, inside the longest frame and between the two frames 50 flags apart, and handed back with
    set_state; the fourth goes on from it.  Impossible blobs are refused."""
    names, plane, _, _, _ = builders()
    rws = [names.index(n) for n in ("the longest frame", "a short UI frame", "two frames 50 flags apart", "white noise", "two frames sharing one flag")]
    masks = [np.ones(5, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(5, np.uint8), np.ones(5, np.uint8)]
    st = fresh_state(5)
    st["x"][:] = np.random.default_rng(9).normal(0, 0.05, (5, 14)).astype(np.float32)
    frames, state = run_calls(pkg, plane[rws], (2, 2, 3, 17), "set_rows", masks=masks, twin_at=2, state=st, cfg=pkg.ax25_cfg(strict=False), model_kw=dict(strict=False))
    assert len(frames) >= 4 and state["batch"][0] == 24 and state["batch"][1] == 22
    ax = pkg.Ax25([1], max_batches=2)
    for what, blob, words in m.bad_blobs():
        if words is None:
            ax.set_state(blob)
            continue
        with pytest.raises(pkg.MiError) as e:
            ax.set_state(blob)
        assert e.value.code == pkg.MI_ERR_INVALID and "packet stage state: " in str(e.value) and words in str(e.value), what
    ax.close()


@gpu
def test_a_malformed_address_field_without_strict(pkg):
    """the bad callsign byte's row beside a well-formed one under MI_AX25_STRICT_OFF, in calls of 4 batches: device = model = twin,
    and the malformed frame is one record with naddr 0 whose bytes are the ones sent; a strict handle drops it"""
    names, plane, found, loose, _ = builders()
    r = names.index("a bad callsign byte")
    rws = [r, names.index("a short UI frame")]
    frames, _ = run_calls(pkg, plane[rws, :8 * WAVE_BATCH], (4, 4), "strict off", cfg=pkg.ax25_cfg(strict=False), model_kw=dict(strict=False))
    bad = frames[frames["row"] == 0]
    assert len(bad) == 1 and bad[0]["naddr"] == 0 and [bytes(bad[0]["bytes"][:bad[0]["nbytes"]])] == loose[r] and (frames[frames["row"] == 1]["naddr"] == 2).all()
    frames, _ = run_calls(pkg, plane[rws, :8 * WAVE_BATCH], (8,), "strict on")
    assert (frames["row"] == 1).all() and len(frames) == 1


@gpu
@pytest.mark.parametrize("scratch", [False, True])
def test_capped_frames_padded_unequal_strides_and_a_side_stream(pkg, scratch):
    """a frame buffer shorter than the call's frames is left untouched beyond its cap, with the bits in the caller's buffer and in
    the handle's; the planes are laid out for three and for one batch more than the call; everything is enqueued on a side stream
    with no synchronisation before download"""
    import torch
    plane = builders()[1][:10, :12 * WAVE_BATCH]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    frames, _ = run_calls(pkg, plane, (5, 7), f"cap 3, scratch {scratch}", cap=3, pads=(3, 1), stream=side, scratch=scratch)
    assert len(frames) > 3


@gpu
def test_more_blocks_than_a_grid_slot_each(pkg):
    """1050 rows of 4 batches, 4200 blocks, one row in sixteen carrying a frame and the others silence or noise"""
    names, plane, _, _, _ = builders()
    short = plane[names.index("a short UI frame"), :4 * WAVE_BATCH]
    rows = 1050
    big = np.zeros((rows, 4 * WAVE_BATCH), np.float32)
    big[::16] = short
    big[5::16] = plane[names.index("white noise"), :4 * WAVE_BATCH]
    frames, _ = run_calls(pkg, big, (4,), "4200 blocks")
    assert len(frames) == len(range(0, rows, 16))


@gpu
def test_the_40_start_thirds_the_ordering_cases_and_the_bound(pkg):
    plane, f = m.start_thirds()
    frames, _ = run_calls(pkg, plane, (m.START_BATCHES,), "start thirds")
    assert len(frames) == 40 and all(bytes(x["bytes"][:x["nbytes"]]) == f for x in frames)
    names, st, oplane, expect = m.ordering_cases()
    frames, _ = run_calls(pkg, oplane, (1,), "ordering", state=st)
    assert [int((frames["row"] == r).sum()) for r in range(len(names))] == expect
    for nb in (1, 2):
        st, cplane = m.capacity_case(nb)
        frames, _ = run_calls(pkg, cplane, (nb,), f"capacity {nb}", state=st)
        assert len(frames) == pkg.ax25_max_frames(nb)


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    ax = pkg.Ax25([1, 1, 0], max_batches=nb)
    dest = Dest(rows, nb, rows)
    plane = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_plane=plane.data_ptr(), row_stride=nb * WAVE_BATCH, d_frames=dest.frames.data_ptr(), d_bits=None,
             d_first=dest.row_first.data_ptr(), d_count=dest.count.data_ptr()):
        ax.process_device(d_plane, row_stride, nbatches, d_frames, d_first, d_count, d_bits=d_bits, hip_stream=s)

    null, count, short, align = "NULL argument", "nbatches outside 1 .. max_batches", "a row stride is shorter than the call", \
        "the plane must be 16-byte aligned with a row stride that is a multiple of 4 floats; frame records 8-byte aligned"
    for bad, words in ((dict(nbatches=0), count), (dict(nbatches=nb + 1), count), (dict(d_frames=None), null), (dict(d_plane=None), null),
                       (dict(d_first=None), null), (dict(d_count=None), null), (dict(d_plane=plane.data_ptr() + 4), align),
                       (dict(d_frames=dest.frames.data_ptr() + 4), align), (dict(d_bits=dest.bits.data_ptr() + 2), align),
                       (dict(row_stride=nb * WAVE_BATCH + 2), align), (dict(row_stride=WAVE_BATCH), short),
                       (dict(d_first=dest.row_first.data_ptr() + 2), align), (dict(d_count=dest.count.data_ptr() + 2), align)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID and words in str(e.value), (bad, str(e.value))
    with pytest.raises(pkg.MiError) as e:
        ax.download(s)  # nothing was enqueued yet
    assert "no mi_ax25_process_device call" in str(e.value)
    call()
    frames, first, count = ax.download(s)
    assert tuple(count) == (0, 0) and list(first) == [0, 0, 0, 0] and len(frames) == 0
    ax.set_timing(True)
    call()
    assert len(ax.last_launch_ms()) == 5
    ax.close()


E2E_BATCHES = 10
E2E = dict(src="E2E", src_ssid=9, dst="APRS", digis=[("WIDE2", 1, True)], info=b">behind the NFM demodulator")


def e2e_setup(pkg):
    """One stream, one NFM channel five bins above the centre at fft 512, 2.56 Msps: a carrier frequency-modulated at one deviation
    (3 kHz peak, no pre-emphasis) by the model's AFSK of one frame, which begins half a second in: (dev, chans, iq uint8, batches)."""
    from common import AGC_EXTRA
    rate, centre = 2560000, 144000000
    dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9)
    chans = [pkg.channel_cfg(centre + 25000, modulation=pkg.MOD_NFM)]
    hop = rate // 16000
    n_audio = E2E_BATCHES * WAVE_BATCH + AGC_EXTRA + 8
    audio = m.modulate(m.burst_bits([m.ui_frame(**E2E)], before=30), 3 * 8000 + 11, n_audio, amp=1.0)
    n = n_audio * hop
    dphi = 2.0 * np.pi * (25000.0 + 3000.0 * np.repeat(audio, hop)) / rate
    z = 30.0 * np.exp(1j * np.cumsum(dphi)).astype(np.complex64)
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    iq += np.random.default_rng(74).normal(0.0, 1.5, 2 * n).astype(np.float32)
    return dev, chans, np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8), E2E_BATCHES


@gpu
def test_behind_the_demodulator(pkg):
    """An NFM carrier modulated by one frame, 1.25 s of u8 I/Q built on the host, through mi_demod_process_device and the stage: the
    frame sent is the frame found, and bits, record and state equal the model over the audio the demodulator returned.  Which
    slicers decode the capture alone is printed."""
    dev, chans, iq, nb = e2e_setup(pkg)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
    wo, axc, _, _ = d.process([iq], nb)
    d.close()
    plane = np.ascontiguousarray(wo[0][:, :nb * WAVE_BATCH])
    ax = pkg.Ax25([1], max_batches=nb)
    dest = Dest(1, nb, ax.max_frames)
    got = ax_call(ax, to_dev(plane), nb * WAVE_BATCH, nb, dest)
    want = ax25_model(plane)
    check("behind the demodulator", got, dest, 1, nb, [1], want)
    assert ax.state().tobytes() == want[3].tobytes()
    ax.close()
    f = m.ui_frame(**E2E)
    assert [bytes(x["bytes"][:x["nbytes"]]) for x in got[0]] == [bytes(f)]
    assert pkg.ax25_frame_text(got[0][0]) == "E2E-9>APRS,WIDE2-1*:>behind the NFM demodulator"
    off = 1e30
    alone = [len(pkg.ax25_plan_host([1], plane, pkg.ax25_cfg(gain=g))[0]) for g in ((1.0, off, off), (off, m.DEFAULT_GAIN[1], off), (off, off, m.DEFAULT_GAIN[2]))]
    print(f"behind the NFM demodulator: record on lane {int(got[0][0]['lane'])}; slicers alone decode {alone}")
