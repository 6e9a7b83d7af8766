"""The CTCSS tone finder on the GPU (mi_tones_*, csrc/tones.hip) against the numpy restatement in tones_model.py and against its host
twin mi_tones_plan_host.

Every comparison is bit for bit: records, powers and the state blob travel and are compared as bytes -- the recurrence, the order of
the sum and the tie rules are part of the definition.  Every destination buffer is filled with a sentinel before a call and is
longer than the capacity the finder is told; what it must not write must still hold the sentinel afterwards."""
import numpy as np
import pytest

from common import AGC_EXTRA
from test_tones_model import E2E_BATCHES, LONG_NB, LONG_WINDOWS, STAR, assert_long_call_conditions, case, e2e_setup, e2e_verdict
from tones_model import (LANES, LONG_PRELUDE, NO_SIGNAL, NTONES, RECORD, WAVE_BATCH, fresh_state, long_call_masks, long_call_planes, run_in_calls,
                         tones_model)

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity


class Dest:
    """destination buffers for `cap` records, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, cap, powers=True):
        import torch
        self.cap = cap
        self.records = torch.full(((cap + GUARD) * RECORD.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.powers = torch.full(((cap + GUARD) * LANES * 4,), SENT_BYTE, dtype=torch.uint8, device="cuda") if powers else None
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def tones_call(tn, d_wave, row_stride, d_axc, axc_stride, nb, dest, stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    tn.process_device(d_wave.data_ptr(), row_stride, d_axc.data_ptr(), axc_stride, nb, dest.records.data_ptr(), dest.row_first.data_ptr(),
                      dest.count.data_ptr(), d_powers=None if dest.powers is None else dest.powers.data_ptr(), hip_stream=s)
    return tn.download(s)


def check(what, got, dest, rows, want_rec, want_pw, want_first):
    rec, pw, row_first, count = got
    total, k = len(want_rec), min(len(want_rec), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, want_first), f"{what}: row_first_record"
    assert rec.tobytes() == want_rec[:k].tobytes(), f"{what}: records\n{rec}\nwant\n{want_rec[:k]}"
    d_rec = dest.records.cpu().numpy()
    assert d_rec[:k * RECORD.itemsize].tobytes() == want_rec[:k].tobytes(), f"{what}: records on the device"
    assert (d_rec[k * RECORD.itemsize:] == SENT_BYTE).all(), f"{what}: something was written behind record {k}"
    if dest.powers is None:
        assert pw is None
    else:
        assert pw.tobytes() == want_pw[:k].tobytes(), f"{what}: powers"
        d_pw = dest.powers.cpu().numpy()
        assert d_pw[:k * LANES * 4].tobytes() == want_pw[:k].tobytes() and (d_pw[k * LANES * 4:] == SENT_BYTE).all(), f"{what}: powers on the device"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def run_calls(pkg, axc, wave, window, cuts, what, masks=None, cap=0, powers=True, pad=0, stream=None, twin_at=None):
    """One finder over consecutive calls of the lengths `cuts`, each over buffers laid out for `pad` more batches than the call (their
    flags the opposite of the row's last, so a walk or a twin that read them would reset or run on where the model does not):
    records, powers and the state after every call against the model, and the state against the host twin run from the same blob.
    masks: the enabled rows of each call (set_rows in between).  twin_at: that call is made by the host twin from the device's state
    blob, whose state goes back to the device."""
    import torch
    rows = axc.shape[0]
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    tn = pkg.Tones(masks[0], max_batches=max(cuts), window=window, max_records=cap)
    room = cap or rows * pkg.tones_max_windows(window, max(cuts))
    state, done, total = fresh_state(rows), 0, 0
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            tn.set_rows(en)
        lay = n + pad
        a = np.full((rows, lay), NO_SIGNAL, np.uint8)
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.5))
        a[:, :n], w[:, :n * WAVE_BATCH] = axc[:, done:done + n], wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        a[:, n:] = np.where(a[:, n - 1:n] == NO_SIGNAL, STAR, NO_SIGNAL)  # behind the call: the opposite of the row's last flag
        want_rec, want_pw, want_first, after = tones_model(a[:, :n], w[:, :n * WAVE_BATCH], state, en, window)
        before = tn.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin = pkg.tones_plan_host(en, a, w, before, window, nbatches=n)
        assert twin[0].tobytes() == want_rec.tobytes() and twin[1].tobytes() == want_pw.tobytes() and twin[4].tobytes() == after.tobytes()
        if i == twin_at:
            tn.set_state(twin[4])
        else:
            dest = Dest(rows, room, powers)
            if stream is not None:
                with torch.cuda.stream(stream):
                    d_w, d_a = to_dev(w), to_dev(a)
            else:
                d_w, d_a = to_dev(w), to_dev(a)
            got = tones_call(tn, d_w, lay * WAVE_BATCH, d_a, lay, n, dest, None if stream is None else stream.cuda_stream)
            check(f"{what}, call {i} at batch {done}", got, dest, rows, want_rec, want_pw, want_first)
        assert tn.state().tobytes() == after.tobytes(), f"{what}, call {i}: state blob after"
        state, done, total = after, done + n, total + len(want_rec)
    tn.close()
    return total, state


@gpu
@pytest.mark.parametrize("window", [800, 2000, 6400, 64000])
@pytest.mark.parametrize("rows", [1, 5, 70])
def test_device_equals_model_and_twin(pkg, rows, window):
    """Three calls of 1, 4 and 16 batches on one handle: the first completes no window at 6400 and 64000 (the state alone), windows
    begin in the carried state, and flags reset rows in mid-call.  1, 5 and 70 rows: one wave, across the four-row workgroup, and many
    workgroups.  Pieces begin and end off the 64-sample groups (800 = 12.5 * 64, a batch = 31.25 * 64) and on them (1600, 6400)."""
    axc, wave = case(rows, 21, window, seed=1)
    total, state = run_calls(pkg, axc, wave, window, (1, 4, 16), f"{rows} rows, window {window}")
    assert (total > 0) == (window < 64000)
    if window == 64000:
        assert int(state[0]["count"]) == 21 * WAVE_BATCH and state[0]["q1"][:NTONES].any() and not state[0]["q1"][NTONES:].any()


@gpu
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg):
    """rows 1 and 3 sit the second of four calls out -- no record, every byte of their state stays --; the third call is made by the
    host twin from the device's blob and handed back with set_state; the fourth goes on from it"""
    rows = 5
    axc, wave = case(rows, 16, 2000, seed=2)
    masks = [np.ones(rows, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(rows, np.uint8), np.ones(rows, np.uint8)]
    total, state = run_calls(pkg, axc, wave, 6400, (3, 5, 3, 5), "set_rows", masks=masks, twin_at=2)
    assert total >= 4 and int(state["seq"][0]) == 16 * WAVE_BATCH // 6400  # (row 0 has no reset; seq counts the twin's windows too)
    with pytest.raises(pkg.MiError) as e:
        bad = fresh_state(1)
        bad[0]["count"] = 6400
        t = pkg.Tones([1], max_batches=2)
        t.set_state(bad)
    assert e.value.code == pkg.MI_ERR_INVALID


@gpu
@pytest.mark.parametrize("powers", [True, False])
def test_capped_records_padded_strides_and_a_side_stream(pkg, powers):
    """a record buffer shorter than the call's records is left untouched beyond its cap, with and without d_powers; the buffers are
    laid out for three batches more than the call; everything is enqueued on a side stream with no synchronisation before download"""
    import torch
    axc, wave = case(5, 12, 800, seed=3)
    want = run_in_calls(axc, wave, (5, 7), 800)[0]
    cap = min(len(c[1]) for c in want) // 2
    assert cap >= 2
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    run_calls(pkg, axc, wave, 800, (5, 7), f"cap {cap}, powers {powers}", cap=cap, powers=powers, pad=3, stream=side)


def long_case(nb, window):
    """long_call_planes, with the conditions that make it worth running checked from the model before the device sees it"""
    axc, wave = long_call_planes(nb, window)
    masks = long_call_masks()
    calls = run_in_calls(axc, wave, (LONG_PRELUDE, nb), window, masks=masks)[0]
    assert_long_call_conditions(nb, window, calls)
    return axc, wave, masks, calls


@gpu
@pytest.mark.parametrize("window", LONG_WINDOWS)
@pytest.mark.parametrize("nb", LONG_NB)
def test_calls_past_64_batches_equal_model_and_twin(pkg, nb, window):
    """A 3-batch call, then one of 64, 65, 128 or 130 batches in the carried state: k_tones_walk takes each row in two or three trips
    of 64 flags and carries count, window start, carried-state mark and record count from trip to trip.  Nine rows (tones_model.py,
    long_call_planes): all signal -- whole trips, more than 64 windows a stretch at window 800, a window across the trip boundary at
    64000 --, all silent, a reset on the last lane of trip 0 and on the first of trip 1, a run from lane 62 to lane 2 of the next
    trip, a silent first trip, two drawn rows and one the long call disables."""
    axc, wave, masks, calls = long_case(nb, window)
    total, state = run_calls(pkg, axc, wave, window, (LONG_PRELUDE, nb), f"long call of {nb}, window {window}", masks=masks)
    assert total == sum(len(c[1]) for c in calls) and state.tobytes() == calls[1][4].tobytes()


@gpu
def test_long_call_with_half_its_records_stored(pkg):
    """130 batches at window 800 with room for half the long call's records: the walk writes no piece and the bank no record at or
    behind the capacity, row_first_record and count[0] still count them all, and every row's tail still writes its state"""
    axc, wave, masks, calls = long_case(130, 800)
    cap = len(calls[1][1]) // 2
    assert cap > len(calls[0][1]) and cap > 129
    for powers in (True, False):
        run_calls(pkg, axc, wave, 800, (LONG_PRELUDE, 130), f"long call, cap {cap}, powers {powers}", masks=masks, cap=cap, powers=powers)


@gpu
def test_long_call_padded_strides_on_a_side_stream(pkg):
    """65 batches in buffers laid out for 68, enqueued on a side stream behind the uploads: lane 0 of the second trip reads batch 64 of
    its own row, not what lies behind the call"""
    import torch
    axc, wave, masks, _ = long_case(65, 800)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    run_calls(pkg, axc, wave, 800, (LONG_PRELUDE, 65), "long call, padded, side stream", masks=masks, pad=3, stream=side)


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    tn = pkg.Tones([1, 1, 0], max_batches=nb, window=800)
    dest = Dest(rows, rows * 5)
    wave = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    axc = torch.full((rows, nb), STAR, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=wave.data_ptr(), row_stride=nb * WAVE_BATCH, d_records=dest.records.data_ptr(), d_axc=axc.data_ptr(), d_powers=None):
        tn.process_device(d_wave, row_stride, d_axc, nb, nbatches, d_records, dest.row_first.data_ptr(), dest.count.data_ptr(), d_powers=d_powers,
                          hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_axc=None), dict(d_records=None), dict(d_wave=None), dict(d_wave=wave.data_ptr() + 4),
                dict(d_records=dest.records.data_ptr() + 4), dict(row_stride=nb * WAVE_BATCH + 2), dict(row_stride=WAVE_BATCH),
                dict(d_powers=dest.powers.data_ptr() + 2)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        tn.download(s)  # nothing was enqueued yet
    call()
    rec, pw, first, count = tn.download(s)
    assert tuple(count) == (10, 10) and list(first) == [0, 5, 10, 10] and pw is None and not rec["best_power"].any()
    with pytest.raises(pkg.MiError) as e:  # powers asked for after a call that stored none
        tn._with_powers = True
        tn.download(s)
    assert e.value.code == pkg.MI_ERR_INVALID
    for kw in (dict(max_batches=0), dict(window=799), dict(window=64001)):
        with pytest.raises(pkg.MiError) as e:
            pkg.Tones(np.ones(5), **{"max_batches": 2, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID
    tn.close()


@gpu
def test_behind_the_demodulator(pkg):
    """The capture of the CPU end-to-end test, generated on the device, through mi_demod_process_device and the finder on one stream in
    three calls of 8 batches: records, powers and state equal the model over the audio and flags the demodulator returned; the vote
    gives 100.0 on the first row and nothing on the second; and a second demodulator planned with ctcss = 100.0 on that channel
    counts the tone too."""
    import torch
    calls = (8, 8, 8)
    dev, chans, cfg, nbytes = e2e_setup(pkg)
    rows = len(chans)
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, 1, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    tn = pkg.Tones(np.ones(rows), max_batches=max(calls))
    outs, done = [], 0
    for n in calls:  # (no host synchronisation between the demodulator and the finder)
        wo = torch.zeros((rows, n * WAVE_BATCH), dtype=torch.float32, device="cuda")
        ax = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
        dest = Dest(rows, rows * pkg.tones_max_windows(0, n))
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, nbytes, n, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        got = tones_call(tn, wo, n * WAVE_BATCH, ax, n, n, dest, stream=s)
        outs.append((got, dest, wo.cpu().numpy(), ax.cpu().numpy()))
        done += n
    d.close()
    state, recs = None, []
    for i, (got, dest, wo, ax) in enumerate(outs):
        want_rec, want_pw, want_first, state = tones_model(ax, wo, state)
        check(f"behind the demodulator, call {i}", got, dest, rows, want_rec, want_pw, want_first)
        recs.append((got[0], got[2]))
    assert tn.state().tobytes() == state.tobytes()
    tn.close()
    print("flags:", ["".join(bytes(o[3][r]).decode() for o in outs) for r in range(rows)])
    per_row = [np.concatenate([rec[first[r]:first[r + 1]] for rec, first in recs]) for r in range(rows)]
    e2e_verdict(pkg, np.concatenate(per_row), np.cumsum([0] + [len(x) for x in per_row]))
    chans[0] = pkg.channel_cfg(chans[0].freq, modulation=pkg.MOD_NFM, bandwidth=12500, ctcss=100.0)
    d2 = pkg.Demod(dev, chans, nstreams=1, max_batches=E2E_BATCHES)
    wo = torch.zeros((rows, E2E_BATCHES * WAVE_BATCH), dtype=torch.float32, device="cuda")
    ax = torch.zeros((rows, E2E_BATCHES), dtype=torch.uint8, device="cuda")
    d2.process_device(d_iq.data_ptr(), nbytes, E2E_BATCHES, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
    torch.cuda.synchronize()
    stats = d2.stats()
    d2.close()
    print("planned with ctcss 100.0: ctcss_count", stats[0].ctcss_count, "no_ctcss_count", stats[0].no_ctcss_count)
    assert stats[0].ctcss_count > 0
