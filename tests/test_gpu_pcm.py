"""The PCM stage on the GPU (mi_pcm_*, csrc/pcm.hip) against the numpy restatement in pcm_model.py and against its host twin
mi_pcm_plan_host.

Every comparison is bit for bit: blocks and the state blob travel and are compared as bytes -- the order of the filter's sum, the
rounding of the quantiser and the encoder's recurrence are part of the definition.  The index and the counts the stage reads are the
ones an output gate wrote on the same stream just before, with no host step between -- or, in run_by_hand, ones uploaded by hand
that no gate writes: more entries than the call's grid has workgroups, and entries that are not of the call.  The destination is filled with a sentinel
before a call and is longer than the capacity the stage is told; what it must not write must still hold the sentinel afterwards."""
import numpy as np
import pytest

import pcm_model as pm
from common import AGC_EXTRA, bytes_for_batches
from gate_model import NO_SIGNAL, draw_flags, gate_model
from pcm_model import CONFIGS, HISTORY, IMA4, S16, WAVE_BATCH, audio, pcm_model

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 2  # blocks allocated behind the capacity
GATE_OPEN_TRAIL, GATE_ALL = 2, 3


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class GateDest:
    """what the gate writes, for rows * nb blocks"""

    def __init__(self, rows, nb):
        import torch
        self.blocks = torch.empty((rows * nb, WAVE_BATCH), dtype=torch.float32, device="cuda")
        self.index = torch.full((rows * nb + GUARD, 2), SENT32, dtype=torch.int32, device="cuda")
        self.row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
        self.count = torch.zeros(2, dtype=torch.int32, device="cuda")


def flags_for(rows, nb, seed, p_open=0.6):
    axc = draw_flags(np.random.default_rng(seed), rows, nb, p_open)
    axc[0, 0] = ord("*")  # (some block travels whatever was drawn)
    return axc


def run_calls(pkg, wave, axc, cuts, rate, fmt, what, masks=None, cap=0, pad=0, stream=None, twin_at=None, rule=GATE_OPEN_TRAIL):
    """One gate and one PCM stage over consecutive calls of the lengths `cuts`, each over buffers laid out for `pad` more batches than
    the call (filled with 0.5, flags open: a stage that read them would encode something else): gate and stage are enqueued back to
    back on one stream; the blocks against the model over the gate's own index, the device's state after every call against the
    model's and the twin's.  masks: the enabled rows of each call (set_rows in between).  twin_at: that call is made by the host twin
    from the device's state blob, whose state goes back to the device.  Returns [(index, blocks)] per call and the last state."""
    import torch
    rows = wave.shape[0]
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    bb = pm.block_bytes(rate, fmt)
    gate = pkg.OutputGate(np.full(rows, rule, np.uint8), max_batches=max(cuts))
    pcm = pkg.Pcm(masks[0], max_batches=max(cuts), rate=rate, fmt=fmt, max_blocks=cap)
    assert pcm.block_bytes == bb and pcm.max_blocks == (min(cap, rows * max(cuts)) if cap else rows * max(cuts))
    s = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    state, carried, done, outs = pm.fresh_state(rows), np.zeros(rows, np.uint8), 0, []
    for i, (n, en) in enumerate(zip(cuts, masks)):
        if i:
            pcm.set_rows(en)
        lay = n + pad
        a = np.full((rows, lay), ord("*"), np.uint8)
        w = np.full((rows, lay * WAVE_BATCH), np.float32(0.5))
        a[:, :n], w[:, :n * WAVE_BATCH] = axc[:, done:done + n], wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        index, _, carried = gate_model(np.full(rows, rule, np.uint8), a[:, :n], carried)
        want, after = pcm_model(w, index, state, en, rate, fmt, nbatches=n)
        before = pcm.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin_blocks, twin_state = pkg.pcm_plan_host(en, w, index, before, rate, fmt, nbatches=n)
        assert twin_blocks.tobytes() == want.tobytes() and twin_state.tobytes() == after.tobytes(), f"{what}, call {i}: the twin"
        room = pcm.max_blocks
        k = min(len(index), room)
        if i == twin_at:
            pcm.set_state(twin_state)
            # (the gate's carried flags move on as the model's did)
            gate.set_state(carried)
        else:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                d_w, d_a = to_dev(w), to_dev(a)
                gd = GateDest(rows, n)
                d_out = torch.full(((room + GUARD) * bb,), SENT_BYTE, dtype=torch.uint8, device="cuda")
            gate.process_device(d_w.data_ptr(), lay * WAVE_BATCH, d_a.data_ptr(), lay, n, gd.blocks.data_ptr(), gd.index.data_ptr(),
                                gd.row_first.data_ptr(), gd.count.data_ptr(), hip_stream=s)
            pcm.process_device(d_w.data_ptr(), lay * WAVE_BATCH, n, gd.index.data_ptr(), gd.count.data_ptr(), d_out.data_ptr(), hip_stream=s)
            got, count = pcm.download(s)
            assert np.array_equal(gate.download(s)[2], index), f"{what}, call {i}: the gate's index is not the model's"
            assert (int(count[0]), int(count[1])) == (len(index), k), f"{what}, call {i}: counts {count}"
            assert got.shape == (k, bb) and got.tobytes() == want[:k].tobytes(), f"{what}, call {i} at batch {done}: blocks"
            raw = d_out.cpu().numpy()
            assert raw[:k * bb].tobytes() == want[:k].tobytes(), f"{what}, call {i}: blocks on the device"
            assert (raw[k * bb:] == SENT_BYTE).all(), f"{what}, call {i}: something was written behind block {k}"
        assert pcm.state().tobytes() == after.tobytes(), f"{what}, call {i}: state blob after"
        outs.append((index, want))
        state, done = after, done + n
    pcm.close()
    gate.close()
    return outs, state


@gpu
@pytest.mark.parametrize("rate,fmt", CONFIGS)
@pytest.mark.parametrize("rows", [1, 5, 70])
@pytest.mark.parametrize("nb", [1, 4])
def test_device_equals_model_and_twin(pkg, nb, rows, rate, fmt):
    """Every builder through a call of nb batches and one more batch behind it, whose history is the carried state.  1, 5 and 70 rows:
    one block, a handful, and more workgroups than one batch has rows.  The index comes straight from mi_outgate_process_device under
    MI_GATE_OPEN_TRAIL with drawn flags."""
    for name in pm.BUILDERS:
        wave = audio(name, rows, nb + 1)
        outs, state = run_calls(pkg, wave, flags_for(rows, nb + 1, seed=rows * 10 + nb), (nb, 1), rate, fmt, f"{name}, {rows} rows, {nb} batches")
        assert len(outs[0][0]) >= 1 and state["x"].tobytes() == wave[:, -HISTORY:].tobytes()


@gpu
@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_capacity_smaller_than_the_gate_s_count(pkg, rate, fmt):
    """max_blocks below what the gate stored: the first max_blocks blocks, nothing touched beyond, every tail still carried"""
    rows, nb = 5, 4
    axc = flags_for(rows, nb + 1, seed=7, p_open=0.9)
    total = len(gate_model(np.full(rows, GATE_OPEN_TRAIL, np.uint8), axc[:, :nb])[0])
    cap = total // 2
    assert cap >= 3
    run_calls(pkg, audio("noise", rows, nb + 1), axc, (nb, 1), rate, fmt, f"cap {cap} of {total}", cap=cap)


@gpu
@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_call_cuts_give_identical_blocks(pkg, rate, fmt):
    """4 = 1 + 1 + 1 + 1 = 1 + 3 under MI_GATE_ALL: a block's bytes do not depend on whether its history came from the row's previous
    batch or from the carried tail"""
    rows, nb = 5, 4
    wave = audio("voice", rows, nb)
    axc = np.full((rows, nb), ord("*"), np.uint8)
    whole, whole_state = run_calls(pkg, wave, axc, (nb,), rate, fmt, "one call", rule=GATE_ALL)
    want = whole[0][1].reshape(rows, nb, -1)
    for cuts in ((1, 1, 1, 1), (1, 3)):
        outs, state = run_calls(pkg, wave, axc, cuts, rate, fmt, f"cuts {cuts}", rule=GATE_ALL)
        done = 0
        for n, (index, blocks) in zip(cuts, outs):
            assert blocks.reshape(rows, n, -1).tobytes() == want[:, done:done + n].tobytes(), f"cuts {cuts}, batch {done}"
            done += n
        assert state.tobytes() == whole_state.tobytes()


@gpu
@pytest.mark.parametrize("rate,fmt", [(8000, IMA4), (16000, S16)])
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg, rate, fmt):
    """rows 1 and 3 sit the second of four calls out -- their carried samples keep their bytes, and their blocks in the gate's index
    are encoded from them --; the third call is made by the host twin from the device's blob and handed back with set_state; the
    fourth goes on from it"""
    rows = 5
    wave = audio("noise", rows, 8)
    masks = [np.ones(rows, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(rows, np.uint8), np.ones(rows, np.uint8)]
    _, state = run_calls(pkg, wave, flags_for(rows, 8, seed=3), (2, 3, 1, 2), rate, fmt, "set_rows", masks=masks, twin_at=2)
    assert state["x"].tobytes() == wave[:, -HISTORY:].tobytes()
    p = pkg.Pcm(np.ones(2), max_batches=1)
    for bad in (np.zeros(2 * 248 - 4, np.uint8), np.zeros(3 * 248, np.uint8)):
        with pytest.raises(pkg.MiError) as e:
            p.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID
    p.close()


@gpu
@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_padded_strides_on_a_side_stream(pkg, rate, fmt):
    """buffers laid out for three batches more than the call, everything enqueued on a side stream behind the uploads with no
    synchronisation before the download: the tails come from the call's last batch, not from the end of the row"""
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    run_calls(pkg, audio("voice", 5, 5), flags_for(5, 5, seed=11), (3, 2), rate, fmt, "padded, side stream", pad=3, stream=side)


def run_by_hand(pkg, pcm, long, index, count, stored, rate, fmt, what, calls=2):
    """`calls` consecutive calls of FOREIGN_SHAPE's nbatches on one handle over `long`, with an index and counts uploaded by hand
    (no gate), the input laid out for the handle's max_batches with FOREIGN_FILL behind the call, the destination sentinel-filled
    with guard blocks behind the capacity: blocks on the device and as downloaded against the model and the twin over the first
    `stored` entries, the state blob before and after every call."""
    import torch
    rows, nb, mb = pm.FOREIGN_SHAPE
    bb, room = pm.block_bytes(rate, fmt), pcm.max_blocks
    assert stored == pm.stored_blocks(count, room) <= len(index) and pcm.rows == rows and pcm.max_batches == mb
    s = torch.cuda.current_stream().cuda_stream
    d_index = torch.full((rows * mb + GUARD, 2), SENT32, dtype=torch.int32, device="cuda")  # (what lies behind the entries is of no call either)
    d_index[:len(index)] = to_dev(index.view(np.int32))
    d_count = to_dev(count.view(np.int32))
    state = pcm.state().view(pm.STATE).reshape(rows)
    for call in range(calls):
        w = pm.foreign_wave(long[:, call * nb * WAVE_BATCH:], nb, mb)
        want, after = pcm_model(w, index[:stored], state, rate=rate, fmt=fmt, nbatches=nb)
        twin_blocks, twin_state = pkg.pcm_plan_host(np.ones(rows), w, index[:stored], state, rate, fmt, nbatches=nb)
        assert twin_blocks.tobytes() == want.tobytes() and twin_state.tobytes() == after.tobytes(), f"{what}, call {call}: the twin"
        d_w = to_dev(w)
        d_out = torch.full(((room + GUARD) * bb,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        pcm.process_device(d_w.data_ptr(), mb * WAVE_BATCH, nb, d_index.data_ptr(), d_count.data_ptr(), d_out.data_ptr(), hip_stream=s)
        got, cnt = pcm.download(s)
        raw = d_out.cpu().numpy()
        assert (int(cnt[0]), int(cnt[1])) == (int(count[0]), stored), f"{what}, call {call}: counts {cnt}"
        assert raw[:stored * bb].tobytes() == want.tobytes(), f"{what}, call {call}: blocks on the device differ in " \
            f"{sorted(set(np.flatnonzero(raw[:stored * bb] != want.reshape(-1)) // bb))}"
        assert (raw[stored * bb:] == SENT_BYTE).all(), f"{what}, call {call}: something was written behind block {stored}"
        assert got.shape == (stored, bb) and got.tobytes() == raw[:stored * bb].tobytes(), f"{what}, call {call}: what download returns"
        assert pcm.state().tobytes() == after.tobytes(), f"{what}, call {call}: state blob after"
        state = after
    return state


@gpu
@pytest.mark.parametrize("rate,fmt", CONFIGS)
@pytest.mark.parametrize("case", pm.FOREIGN_CASES)
def test_foreign_index_on_a_grid_shorter_than_the_count(pkg, case, rate, fmt):
    """pcm_model.foreign_index, uploaded by hand: 3 rows on a handle of 8 batches, a call of 2, so 6 workgroups walk 20 entries (13
    under max_blocks 13; 24 under a count of 40), each making two to four trips over the same LDS, with zero entries of every kind
    as first, middle and last trips.  Twice in a row on one handle: the second call's batch 0 entries, later trips among them, read
    the first call's tails."""
    rows, nb, mb = pm.FOREIGN_SHAPE
    index, count, _, cap, stored = pm.foreign_case(case)
    pcm = pkg.Pcm(np.ones(rows), max_batches=mb, rate=rate, fmt=fmt, max_blocks=0 if cap == rows * mb else cap)
    assert pcm.max_blocks == cap and min(rows * nb, cap) == 6 < stored
    long = audio("noise" if fmt == IMA4 else "voice", rows, 2 * nb)
    state = run_by_hand(pkg, pcm, long, index, count, stored, rate, fmt, f"{case}, {rate} / {fmt}")
    assert state["x"].tobytes() == long[:, -HISTORY:].tobytes()
    pcm.close()


@gpu
@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_a_call_shorter_than_the_handle(pkg, rate, fmt):
    """the ordinary short last call: 2 batches on a handle of 8 with the full valid index of 6, grid and count the same"""
    rows, nb, mb = pm.FOREIGN_SHAPE
    pcm = pkg.Pcm(np.ones(rows), max_batches=mb, rate=rate, fmt=fmt)
    index = pm.full_index(rows, nb)
    run_by_hand(pkg, pcm, audio("voice", rows, 2 * nb), index, np.array([len(index)] * 2, np.uint32), len(index), rate, fmt, "short call")
    pcm.close()


@gpu
def test_timing_and_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    pcm = pkg.Pcm([1, 1, 0], max_batches=nb, fmt=IMA4)
    wave = torch.zeros((rows, nb * WAVE_BATCH + 4), dtype=torch.float32, device="cuda")
    index = to_dev(pm.full_index(rows, nb))
    count = to_dev(np.array([rows * nb, rows * nb], np.uint32))
    out = torch.full((rows * nb * 640 + 16,), SENT_BYTE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=wave.data_ptr(), row_stride=nb * WAVE_BATCH + 4, d_index=index.data_ptr(), d_count=count.data_ptr(), d_out=out.data_ptr()):
        pcm.process_device(d_wave, row_stride, nbatches, d_index, d_count, d_out, hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_wave=None), dict(d_index=None), dict(d_count=None), dict(d_out=None),
                dict(d_wave=wave.data_ptr() + 4), dict(d_out=out.data_ptr() + 8), dict(d_index=index.data_ptr() + 4), dict(d_count=count.data_ptr() + 2),
                dict(row_stride=nb * WAVE_BATCH + 2), dict(row_stride=nb * WAVE_BATCH - 4), dict(row_stride=WAVE_BATCH)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        pcm.download(s)  # nothing was enqueued yet
    with pytest.raises(pkg.MiError):
        pcm.last_launch_ms()
    pcm.set_timing(True)
    call()
    blocks, cnt = pcm.download(s)
    ms = pcm.last_launch_ms()
    print("encode / tails ms:", ms)
    assert tuple(cnt) == (6, 6) and blocks.shape == (6, 640) and len(ms) == 2 and all(m >= 0 for m in ms)
    assert not blocks.any()  # digital silence: s[0] = 0, index0 = 0, every code 0
    assert (out.cpu().numpy()[6 * 640:] == SENT_BYTE).all()
    for kw in (dict(max_batches=0), dict(rate=44100), dict(fmt=3)):
        with pytest.raises(pkg.MiError) as e:
            pkg.Pcm(np.ones(5), **{"max_batches": 2, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID
    pcm.close()


@gpu
def test_behind_the_demodulator(pkg):
    """1 stream x 2 AM channels x 8 batches of a gated mi_iqgen capture in two calls of 4: demodulator, gate (MI_GATE_ALL on row 0,
    MI_GATE_OPEN_TRAIL on row 1) and the PCM stage back to back on one stream, then the twin over the downloaded audio and index"""
    import torch
    calls = (4, 4)
    centre = 120000000
    dev = pkg.device_cfg(centerfreq=centre)
    offsets = (250000, -250000)
    chans = [pkg.channel_cfg(centre + o, squelch_threshold_dbfs=-45) for o in offsets]
    rows = len(chans)
    nbytes = (bytes_for_batches(dev, sum(calls)) + 255) // 256 * 256
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate * 2 * WAVE_BATCH // pm.WAVE_RATE,
                        carriers=[(offsets[0], 1, 3072, 1), (offsets[1], 1, 3072, 0)])
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, 1, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    rule = np.array([GATE_ALL, GATE_OPEN_TRAIL], np.uint8)
    gate = pkg.OutputGate(rule, max_batches=max(calls))
    outs, done = [], 0
    for fmt in (S16, IMA4):
        assert pkg.pcm_block_bytes(8000, fmt) in (2000, 640)
    stages = {fmt: pkg.Pcm(np.ones(rows), max_batches=max(calls), fmt=fmt) for fmt in (S16, IMA4)}
    for n in calls:  # (no host synchronisation between the demodulator, the gate and the stage)
        wo = torch.zeros((rows, n * WAVE_BATCH), dtype=torch.float32, device="cuda")
        ax = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
        gd = GateDest(rows, n)
        d_out = {fmt: torch.full(((rows * n + GUARD) * p.block_bytes,), SENT_BYTE, dtype=torch.uint8, device="cuda") for fmt, p in stages.items()}
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, nbytes, n, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        gate.process_device(wo.data_ptr(), n * WAVE_BATCH, ax.data_ptr(), n, n, gd.blocks.data_ptr(), gd.index.data_ptr(), gd.row_first.data_ptr(),
                            gd.count.data_ptr(), hip_stream=s)
        for fmt, p in stages.items():
            p.process_device(wo.data_ptr(), n * WAVE_BATCH, n, gd.index.data_ptr(), gd.count.data_ptr(), d_out[fmt].data_ptr(), hip_stream=s)
        got = {fmt: p.download(s) for fmt, p in stages.items()}
        outs.append((n, got, gate.download(s)[2], wo.cpu().numpy(), ax.cpu().numpy(), {f: o.cpu().numpy() for f, o in d_out.items()}))
        done += n
    d.close()
    gate.close()
    print("flags per row:", [bytes(np.concatenate([o[4][r] for o in outs])).decode() for r in range(rows)])
    peaks = [float(max(np.abs(o[3][r]).max() for o in outs)) for r in range(rows)]
    print("peak |audio| per row:", peaks)
    assert all(p > 0.0 for p in peaks), "a row's audio is digital silence: the capture should open both channels"
    for fmt, p in stages.items():
        state = None
        for i, (n, got, index, wo, ax, raw) in enumerate(outs):
            blocks, count = got[fmt]
            assert len(index) >= n and int(count[0]) == int(count[1]) == len(index) == len(blocks)  # (row 0 travels whole)
            want, state = pkg.pcm_plan_host(np.ones(rows), wo, index, state, 8000, fmt)
            model, _ = pcm_model(wo, index, None if i == 0 else prev, rate=8000, fmt=fmt)
            assert blocks.tobytes() == want.tobytes() == model.tobytes(), f"format {fmt}, call {i}"
            assert raw[fmt][:blocks.size].tobytes() == want.tobytes() and (raw[fmt][blocks.size:] == SENT_BYTE).all()
            prev = state
        assert p.state().tobytes() == state.tobytes()
        p.close()
