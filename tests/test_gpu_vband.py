"""The voice band stage on the GPU (mi_vband_*, csrc/vband.hip) against the numpy restatement in vband_model.py and against its host
twin mi_vband_plan_host.

Every comparison is bit for bit: the filtered plane and the state blob travel and are compared as bytes -- the order of the filter's
sum and the clamp are part of the definition.  The output plane is filled with a sentinel before a call and is laid out longer than
the call; what the stage must not write -- a disabled row, anything behind the call's batches -- must still hold the sentinel."""
import numpy as np
import pytest

import vband_model as vm
from common import AGC_EXTRA
from gate_model import gate_model
from test_vband_model import SENT, classes_for
from vband_model import HISTORY, THREE_CLASSES, WAVE_BATCH, audio, vband_model

gpu = pytest.mark.gpu
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GATE_OPEN_TRAIL = 2
MAX_GRID = 2048  # kMaxGrid of vband.hip: more blocks than that and a workgroup strides on


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run_calls(pkg, wave, cfgs, cuts, what, masks=None, pad_in=0, pad_out=0, stream=None, twin_at=None):
    """One stage over consecutive calls of the lengths `cuts`.  The input is laid out for `pad_in` more batches than the call (filled
    with 0.5: a stage that read them would write something else) and the output for `pad_out` more and four floats (the sentinel).
    cfgs: the rows' settings, or a list with those of each call (set_rows in between, as for masks, the enabled rows of each call).
    The plane against the model and the twin, the device's state before and after every call against theirs.  twin_at: that call is
    made by the host twin from the device's state blob, whose state goes back to the device.  Returns the planes' call parts and the
    last state."""
    import torch
    rows = wave.shape[0]
    per_call = np.ndim(cfgs) == 3
    cfgs = cfgs if per_call else [cfgs] * len(cuts)
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    vb = pkg.Vband(masks[0], cfgs[0], max_batches=max(cuts))
    q = stream if stream is not None else torch.cuda.current_stream()
    s = q.cuda_stream
    state, done, outs = vm.fresh_state(rows), 0, []
    for i, (n, en, cfg) in enumerate(zip(cuts, masks, cfgs)):
        if i and (en is not masks[i - 1] or cfg is not cfgs[i - 1]):
            vb.set_rows(None if en is masks[i - 1] else en, None if cfg is cfgs[i - 1] else cfg)
        in_stride, out_stride = (n + pad_in) * WAVE_BATCH, (n + pad_out) * WAVE_BATCH + 4
        w = np.full((rows, in_stride), np.float32(0.5))
        w[:, :n * WAVE_BATCH] = wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        blank = np.full((rows, out_stride), SENT)
        want, after = vband_model(w, cfg, state, en, nbatches=n, out=blank)
        before = vb.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin, twin_state = pkg.vband_plan_host(en, w, cfg, before, nbatches=n, out=blank.copy())
        assert twin.tobytes() == want.tobytes() and twin_state.tobytes() == after.tobytes(), f"{what}, call {i}: the twin"
        if i == twin_at:
            vb.set_state(twin_state)
        else:
            with torch.cuda.stream(q):
                d_w, d_out = to_dev(w), to_dev(blank)
            vb.process_device(d_w.data_ptr(), in_stride, n, d_out.data_ptr(), out_stride, hip_stream=s)
            q.synchronize()
            got = d_out.cpu().numpy()
            if got.tobytes() != want.tobytes():
                bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                raise AssertionError(f"{what}, call {i} at batch {done}: {len(bad)} floats differ, the first at row {bad[0][0]}, float {bad[0][1]}: "
                                     f"{got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")
        assert vb.state().tobytes() == after.tobytes(), f"{what}, call {i}: state blob after"
        outs.append(want[:, :n * WAVE_BATCH])
        state, done = after, done + n
    vb.close()
    return outs, state


@gpu
@pytest.mark.parametrize("rows,nb,kind", [(1, 1, "one"), (1, 4, "one"), (5, 1, "one"), (5, 1, "three"), (5, 4, "three"), (5, 4, "per_row"), (70, 1, "three"),
                                          (70, 4, "per_row")])
def test_device_equals_model_and_twin(pkg, rows, nb, kind):
    """Every builder through a call of nb batches and one more batch behind it, whose history is the carried state.  1, 5 and 70 rows:
    one block, a handful, and more blocks than one wave of workgroups at four batches; one class, three, and one per row."""
    cfg = classes_for(rows, kind)
    for name in vm.BUILDERS:
        wave = audio(name, rows, nb + 1)
        if name == "subnormal" and rows > 5:  # (subnormal arithmetic is slow on the host: five such rows, silence on the others)
            wave = wave.copy()
            wave[5:] = 0.0
        _, state = run_calls(pkg, wave, cfg, (nb, 1), f"{name}, {rows} rows, {nb} batches, {kind}")
        assert state["x"].tobytes() == wave[:, -HISTORY:].tobytes()


@gpu
def test_call_cuts_give_identical_planes(pkg):
    """4 = 1 + 1 + 1 + 1 = 1 + 3: a block's bytes do not depend on whether its history came from the row's previous batch or from the
    carried samples"""
    rows, nb = 5, 4
    cfg = classes_for(rows, "three")
    for name in ("voice_hum", "square", "lone_last"):
        wave = audio(name, rows, nb)
        whole, whole_state = run_calls(pkg, wave, cfg, (nb,), f"{name}, one call")
        for cuts in ((1, 1, 1, 1), (1, 3)):
            outs, state = run_calls(pkg, wave, cfg, cuts, f"{name}, cuts {cuts}")
            assert np.concatenate(outs, axis=1).tobytes() == whole[0].tobytes() and state.tobytes() == whole_state.tobytes(), f"{name}, cuts {cuts}"


@gpu
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg):
    """rows 1 and 3 sit the second of four calls out -- their output rows are not written and their carried samples keep their bytes
    --; the second call also runs under other settings, one class per row, and the fourth under three classes again; the third call
    is made by the host twin from the device's blob and handed back with set_state; the fourth goes on from it"""
    rows = 5
    wave = audio("noise", rows, 8)
    everyone = np.ones(rows, np.uint8)
    masks = [everyone, np.array([1, 0, 1, 0, 1], np.uint8), everyone, everyone]
    three, each = classes_for(rows, "three"), classes_for(rows, "per_row")
    _, state = run_calls(pkg, wave, [three, each, each, three], (2, 3, 1, 2), "set_rows", masks=masks, twin_at=2)
    assert state["x"].tobytes() == wave[:, -HISTORY:].tobytes()
    v = pkg.Vband(np.ones(2), max_batches=1)
    for bad in (np.zeros(2 * 2040 - 4, np.uint8), np.zeros(3 * 2040, np.uint8)):
        with pytest.raises(pkg.MiError) as e:
            v.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID
    with pytest.raises(pkg.MiError) as e:
        v.set_rows(None, [(100, 2500), (100, 250)])
    assert e.value.code == pkg.MI_ERR_INVALID
    with pytest.raises(pkg.MiError) as e:
        v.set_rows(None, None)
    assert e.value.code == pkg.MI_ERR_INVALID
    v.close()


@gpu
def test_padded_unequal_strides_on_a_side_stream(pkg):
    """the input laid out for three batches more than the call and the output for one more, everything enqueued on a side stream
    behind the uploads: the carried samples come from the call's last batch, not from the end of the row"""
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    run_calls(pkg, audio("voice_hum", 5, 5), classes_for(5, "three"), (3, 2), "padded, side stream", pad_in=3, pad_out=1, stream=side)


@gpu
def test_more_blocks_than_the_grid(pkg):
    """70 rows x 30 batches = 2100 blocks on a grid capped at 2048: the workgroups that stride on filter blocks of row 68 and 69.
    Rows are independent, so the model runs on the three distinct (audio, settings) pairs and every row is compared with its pair's."""
    import torch
    rows, nb, distinct = 70, 30, 3
    assert rows * nb > MAX_GRID
    base = np.stack([audio("noise", 1, nb)[0], audio("voice_hum", 1, nb)[0], audio("lone_last", 1, nb)[0]])
    want3, after3 = vband_model(base, THREE_CLASSES)
    twin3, twin_state3 = pkg.vband_plan_host(np.ones(distinct), base, THREE_CLASSES)
    assert twin3.tobytes() == want3.tobytes() and twin_state3.tobytes() == after3.tobytes()
    pick = np.arange(rows) % distinct
    vb = pkg.Vband(np.ones(rows), [THREE_CLASSES[p] for p in pick], max_batches=nb)
    d_w = to_dev(base[pick])
    d_out = torch.full((rows, nb * WAVE_BATCH), float(SENT), dtype=torch.float32, device="cuda")
    vb.process_device(d_w.data_ptr(), nb * WAVE_BATCH, nb, d_out.data_ptr(), nb * WAVE_BATCH, hip_stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    for r in range(rows):
        assert got[r].tobytes() == want3[pick[r]].tobytes(), f"row {r}"
    assert vb.state().tobytes() == after3[pick].tobytes()
    vb.close()


@gpu
def test_timing_and_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    n = nb * WAVE_BATCH
    vb = pkg.Vband([1, 1, 0], max_batches=nb)
    both = torch.zeros(2 * rows * (n + 4) + 8, dtype=torch.float32, device="cuda")
    wave, out = both.data_ptr(), both.data_ptr() + 4 * rows * (n + 4)
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=wave, row_stride=n + 4, d_out=out, out_stride=n + 4):
        vb.process_device(d_wave, row_stride, nbatches, d_out, out_stride, hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_wave=None), dict(d_out=None), dict(d_wave=wave + 4), dict(d_out=out + 8),
                dict(row_stride=n + 2), dict(out_stride=n + 2), dict(row_stride=n - 4), dict(out_stride=n - 4), dict(row_stride=WAVE_BATCH),
                dict(d_out=wave), dict(d_out=wave + 16), dict(d_out=out - 32), dict(d_wave=out + 4 * (3 * n + 8) - 16)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        vb.last_launch_ms()
    vb.set_timing(True)
    both[:] = float(SENT)
    both[:rows * (n + 4)] = 0.0
    call()
    torch.cuda.synchronize()
    ms = vb.last_launch_ms()
    print("filter / tails ms:", ms)
    assert len(ms) == 2 and all(m >= 0 for m in ms)
    got = both.cpu().numpy()[rows * (n + 4):rows * (n + 4) * 2].reshape(rows, n + 4)
    assert (got[:2, :n].view(np.uint32) == 0).all() and (got[:2, n:] == SENT).all() and (got[2] == SENT).all()  # digital silence; row 2 is disabled
    for kw in (dict(max_batches=0), dict(rows_cfg=(49, 2500)), dict(rows_cfg=(100, 7801)), dict(rows_cfg=(2400, 2500))):
        with pytest.raises(pkg.MiError) as e:
            pkg.Vband(np.ones(5), **{"max_batches": 2, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID
    vb.close()


@gpu
def test_chain_behind_the_demodulator(pkg):
    """The generated NFM + 100 Hz CTCSS capture of the tone finder's tests in three calls of 8 batches, with no host synchronisation
    inside a call: demodulator -> voice band stage (300, 3400) -> output gate (MI_GATE_OPEN_TRAIL) -> PCM stage, gate and PCM stage on
    the filtered plane; the spectrum stage runs on the filtered and on the unfiltered plane over the same index.  The filtered plane
    and the PCM bytes equal the host twins' chained on the same audio, and on the row with the tone the bins around 100 Hz (11 .. 14 of
    7.8125 Hz) of every travelling block lie at least 60 dB below the same bins of the unfiltered plane: the filter's own bound is 70
    dB, and 10 dB cover the Hann window's leakage from the voice band.  The two host twins on the CPU oracle's audio of this capture
    give -87.6 to -92.1 dB per block."""
    import torch
    from test_tones_model import e2e_setup
    calls = (8, 8, 8)
    dev, chans, cfg, nbytes = e2e_setup(pkg)
    rows = len(chans)
    band = (300, 3400)
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, 1, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    vb = pkg.Vband(np.ones(rows), band, max_batches=max(calls))
    rule = np.full(rows, GATE_OPEN_TRAIL, np.uint8)
    gate = pkg.OutputGate(rule, max_batches=max(calls))
    pcm = pkg.Pcm(np.ones(rows), max_batches=max(calls))
    spec = [pkg.Aspec(rows, max_batches=max(calls)) for _ in range(2)]
    outs, done = [], 0
    for n in calls:
        stride, cap = n * WAVE_BATCH, rows * n
        wo = torch.zeros((rows, stride), dtype=torch.float32, device="cuda")
        ax = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
        filt = torch.full((rows, stride), float(SENT), dtype=torch.float32, device="cuda")
        blocks = torch.empty((cap, WAVE_BATCH), dtype=torch.float32, device="cuda")
        index = torch.full((cap, 2), SENT32, dtype=torch.int32, device="cuda")
        row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
        count = torch.zeros(2, dtype=torch.int32, device="cuda")
        d_pcm = torch.zeros(cap * pcm.block_bytes, dtype=torch.uint8, device="cuda")
        records = [torch.zeros(cap * pkg.ASPEC_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda") for _ in spec]
        power = [torch.zeros((cap, pkg.ASPEC_BINS), dtype=torch.float32, device="cuda") for _ in spec]
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, nbytes, n, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        vb.process_device(wo.data_ptr(), stride, n, filt.data_ptr(), stride, hip_stream=s)
        gate.process_device(filt.data_ptr(), stride, ax.data_ptr(), n, n, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(), count.data_ptr(),
                            hip_stream=s)
        pcm.process_device(filt.data_ptr(), stride, n, index.data_ptr(), count.data_ptr(), d_pcm.data_ptr(), hip_stream=s)
        for a, plane, rec, pw in zip(spec, (wo, filt), records, power):
            a.process_device(plane.data_ptr(), stride, n, index.data_ptr(), None, count.data_ptr(), rec.data_ptr(), d_power=pw.data_ptr(), hip_stream=s)
        got_pcm, got_count = pcm.download(s)
        got_power = [a.download(s)[1] for a in spec]
        outs.append((n, wo.cpu().numpy(), ax.cpu().numpy(), filt.cpu().numpy(), gate.download(s)[2], got_pcm, got_power))
        done += n
    vb_state = vb.state()
    for h in [d, vb, gate, pcm] + spec:
        h.close()
    print("flags per row:", [bytes(np.concatenate([o[2][r] for o in outs])).decode() for r in range(rows)])
    state = pcm_state = None
    carried = np.zeros(rows, np.uint8)
    worst, checked = -np.inf, 0
    for i, (n, wo, ax, filt, index, got_pcm, got_power) in enumerate(outs):
        want, state = pkg.vband_plan_host(np.ones(rows), wo, band, state)
        model, _ = vband_model(wo, band, None if i == 0 else prev)
        assert filt.tobytes() == want.tobytes() == model.tobytes(), f"call {i}: the filtered plane"
        want_index, _, carried = gate_model(rule, ax, carried)
        assert np.array_equal(index, want_index), f"call {i}: the gate's index"
        want_pcm, pcm_state = pkg.pcm_plan_host(np.ones(rows), want, index, pcm_state)
        assert got_pcm.tobytes() == want_pcm.tobytes(), f"call {i}: the PCM bytes"
        twin_power = [pkg.aspec_plan_host(rows, plane, index)[1] for plane in (wo, want)]
        for k, (row, batch) in enumerate(index):
            assert got_power[0][k].tobytes() == twin_power[0][k].tobytes() and got_power[1][k].tobytes() == twin_power[1][k].tobytes()
            if row == 0:
                raw, cut = (float(p[k, 11:15].astype(np.float64).sum()) for p in got_power)
                db = 10 * np.log10(max(cut, 1e-300) / raw)
                print(f"call {i}, row 0, batch {batch}: bins 11 .. 14 at {db:.1f} dB of the unfiltered plane's")
                assert db <= -60.0
                worst, checked = max(worst, db), checked + 1
        prev = state
    assert checked >= 8, "the capture should open the row with the tone for half of its batches"
    assert vb_state.tobytes() == state.tobytes()
    print(f"worst of {checked} blocks: {worst:.1f} dB")
