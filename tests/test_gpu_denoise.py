"""The noise reduction stage on the GPU (mi_denoise_*, csrc/denoise.hip) against the numpy restatement in denoise_model.py and
against its host twin mi_denoise_plan_host.

Every comparison is bit for bit: the plane and the state blob travel and are compared as bytes -- the transform's graph, the order of
the sums, the division and the clamp are part of the definition.  The output plane is filled with a sentinel before a call and is
laid out longer than the call; what the stage must not write -- a disabled row, anything behind the call's batches -- must still
hold the sentinel."""
import numpy as np
import pytest

import denoise_model as dm
from common import AGC_EXTRA
from denoise_model import FRAME, THREE_CLASSES, WAVE_BATCH, audio, denoise_model
from gate_model import gate_model
from test_denoise_model import SENT, classes_for

gpu = pytest.mark.gpu
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GATE_OPEN_TRAIL = 2
MAX_GRID = 512  # kMaxGrid of denoise.hip: more blocks than that and a workgroup strides on
DISTINCT = 5    # rows are independent: 70 rows are five distinct (audio, settings) pairs, and the model runs on those


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run_calls(pkg, wave, cfgs, cuts, what, masks=None, pad_in=0, pad_out=0, stream=None, twin_at=None, spread=1):
    """One stage over consecutive calls of the lengths `cuts`.  The input is laid out for `pad_in` more batches than the call (filled
    with 0.5: a stage that read them would write something else) and the output for `pad_out` more and four floats (the sentinel).
    cfgs: the rows' settings, or a list with those of each call (set_rows in between, as for masks, the enabled rows of each call).
    The plane against the model and the twin, the device's state before and after every call against theirs.  twin_at: that call is
    made by the host twin from the device's state blob, whose state goes back to the device.  spread: the device runs every row
    `spread` times over (rows r, r + rows, ...), and every copy must equal the model's row.  Returns the planes' call parts and the
    last state."""
    import torch
    rows = wave.shape[0]
    per_call = np.ndim(cfgs) == 3
    cfgs = cfgs if per_call else [cfgs] * len(cuts)
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    tile = lambda a: np.concatenate([np.asarray(a)] * spread)
    dn = pkg.Denoise(tile(masks[0]), tile(cfgs[0]), max_batches=max(cuts))
    q = stream if stream is not None else torch.cuda.current_stream()
    s = q.cuda_stream
    state, done, outs = dm.fresh_state(rows), 0, []
    for i, (n, en, cfg) in enumerate(zip(cuts, masks, cfgs)):
        if i and (en is not masks[i - 1] or cfg is not cfgs[i - 1]):
            dn.set_rows(None if en is masks[i - 1] else tile(en), None if cfg is cfgs[i - 1] else tile(cfg))
        in_stride, out_stride = (n + pad_in) * WAVE_BATCH, (n + pad_out) * WAVE_BATCH + 4
        w = np.full((rows, in_stride), np.float32(0.5))
        w[:, :n * WAVE_BATCH] = wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        blank = np.full((rows, out_stride), SENT)
        want, after = denoise_model(w, cfg, state, en, nbatches=n, out=blank)
        before = dn.state()
        assert before.tobytes() == tile(state).tobytes(), f"{what}, call {i}: state before"
        twin, twin_state = pkg.denoise_plan_host(en, w, cfg, before[:rows * dm.STATE.itemsize], nbatches=n, out=blank.copy())
        assert twin.tobytes() == want.tobytes() and twin_state.tobytes() == after.tobytes(), f"{what}, call {i}: the twin"
        if i == twin_at:
            dn.set_state(tile(twin_state.view(dm.STATE)))
        else:
            with torch.cuda.stream(q):
                d_w, d_out = to_dev(tile(w)), to_dev(tile(blank))
            dn.process_device(d_w.data_ptr(), in_stride, n, d_out.data_ptr(), out_stride, hip_stream=s)
            q.synchronize()
            got = d_out.cpu().numpy()
            expect = tile(want)
            if got.tobytes() != expect.tobytes():
                bad = np.argwhere(got.view(np.uint32) != expect.view(np.uint32))
                raise AssertionError(f"{what}, call {i} at batch {done}: {len(bad)} floats differ, the first at row {bad[0][0]}, float {bad[0][1]}: "
                                     f"{got[tuple(bad[0])]!r} for {expect[tuple(bad[0])]!r}")
        assert dn.state().tobytes() == tile(after).tobytes(), f"{what}, call {i}: state blob after"
        outs.append(want[:, :n * WAVE_BATCH])
        state, done = after, done + n
    dn.close()
    return outs, state


@gpu
@pytest.mark.parametrize("rows,nb,kind", [(1, 1, "one"), (1, 4, "one"), (5, 1, "three"), (5, 4, "per_row"), (70, 1, "three"), (70, 4, "per_row")])
def test_device_equals_model_and_twin(pkg, rows, nb, kind):
    """Every builder through a call of nb batches and one more batch behind it, whose history is the carried state.  1, 5 and 70 rows:
    one block, a handful, and 280 at four batches; one class, three, and one per distinct row.  70 rows are 14 copies of five."""
    base = min(rows, DISTINCT)
    cfg = classes_for(base, kind)
    for name in dm.BUILDERS:
        wave = audio(name, base, nb + 1)
        _, state = run_calls(pkg, wave, cfg, (nb, 1), f"{name}, {rows} rows, {nb} batches, {kind}", spread=rows // base)
        assert state["x"].tobytes() == wave[:, -FRAME:].tobytes()


@gpu
@pytest.mark.parametrize("cuts", [(12,), (5, 7), (1,) * 12])
def test_twelve_batches_and_their_cuts(pkg, cuts):
    """The stepping noise over 12 batches, and a batch behind them, at 70 rows -- 840 blocks on a grid of 512, so workgroups stride on
    --: m reads the carried rows and the call's scratch, and the bytes do not depend on how the calls were cut"""
    rows = DISTINCT
    assert 14 * rows * 12 > MAX_GRID
    cfg = classes_for(rows, "three")
    for name, spread in (("stepping_noise", 14), ("tx_after_silence", 1)):
        wave = audio(name, rows, 13)
        whole, whole_state = denoise_model(wave, cfg)
        outs, state = run_calls(pkg, wave, cfg, cuts + (1,), f"{name}, cuts {cuts}", spread=spread)
        assert np.concatenate(outs, axis=1).tobytes() == whole.tobytes() and state.tobytes() == whole_state.tobytes(), f"{name}, cuts {cuts}"


@gpu
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg):
    """rows 1 and 3 sit the second of four calls out -- their output rows are not written and their state keeps its bytes --; the
    second call also runs under other settings, one class per row, and the fourth under three classes again; the third call is made
    by the host twin from the device's blob and handed back with set_state; the fourth goes on from it"""
    rows = 5
    wave = audio("noise_mid", rows, 8)
    everyone = np.ones(rows, np.uint8)
    masks = [everyone, np.array([1, 0, 1, 0, 1], np.uint8), everyone, everyone]
    three, each = classes_for(rows, "three"), classes_for(rows, "per_row")
    _, state = run_calls(pkg, wave, [three, each, each, three], (2, 3, 1, 2), "set_rows", masks=masks, twin_at=2)
    assert state["x"].tobytes() == wave[:, -FRAME:].tobytes()
    d = pkg.Denoise(np.ones(2), max_batches=1)
    assert d.state().tobytes() == pkg.denoise_fresh_state(2).tobytes()
    for bad in (np.zeros(2 * 9196 - 4, np.uint8), np.zeros(3 * 9196, np.uint8)):
        with pytest.raises(pkg.MiError) as e:
            d.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID
    for bad in ([(12.0, 4.5), (40.5, 4.5)], [(12.0, 64.5), (12.0, 4.5)]):
        with pytest.raises(pkg.MiError) as e:
            d.set_rows(None, bad)
        assert e.value.code == pkg.MI_ERR_INVALID
    with pytest.raises(pkg.MiError) as e:
        d.set_rows(None, None)
    assert e.value.code == pkg.MI_ERR_INVALID
    d.close()


@gpu
def test_padded_unequal_strides_on_a_side_stream(pkg):
    """the input laid out for three batches more than the call and the output for one more, everything enqueued on a side stream
    behind the uploads: the carried samples come from the call's last batch, not from the end of the row"""
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    run_calls(pkg, audio("voice_in_noise", 5, 5), classes_for(5, "three"), (3, 2), "padded, side stream", pad_in=3, pad_out=1, stream=side)


@gpu
def test_timing_and_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    n = nb * WAVE_BATCH
    dn = pkg.Denoise([1, 1, 0], max_batches=nb)
    both = torch.zeros(2 * rows * (n + 4) + 8, dtype=torch.float32, device="cuda")
    wave, out = both.data_ptr(), both.data_ptr() + 4 * rows * (n + 4)
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=wave, row_stride=n + 4, d_out=out, out_stride=n + 4):
        dn.process_device(d_wave, row_stride, nbatches, d_out, out_stride, hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_wave=None), dict(d_out=None), dict(d_wave=wave + 4), dict(d_out=out + 8),
                dict(row_stride=n + 2), dict(out_stride=n + 2), dict(row_stride=n - 4), dict(out_stride=n - 4), dict(row_stride=WAVE_BATCH),
                dict(d_out=wave), dict(d_out=wave + 16), dict(d_out=out - 32), dict(d_wave=out + 4 * (3 * n + 8) - 16)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        dn.last_launch_ms()
    dn.set_timing(True)
    both[:] = float(SENT)
    both[:rows * (n + 4)] = 0.0
    call()
    torch.cuda.synchronize()
    ms = dn.last_launch_ms()
    print("floor / apply / tails ms:", ms)
    assert len(ms) == 3 and all(m >= 0 for m in ms)
    got = both.cpu().numpy()[rows * (n + 4):rows * (n + 4) * 2].reshape(rows, n + 4)
    assert (got[:2, :n].view(np.uint32) == 0).all() and (got[:2, n:] == SENT).all() and (got[2] == SENT).all()  # digital silence; row 2 is disabled
    for kw in (dict(max_batches=0), dict(rows_cfg=(-1.0, 4.5)), dict(rows_cfg=(40.5, 4.5)), dict(rows_cfg=(12.0, 65.0))):
        with pytest.raises(pkg.MiError) as e:
            pkg.Denoise(np.ones(5), **{"max_batches": 2, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID
    dn.close()


HISS_BINS = (slice(400, 460), slice(560, 1000))  # bins of 7.8125 Hz: 3.1 to 3.6 kHz and 4.4 to 7.8 kHz, clear of the capture's tone and its harmonics


@gpu
def test_chain_behind_the_demodulator(pkg):
    """The generated NFM capture of the tone finder's tests in three calls of 8 batches, with no host synchronisation inside a call:
    demodulator -> noise reduction (default row) -> voice band stage (300, 3400) -> output gate (MI_GATE_OPEN_TRAIL) -> PCM stage; the
    spectrum stage runs on the demodulator's plane and on the noise reduction's over the same index.  Every plane and the PCM bytes
    equal the host twins' chained on the same audio.  On the rows' travelling blocks from the second open second on, the power in the
    bins outside the voice's lines (HISS_BINS) is lower behind the stage than in front of it, summed over those blocks."""
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
    dn = pkg.Denoise(np.ones(rows), max_batches=max(calls))
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
        clean = torch.full((rows, stride), float(SENT), dtype=torch.float32, device="cuda")
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
        dn.process_device(wo.data_ptr(), stride, n, clean.data_ptr(), stride, hip_stream=s)
        vb.process_device(clean.data_ptr(), stride, n, filt.data_ptr(), stride, hip_stream=s)
        gate.process_device(filt.data_ptr(), stride, ax.data_ptr(), n, n, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(), count.data_ptr(),
                            hip_stream=s)
        pcm.process_device(filt.data_ptr(), stride, n, index.data_ptr(), count.data_ptr(), d_pcm.data_ptr(), hip_stream=s)
        for a, plane, rec, pw in zip(spec, (wo, clean), records, power):
            a.process_device(plane.data_ptr(), stride, n, index.data_ptr(), None, count.data_ptr(), rec.data_ptr(), d_power=pw.data_ptr(), hip_stream=s)
        got_pcm, _ = pcm.download(s)
        got_power = [a.download(s)[1] for a in spec]
        outs.append((n, wo.cpu().numpy(), ax.cpu().numpy(), clean.cpu().numpy(), filt.cpu().numpy(), gate.download(s)[2], got_pcm, got_power))
        done += n
    dn_state, vb_state = dn.state(), vb.state()
    for h in [d, dn, vb, gate, pcm] + spec:
        h.close()
    print("flags per row:", [bytes(np.concatenate([o[2][r] for o in outs])).decode() for r in range(rows)])
    state = model_state = vstate = pcm_state = None
    carried = np.zeros(rows, np.uint8)
    raw_sum = cut_sum = 0.0
    seen, checked = np.zeros(rows, int), 0
    for i, (n, wo, ax, clean, filt, index, got_pcm, got_power) in enumerate(outs):
        want, state = pkg.denoise_plan_host(np.ones(rows), wo, None, state)
        model, model_state = denoise_model(wo, None, model_state)
        assert clean.tobytes() == want.tobytes() == model.tobytes(), f"call {i}: the noise reduction's plane"
        want_filt, vstate = pkg.vband_plan_host(np.ones(rows), want, band, vstate)
        assert filt.tobytes() == want_filt.tobytes(), f"call {i}: the filtered plane"
        want_index, _, carried = gate_model(rule, ax, carried)
        assert np.array_equal(index, want_index), f"call {i}: the gate's index"
        want_pcm, pcm_state = pkg.pcm_plan_host(np.ones(rows), want_filt, index, pcm_state)
        assert got_pcm.tobytes() == want_pcm.tobytes(), f"call {i}: the PCM bytes"
        twin_power = [pkg.aspec_plan_host(rows, plane, index)[1] for plane in (wo, want)]
        for k, (row, batch) in enumerate(index):
            assert got_power[0][k].tobytes() == twin_power[0][k].tobytes() and got_power[1][k].tobytes() == twin_power[1][k].tobytes()
            seen[row] += 1
            if seen[row] > 8 and ax[row, batch] != ord(" "):  # (the row's second open second: the floor has its eight batches)
                raw, cut = (sum(float(p[k, b].astype(np.float64).sum()) for b in HISS_BINS) for p in got_power)
                print(f"call {i}, row {row}, batch {batch}: hiss bins at {10 * np.log10(max(cut, 1e-300) / max(raw, 1e-300)):.1f} dB of the plane in front")
                raw_sum, cut_sum, checked = raw_sum + raw, cut_sum + cut, checked + 1
    assert dn_state.tobytes() == state.tobytes() == model_state.tobytes() and vb_state.tobytes() == vstate.tobytes()
    assert checked >= 2, "the capture should keep a row open for more than a second"
    print(f"hiss bins over {checked} blocks: {10 * np.log10(cut_sum / raw_sum):.1f} dB")
    assert cut_sum < raw_sum
