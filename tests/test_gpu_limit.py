"""The peak limiter stage on the GPU (mi_limit_*, csrc/limit.hip) against the numpy restatement in limit_model.py and against its host
twin mi_limit_plan_host.

Every comparison is bit for bit: the limited plane and the state blob travel and are compared as bytes -- the order of the gain's sum,
the division and the clamp are part of the definition, and no byte may depend on whether a block took the transparent path.  The
output plane is filled with a sentinel before a call and is laid out longer than the call; what the stage must not write -- a
disabled row, anything behind the call's batches -- must still hold the sentinel.  The input behind the call holds 5.0: a stage that
read it would turn the gain down."""
import numpy as np
import pytest

import limit_model as lm
from limit_model import CEILING, HISTORY, WAVE_BATCH, audio, limit_model, settings_for
from test_limit_model import CUTS, SENT

gpu = pytest.mark.gpu
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GATE_ALL = 3
MAX_GRID = 2048  # kMaxGrid of limit.hip: more blocks than that and a workgroup strides on
PAD_VALUE = np.float32(5.0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run_calls(pkg, wave, cfgs, cuts, what, masks=None, pad_in=0, pad_out=0, stream=None, twin_at=None):
    """One stage over consecutive calls of the lengths `cuts`.  The input is laid out for `pad_in` more batches than the call (filled
    with 5.0) and the output for `pad_out` more and four floats (the sentinel).  cfgs: the rows' settings, or a list with those of
    each call (set_rows in between, as for masks, the enabled rows of each call).  The plane against the model and the twin, the
    device's state before and after every call against theirs.  twin_at: that call is made by the host twin from the device's state
    blob, whose state goes back to the device.  Returns the planes' call parts and the last state."""
    import torch
    rows = wave.shape[0]
    per_call = np.ndim(cfgs) == 3
    cfgs = cfgs if per_call else [cfgs] * len(cuts)
    masks = [np.ones(rows, np.uint8)] * len(cuts) if masks is None else masks
    lim = pkg.Limit(masks[0], cfgs[0], max_batches=max(cuts))
    q = stream if stream is not None else torch.cuda.current_stream()
    s = q.cuda_stream
    state, done, outs = lm.fresh_state(rows), 0, []
    for i, (n, en, cfg) in enumerate(zip(cuts, masks, cfgs)):
        if i and (en is not masks[i - 1] or cfg is not cfgs[i - 1]):
            lim.set_rows(None if en is masks[i - 1] else en, None if cfg is cfgs[i - 1] else cfg)
        in_stride, out_stride = (n + pad_in) * WAVE_BATCH, (n + pad_out) * WAVE_BATCH + 4
        w = np.full((rows, in_stride), PAD_VALUE)
        w[:, :n * WAVE_BATCH] = wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        blank = np.full((rows, out_stride), SENT)
        want, after = limit_model(w, cfg, state, en, nbatches=n, out=blank)
        before = lim.state()
        assert before.tobytes() == state.tobytes(), f"{what}, call {i}: state before"
        twin, twin_state = pkg.limit_plan_host(en, w, cfg, before, nbatches=n, out=blank.copy())
        assert twin.tobytes() == want.tobytes() and twin_state.tobytes() == after.tobytes(), f"{what}, call {i}: the twin"
        if i == twin_at:
            lim.set_state(twin_state)
        else:
            with torch.cuda.stream(q):
                d_w, d_out = to_dev(w), to_dev(blank)
            lim.process_device(d_w.data_ptr(), in_stride, n, d_out.data_ptr(), out_stride, hip_stream=s)
            q.synchronize()
            got = d_out.cpu().numpy()
            if got.tobytes() != want.tobytes():
                bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                raise AssertionError(f"{what}, call {i} at batch {done}: {len(bad)} floats differ, the first at row {bad[0][0]}, float {bad[0][1]}: "
                                     f"{got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}")
        assert lim.state().tobytes() == after.tobytes(), f"{what}, call {i}: state blob after"
        outs.append(want[:, :n * WAVE_BATCH])
        state, done = after, done + n
    lim.close()
    return outs, state


@gpu
@pytest.mark.parametrize("rows,nb,kind", [(1, 1, "one"), (1, 4, "one"), (5, 1, "one"), (5, 1, "three"), (5, 4, "three"), (5, 4, "per_row"), (70, 1, "three"),
                                          (70, 4, "per_row")])
def test_device_equals_model_and_twin(pkg, rows, nb, kind):
    """Every builder through a call of nb batches and one more batch behind it, whose history is the carried state.  1, 5 and 70 rows:
    one block, a handful, and more blocks than one wave of workgroups at four batches; a builder's own settings, three settings in
    turn, and one per row."""
    for name in lm.BUILDERS:
        wave = audio(name, rows, nb + 1)
        _, state = run_calls(pkg, wave, settings_for(name, rows, kind), (nb, 1), f"{name}, {rows} rows, {nb} batches, {kind}")
        assert state["x"].tobytes() == wave[:, -HISTORY:].tobytes()


@gpu
def test_call_cuts_give_identical_planes(pkg):
    """4 = 1 + 3 = 2 + 1 + 1: a block's bytes do not depend on whether its history came from the row's previous batch or from the
    carried samples"""
    rows, nb = 5, 4
    for name in ("four_voices", "loud_noise", "square", "lone_1999", "peaks_1024_apart", "quiet_noise"):
        cfg = settings_for(name, rows, "three")
        wave = audio(name, rows, nb)
        whole = None
        for cuts in CUTS:
            outs, state = run_calls(pkg, wave, cfg, cuts, f"{name}, cuts {cuts}")
            if whole is None:
                whole, whole_state = outs[0], state
            assert np.concatenate(outs, axis=1).tobytes() == whole.tobytes() and state.tobytes() == whole_state.tobytes(), f"{name}, cuts {cuts}"


@gpu
def test_set_rows_between_calls_and_the_state_through_the_host_twin(pkg):
    """rows 1 and 3 sit the second of four calls out -- their output rows are not written and their carried samples keep their bytes
    --; the second call also runs under other settings, one per row, so that the carried samples count under another pregain, and the
    fourth under three settings again; the third call is made by the host twin from the device's blob and handed back with
    set_state; the fourth goes on from it"""
    rows = 5
    wave = audio("four_voices", rows, 8)
    everyone = np.ones(rows, np.uint8)
    masks = [everyone, np.array([1, 0, 1, 0, 1], np.uint8), everyone, everyone]
    three, each = settings_for("four_voices", rows, "three"), settings_for("four_voices", rows, "per_row")
    _, state = run_calls(pkg, wave, [three, each, each, three], (2, 3, 1, 2), "set_rows", masks=masks, twin_at=2)
    assert state["x"].tobytes() == wave[:, -HISTORY:].tobytes()
    lim = pkg.Limit(np.ones(2), max_batches=1)
    for bad in (np.zeros(2 * 4344 - 4, np.uint8), np.zeros(3 * 4344, np.uint8)):
        with pytest.raises(pkg.MiError) as e:
            lim.set_state(bad)
        assert e.value.code == pkg.MI_ERR_INVALID
    with pytest.raises(pkg.MiError) as e:
        lim.set_rows(None, [(1.0, 0.5), (1.0, 0.05)])
    assert e.value.code == pkg.MI_ERR_INVALID
    with pytest.raises(pkg.MiError) as e:
        lim.set_rows(None, None)
    assert e.value.code == pkg.MI_ERR_INVALID
    lim.close()


@gpu
def test_padded_unequal_strides_on_a_side_stream(pkg):
    """the input laid out for three batches more than the call and the output for one more, everything enqueued on a side stream
    behind the uploads: the carried samples come from the call's last batch, not from the end of the row"""
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    run_calls(pkg, audio("four_voices", 5, 5), settings_for("four_voices", 5, "three"), (3, 2), "padded, side stream", pad_in=3, pad_out=1, stream=side)


@gpu
def test_more_blocks_than_the_grid(pkg):
    """70 rows x 30 batches = 2100 blocks on a grid capped at 2048: the workgroups that stride on limit blocks of row 68 and 69, behind
    a first block that may have taken the other path.  Rows are independent, so the model runs on the three distinct (audio,
    settings) pairs and every row is compared with its pair's."""
    import torch
    rows, nb, distinct = 70, 30, 3
    assert rows * nb > MAX_GRID
    base = np.stack([audio("loud_noise", 1, nb)[0], audio("voice", 1, nb)[0], audio("peaks_1024_apart", 1, nb)[0]])
    want3, after3 = limit_model(base, lm.THREE_SETTINGS)
    twin3, twin_state3 = pkg.limit_plan_host(np.ones(distinct), base, lm.THREE_SETTINGS)
    assert twin3.tobytes() == want3.tobytes() and twin_state3.tobytes() == after3.tobytes()
    pick = np.arange(rows) % distinct
    lim = pkg.Limit(np.ones(rows), [lm.THREE_SETTINGS[p] for p in pick], max_batches=nb)
    d_w = to_dev(base[pick])
    d_out = torch.full((rows, nb * WAVE_BATCH), float(SENT), dtype=torch.float32, device="cuda")
    lim.process_device(d_w.data_ptr(), nb * WAVE_BATCH, nb, d_out.data_ptr(), nb * WAVE_BATCH, hip_stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    for r in range(rows):
        assert got[r].tobytes() == want3[pick[r]].tobytes(), f"row {r}"
    assert lim.state().tobytes() == after3[pick].tobytes()
    lim.close()


@gpu
def test_one_slow_block_among_many(pkg):
    """12 rows x 6 batches under the ceiling but for one sample: the block that holds it and the block behind it, which reaches it
    through its history, take the slow path, every other block the transparent one; the plane is the model's all the same"""
    rows, nb = 12, 6
    wave = np.tile(audio("quiet_noise", 1, nb), (rows, 1))
    wave[7, 3 * WAVE_BATCH + 1500] = 1.75
    run_calls(pkg, wave, None, (nb,), "one slow block")
    want, _ = limit_model(wave)
    delayed = np.concatenate([np.zeros((rows, lm.LOOKAHEAD), np.float32), wave[:, :-lm.LOOKAHEAD]], axis=1)
    moved = np.flatnonzero((want != delayed).any(axis=0))
    assert (want[np.arange(rows) != 7] == delayed[np.arange(rows) != 7]).all() and moved.min() >= 3 * WAVE_BATCH and moved.max() < 5 * WAVE_BATCH


@gpu
def test_timing_and_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    n = nb * WAVE_BATCH
    lim = pkg.Limit([1, 1, 0], max_batches=nb)
    both = torch.zeros(2 * rows * (n + 4) + 8, dtype=torch.float32, device="cuda")
    wave, out = both.data_ptr(), both.data_ptr() + 4 * rows * (n + 4)
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=wave, row_stride=n + 4, d_out=out, out_stride=n + 4):
        lim.process_device(d_wave, row_stride, nbatches, d_out, out_stride, hip_stream=s)

    null, count, short = "NULL argument", "nbatches outside 1 .. max_batches", "a row stride is shorter than the call"
    align = "the input plane and the output must be 16-byte aligned with row strides that are multiples of 4 floats"
    overlap = "the output overlaps the input plane"
    for bad, text in ((dict(nbatches=0), count), (dict(nbatches=nb + 1), count), (dict(d_wave=None), null), (dict(d_out=None), null), (dict(d_wave=wave + 4), align),
                      (dict(d_out=out + 8), align), (dict(row_stride=n + 2), align), (dict(out_stride=n + 2), align), (dict(row_stride=n - 4), short),
                      (dict(out_stride=n - 4), short), (dict(row_stride=WAVE_BATCH), short), (dict(d_out=wave), overlap), (dict(d_out=wave + 16), overlap),
                      (dict(d_out=out - 32), overlap), (dict(d_wave=out + 4 * (3 * n + 8) - 16), overlap)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID and str(e.value).endswith(text), bad
    with pytest.raises(pkg.MiError):
        lim.last_launch_ms()
    lim.set_timing(True)
    both[:] = float(SENT)
    both[:rows * (n + 4)] = 0.0
    call()
    torch.cuda.synchronize()
    ms = lim.last_launch_ms()
    print("limit / tails ms:", ms)
    assert len(ms) == 2 and all(m >= 0 for m in ms)
    got = both.cpu().numpy()[rows * (n + 4):rows * (n + 4) * 2].reshape(rows, n + 4)
    assert (got[:2, :n].view(np.uint32) == 0).all() and (got[:2, n:] == SENT).all() and (got[2] == SENT).all()  # digital silence; row 2 is disabled
    for kw in (dict(max_batches=0), dict(rows_cfg=(0.0, 0.5)), dict(rows_cfg=(1.0, 1.5)), dict(rows_cfg=(float("nan"), 0.5)), dict(rows_cfg=(1.0, float("inf")))):
        with pytest.raises(pkg.MiError) as e:
            pkg.Limit(np.ones(5), **{"max_batches": 2, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID
    lim.close()


CHAIN_MIX = [(0, 4.0, 0.0), (1, 4.0, 0.0)]  # both rows of the capture open together; four times their sum passes +-1


@gpu
def test_chain_mixer_limiter_pcm(pkg):
    """The generated NFM + 100 Hz CTCSS capture of the voice band's chain test in three calls of 8 batches, with no host
    synchronisation inside a call: demodulator -> mixer (both rows, which open together, at an ampfactor of 4) -> limiter on the
    mixer's left plane of one row -> output gate (every batch) -> PCM stage; a second PCM stage encodes the mixer's plane as it is.
    The mixer's sum exceeds 1.0 somewhere; the limited plane equals the model's and the twin's on the mixer's plane and stays within
    the ceiling; the PCM blocks equal pcm_model's on the limited plane; and the chain without the limiter gives other PCM bytes.
    The count of saturated int16 samples on either side is printed, not asserted."""
    import torch
    from common import AGC_EXTRA
    from pcm_model import pcm_model
    from test_gpu_mixer import Dest as MixDest
    from test_tones_model import e2e_setup
    calls = (8, 8, 8)
    dev, chans, cfg, nbytes = e2e_setup(pkg)
    rows = len(chans)
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, 1, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    mixer = pkg.Mixer(CHAIN_MIX)
    assert not mixer.stereo
    lim = pkg.Limit([1], max_batches=max(calls))
    gate = pkg.OutputGate([GATE_ALL], max_batches=max(calls))
    pcm = [pkg.Pcm([1], max_batches=max(calls)) for _ in range(2)]  # behind the limiter, and on the mixer's plane as it is
    outs, done = [], 0
    for n in calls:
        stride = n * WAVE_BATCH
        wo = torch.zeros((rows, stride), dtype=torch.float32, device="cuda")
        ax = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
        mix = MixDest(n)
        limited = torch.full((1, stride + 4), float(SENT), dtype=torch.float32, device="cuda")
        blocks = torch.empty((n, WAVE_BATCH), dtype=torch.float32, device="cuda")
        index = torch.full((n, 2), SENT32, dtype=torch.int32, device="cuda")
        row_first = torch.empty(2, dtype=torch.int32, device="cuda")
        count = torch.zeros(2, dtype=torch.int32, device="cuda")
        d_pcm = [torch.zeros(n * p.block_bytes, dtype=torch.uint8, device="cuda") for p in pcm]
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, nbytes, n, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        mixer.process_device(wo.data_ptr(), stride, ax.data_ptr(), n, n, mix.left.data_ptr(), mix.right.data_ptr(), mix.out.data_ptr(), hip_stream=s)
        lim.process_device(mix.left.data_ptr(), stride, n, limited.data_ptr(), stride + 4, hip_stream=s)
        gate.process_device(limited.data_ptr(), stride + 4, mix.out.data_ptr(), n, n, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(), count.data_ptr(),
                            hip_stream=s)
        pcm[0].process_device(limited.data_ptr(), stride + 4, n, index.data_ptr(), count.data_ptr(), d_pcm[0].data_ptr(), hip_stream=s)
        pcm[1].process_device(mix.left.data_ptr(), stride, n, index.data_ptr(), count.data_ptr(), d_pcm[1].data_ptr(), hip_stream=s)
        got_pcm = [p.download(s)[0] for p in pcm]  # (the first wait of the call)
        left = mix.left.cpu().numpy().view(np.float32)[:stride].reshape(1, stride)
        outs.append((n, ax.cpu().numpy(), left, limited.cpu().numpy(), gate.download(s)[2], got_pcm))
        done += n
    lim_state = lim.state()
    for h in [d, mixer, lim, gate] + pcm:
        h.close()
    print("flags per row:", [bytes(np.concatenate([o[1][r] for o in outs])).decode() for r in range(rows)])
    state = model_state = None
    pcm_state = [None, None]
    peak_in = peak_out = 0.0
    saturated = [0, 0]
    for i, (n, ax, left, limited, index, got_pcm) in enumerate(outs):
        blank = np.full(limited.shape, SENT)
        want, state = pkg.limit_plan_host([1], left, None, state, nbatches=n, out=blank)
        model, model_state = limit_model(left, None, model_state, nbatches=n, out=blank)
        assert limited.tobytes() == want.tobytes() == model.tobytes(), f"call {i}: the limited plane, or the sentinel behind it"
        assert state.tobytes() == model_state.tobytes()
        assert np.array_equal(index, np.stack([np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32)], axis=1)), f"call {i}: the gate's index"
        for j, plane in enumerate((want[:, :n * WAVE_BATCH], left)):
            want_pcm, pcm_state[j] = pcm_model(plane, index, pcm_state[j])
            assert got_pcm[j].tobytes() == want_pcm.tobytes(), f"call {i}: the PCM bytes {'behind the limiter' if j == 0 else 'of the mixer as it is'}"
            saturated[j] += int((np.abs(got_pcm[j].view("<i2").astype(np.int32)) >= 32767).sum())
        peak_in, peak_out = max(peak_in, float(np.abs(left).max())), max(peak_out, float(np.abs(want[:, :n * WAVE_BATCH]).max()))
    assert lim_state.tobytes() == state.tobytes()
    print(f"mixer's peak {peak_in:.3f}, limited peak {peak_out:.6f}; saturated PCM samples: {saturated[0]} behind the limiter, {saturated[1]} without it")
    assert peak_in > 1.0, "both rows open at an ampfactor of 4 should pass 1.0"
    assert peak_out <= CEILING
    assert b"".join(o[5][0].tobytes() for o in outs) != b"".join(o[5][1].tobytes() for o in outs)
