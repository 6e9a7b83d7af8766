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


CHAIN_BAND, CHAIN_WINDOW, CHAIN_TONE = (300, 3400), 3200, 12  # tone 12 of the table is 100.0 Hz; at 3200 samples it has a k of its own (20)
CHAIN_MIX = [(0, 1.0, -0.5), (1, 0.5, 0.5)]
# The 100.0 Hz Goertzel power of the filtered plane's windows relative to the unfiltered plane's, row 0, from the host twins
# (mi_vband_plan_host into mi_tones_plan_host, window 3200) on the CPU oracle's audio of the capture, which opens batches 12 .. 23
# and so completes seven windows: -43.4 dB in the window that begins with the squelch's opening -- the filter's 510 samples of history
# reach back into the closed batch, and the step at the opening rings through the highpass -- and -84.6 to -87.6 dB in the six whose
# history lies in open batches too.  test_chain_tone_figures_on_the_oracle holds these to 0.1 dB; the device test asserts 10 dB more.
CHAIN_WORST_DB, CHAIN_SETTLED_DB = -43.4, (-87.6, -84.6)


def chain_tone_ratios(calls, flags, filtered, unfiltered):
    """[(first sample, dB, settled)] of row 0's windows that lie wholly in open batches: 10 log10 of the filtered records' power of
    CHAIN_TONE over the unfiltered records' of the same window.  calls: batches per call; flags [rows][all batches]; filtered and
    unfiltered: per call (records, powers, row_first_record).  settled: the 510 samples the filter carries in front of the window
    lie in open batches as well."""
    out, done = [], 0
    is_open = flags[0] != ord(" ")
    for n, (rf, pf, ff), (ru, pu, fu) in zip(calls, filtered, unfiltered):
        assert ff[0] == fu[0] == 0 and ff[1] == fu[1] and rf["seq"].tolist() == ru["seq"].tolist() and rf["end_sample"].tolist() == ru["end_sample"].tolist()
        for k in range(ff[1]):
            end = (done + int(rf[k]["end_batch"])) * WAVE_BATCH + int(rf[k]["end_sample"])
            first = end - CHAIN_WINDOW + 1
            if first < 0 or not is_open[first // WAVE_BATCH:end // WAVE_BATCH + 1].all():
                continue
            settled = first >= vm.HISTORY and bool(is_open[(first - vm.HISTORY) // WAVE_BATCH])
            assert pu[k, CHAIN_TONE] > 0
            out.append((first, float(10 * np.log10(max(float(pf[k, CHAIN_TONE]), 1e-300) / float(pu[k, CHAIN_TONE]))), settled))
        done += n
    return out


def test_chain_tone_figures_on_the_oracle(pkg):
    """(no GPU) where CHAIN_WORST_DB and CHAIN_SETTLED_DB come from: the capture through the CPU oracle, then the two host twins"""
    from common import oracle_run
    from test_tones_model import E2E_BATCHES, e2e_setup
    dev, chans, cfg, nbytes = e2e_setup(pkg)
    n, wo, axc, _ = oracle_run(dev, chans, pkg.iqgen_host(cfg, 0, 0, nbytes // 2), E2E_BATCHES)
    assert n == E2E_BATCHES
    filt, _ = pkg.vband_plan_host(np.ones(len(chans)), wo, CHAIN_BAND)
    f, u = (pkg.tones_plan_host(np.ones(len(chans)), axc, plane, None, CHAIN_WINDOW) for plane in (filt, wo))
    ratios = chain_tone_ratios((n,), axc, [(f[0], f[1], f[2])], [(u[0], u[1], u[2])])
    print("flags:", bytes(axc[0]).decode(), " windows (first sample, dB, settled):", [(a, round(b, 2), c) for a, b, c in ratios])
    settled = [db for _, db, s in ratios if s]
    assert len(ratios) == 7 and len(settled) == 6
    assert abs(max(db for _, db, _ in ratios) - CHAIN_WORST_DB) < 0.1
    assert abs(min(settled) - CHAIN_SETTLED_DB[0]) < 0.1 and abs(max(settled) - CHAIN_SETTLED_DB[1]) < 0.1


@gpu
def test_filtered_plane_into_the_splitter_the_tone_finder_and_the_mixer(pkg):
    """The generated NFM + 100 Hz CTCSS capture in three calls of 8 batches, with no host synchronisation inside a call: demodulator ->
    voice band stage (300, 3400) -> splitter, tone finder (window 3200) and mixer, all three on the filtered plane; a second tone
    finder reads the unfiltered plane over the same flags.  The filtered plane is laid out two batches and four floats longer than
    the call and the consumers are handed that out_stride as their row_stride; the padding holds a sentinel that must survive.
    Expected values come from the host side alone, on the audio and flags the demodulator returned: mi_vband_plan_host chained into
    mi_tx_plan_host and mi_tones_plan_host, and the oracle's ao_mixer_run with mixer_model.numpy_mixer; records, powers, left /
    right / flags and the three state blobs are compared as bytes.

    One physical assertion, on the row with the tone: the 100.0 Hz Goertzel power of the filtered plane's windows relative to the
    unfiltered plane's.  The host twins on the CPU oracle's audio of this capture (test_chain_tone_figures_on_the_oracle) give -43.4
    dB for the window that begins with the squelch's opening and -84.6 to -87.6 dB for the six windows whose filter history lies in
    open batches too; asserted here are those worst values plus 10 dB -- the Goertzel window leaks voice-band energy into the bin,
    and the device's audio is not the oracle's to the bit -- over at least 4 windows.  The vote on the filtered plane is printed, not
    asserted: it is relative among the 51 tones, and a highpass that lowers them alike may leave it unchanged."""
    import torch
    import libs
    from mixer_model import numpy_mixer
    from test_gpu_mixer import Dest as MixDest
    from test_gpu_tones import Dest as TonesDest, check as tones_check, tones_call
    from test_gpu_txsplit import Dest as TxDest, check as tx_check, tx_call
    from test_tones_model import e2e_setup
    calls = (8, 8, 8)
    dev, chans, cfg, nbytes = e2e_setup(pkg)
    rows = len(chans)
    ones = np.ones(rows, np.uint8)
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, 1, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    vb = pkg.Vband(ones, CHAIN_BAND, max_batches=max(calls))
    tx = pkg.TxSplit(ones, max_batches=max(calls))
    tn = [pkg.Tones(ones, max_batches=max(calls), window=CHAIN_WINDOW) for _ in range(2)]  # the filtered plane, the unfiltered plane
    mixer = pkg.Mixer(CHAIN_MIX)
    assert mixer.stereo
    outs, done = [], 0
    for n in calls:
        stride, out_stride = n * WAVE_BATCH, (n + 2) * WAVE_BATCH + 4
        wo = torch.zeros((rows, stride), dtype=torch.float32, device="cuda")
        ax = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
        filt = torch.full((rows, out_stride), float(SENT), dtype=torch.float32, device="cuda")
        tx_dest = TxDest(rows, rows * (n + 1))
        tn_dest = [TonesDest(rows, rows * pkg.tones_max_windows(CHAIN_WINDOW, n)) for _ in tn]
        mix_dest = MixDest(n)
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, nbytes, n, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        vb.process_device(wo.data_ptr(), stride, n, filt.data_ptr(), out_stride, hip_stream=s)
        tx.process_device(filt.data_ptr(), out_stride, ax.data_ptr(), n, n, tx_dest.records.data_ptr(), tx_dest.row_first.data_ptr(), tx_dest.count.data_ptr(),
                          hip_stream=s)
        for t, plane, row_stride, dest in zip(tn, (filt, wo), (out_stride, stride), tn_dest):
            t.process_device(plane.data_ptr(), row_stride, ax.data_ptr(), n, n, dest.records.data_ptr(), dest.row_first.data_ptr(), dest.count.data_ptr(),
                             d_powers=dest.powers.data_ptr(), hip_stream=s)
        mixer.process_device(filt.data_ptr(), out_stride, ax.data_ptr(), n, n, mix_dest.left.data_ptr(), mix_dest.right.data_ptr(), mix_dest.out.data_ptr(),
                             hip_stream=s)
        got_tx = tx.download(s)  # (the first wait of the call)
        got_tn = [t.download(s) for t in tn]
        outs.append((n, wo.cpu().numpy(), ax.cpu().numpy(), filt.cpu().numpy(), got_tx, tx_dest, got_tn, tn_dest, mix_dest))
        done += n
    states = vb.state(), tx.state(), tn[0].state(), tn[1].state()
    for h in [d, vb, tx, mixer] + tn:
        h.close()
    flags = np.concatenate([o[2] for o in outs], axis=1)
    print("flags per row:", [bytes(f).decode() for f in flags])
    vb_state = tx_state = None
    tn_state = [None, None]
    for i, (n, wo, ax, filt, got_tx, tx_dest, got_tn, tn_dest, mix_dest) in enumerate(outs):
        blank = np.full(filt.shape, SENT)
        want, vb_state = pkg.vband_plan_host(ones, wo, CHAIN_BAND, vb_state, nbatches=n, out=blank)
        assert (want[:, n * WAVE_BATCH:] == SENT).all()
        assert filt.tobytes() == want.tobytes(), f"call {i}: the filtered plane, or the sentinel behind it"
        want_rec, want_first, _, tx_state = pkg.tx_plan_host(ones, ax, tx_state, want, nbatches=n)
        tx_check(f"call {i}: the splitter", got_tx, tx_dest, rows, want_rec, want_first)
        assert (want_rec["energy"][want_rec["nblocks"] > 0] > 0).all()
        for j, (plane, what) in enumerate(((want, "filtered"), (wo, "unfiltered"))):
            rec, pw, first, _, tn_state[j] = pkg.tones_plan_host(ones, ax, plane, tn_state[j], CHAIN_WINDOW, nbatches=n)
            tones_check(f"call {i}: the tone finder on the {what} plane", got_tn[j], tn_dest[j], rows, rec, pw, first)
        left, right, out = libs.oracle_mixer(CHAIN_MIX, want, ax, n)
        model = numpy_mixer(CHAIN_MIX, want, ax, n)
        assert left.tobytes() == model[0].tobytes() and right.tobytes() == model[1].tobytes() and out.tobytes() == model[2].tobytes()
        torch.cuda.synchronize()
        mix_dest.check(f"call {i}: the mixer", left.tobytes(), right.tobytes(), out.tobytes())
        if (ax != ord(" ")).any():
            assert np.abs(left).max() > 0
    assert states[0].tobytes() == vb_state.tobytes() and states[1].tobytes() == tx_state.tobytes()
    assert states[2].tobytes() == tn_state[0].tobytes() and states[3].tobytes() == tn_state[1].tobytes()
    ratios = chain_tone_ratios(calls, flags, *[[(o[6][j][0], o[6][j][1], o[6][j][2]) for o in outs] for j in range(2)])
    print("row 0, 100.0 Hz, filtered over unfiltered (first sample, dB, settled):", [(a, round(b, 2), c) for a, b, c in ratios])
    settled = [db for _, db, ok in ratios if ok]
    assert len(ratios) >= 4 and len(settled) >= 4, "the capture should open the row with the tone for half of its batches"
    assert max(db for _, db, _ in ratios) <= CHAIN_WORST_DB + 10.0
    assert max(settled) <= CHAIN_SETTLED_DB[1] + 10.0
    for j, what in enumerate(("filtered", "unfiltered")):
        v = pkg.tones_vote_host(np.concatenate([o[6][j][0][o[6][j][2][0]:o[6][j][2][1]] for o in outs]))
        print(f"vote on the {what} plane, row 0: found {v.found} tone {v.tone} ({v.freq_hz} Hz), {v.votes} of {v.windows} windows")


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
