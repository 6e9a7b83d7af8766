"""The transmission splitter on the GPU (mi_txsplit_*, csrc/txsplit.hip) against the plain-Python restatement of split_on_transmission
in tx_model.py and against its host twin mi_tx_plan_host.

Every comparison is bit for bit: records travel and are compared as bytes (peak and energy included -- the order of the sums is
part of the definition), the state blob as bytes.  Every destination buffer is filled with a sentinel before a call and is longer
than the capacity the splitter is told; what it must not write must still hold the sentinel afterwards."""
import numpy as np
import pytest

from common import AGC_EXTRA, bytes_for_batches, oracle_run
from gate_model import WAVE_BATCH
from tx_model import (BURST_SHAPES, DEFAULT_CFG, FAMILIES, NONE, RECORD, SMALL_CFG, draw_audio, draw_bursts, draw_family, fresh_state, letters, run_in_calls,
                      tx_model)

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 3  # records / entries allocated behind the capacity
E2E_GATE = (5, 8)  # carriers on for 5 batches and off for 5: gate_samples = sample_rate * 5 / 8


class Dest:
    """destination buffers for `cap` records, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, cap):
        import torch
        self.cap = cap
        self.records = torch.full(((cap + GUARD) * RECORD.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.row_first = torch.full((rows + 1 + GUARD,), SENT32, dtype=torch.int32, device="cuda")
        self.count = torch.full((2 + GUARD,), SENT32, dtype=torch.int32, device="cuda")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def tx_call(tx, d_wave, row_stride, d_axc, axc_stride, nb, dest, stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    tx.process_device(None if d_wave is None else d_wave.data_ptr(), row_stride, d_axc.data_ptr(), axc_stride, nb, dest.records.data_ptr(),
                      dest.row_first.data_ptr(), dest.count.data_ptr(), hip_stream=s)
    return tx.download(s)


def check(what, got, dest, rows, want_rec, want_first):
    rec, row_first, count = got
    total, k = len(want_rec), min(len(want_rec), dest.cap)
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}, the model has {total}"
    assert np.array_equal(row_first, want_first), f"{what}: row_first_record"
    assert rec.tobytes() == want_rec[:k].tobytes(), f"{what}: records\n{rec}\nwant\n{want_rec[:k]}"
    d_rec = dest.records.cpu().numpy()
    assert d_rec[:k * RECORD.itemsize].tobytes() == want_rec[:k].tobytes(), f"{what}: records on the device"
    assert (d_rec[k * RECORD.itemsize:] == SENT_BYTE).all(), f"{what}: something was written behind record {k}"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT32).all() and (dest.count.cpu().numpy()[2:] == SENT32).all()


def synthetic(pkg, rows, nb, family, cfg, seed, cap=0, pad=3, warm=True, audio=True, enabled=None):
    """one splitter, one call over buffers laid out for nb + pad batches, from a mid-run state; device against model and host twin"""
    lay = nb + pad
    rng = np.random.default_rng([seed, rows, nb, FAMILIES.index(family), cfg[0]])
    axc = draw_family(family, rng, rows, lay)
    wave = draw_audio(rng, rows, lay * WAVE_BATCH) if audio else None
    state = tx_model(draw_bursts(rng, rows, 9), cfg=cfg)[2] if warm else fresh_state(rows)
    en = np.ones(rows, np.uint8) if enabled is None else enabled
    want_rec, want_first, want_state, _, _ = tx_model(axc[:, :nb], state, en, wave, cfg)
    tx = pkg.TxSplit(en, max_batches=max(nb, 2), cfg=cfg, max_records=cap)
    tx.set_state(state)
    dest = Dest(rows, cap or rows * (max(nb, 2) + 1))
    got = tx_call(tx, None if wave is None else to_dev(wave), lay * WAVE_BATCH, to_dev(axc), lay, nb, dest)
    what = f"{rows} x {nb} (laid out for {lay}), {family}, cfg {cfg}"
    print(f"{what}: {len(want_rec)} records, capacity {dest.cap}")
    check(what, got, dest, rows, want_rec, want_first)
    after = tx.state()
    assert after.tobytes() == want_state.tobytes(), f"{what}: state blob against the model"
    twin = pkg.tx_plan_host(en, axc, state, wave, cfg, nbatches=nb)
    assert twin[0].tobytes() == want_rec.tobytes() and after.tobytes() == twin[3].tobytes(), f"{what}: host twin"
    tx.close()
    return want_rec


@gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows,nbatches", BURST_SHAPES)
def test_device_equals_model(pkg, rows, nbatches, family):
    """Rows shorter than, equal to and longer than a wave's 64-flag trip (1, 3, 64, 65, 130 batches); row counts on both sides of the
    four-rows-per-workgroup packing and of the scan's 256-row tile (1, 3, 65, 1025); padded strides; small thresholds and the
    reference's own."""
    for cfg in (SMALL_CFG, DEFAULT_CFG):
        synthetic(pkg, rows, nbatches, family, cfg, seed=1)


@gpu
def test_long_rows_reach_every_branch(pkg):
    """3 x 515 batches (nine trips of the walk, the last one short) from a fresh state: closes by idle, appended transmissions and
    splits at max all occur on the device"""
    rec = synthetic(pkg, 3, 515, "bursts", SMALL_CFG, seed=2, warm=False)
    assert (rec["close_batch"] != NONE).sum() > 10
    rec = synthetic(pkg, 3, 515, "p100", SMALL_CFG, seed=2, warm=False)
    assert len(rec) == 3 * 47 and (rec["nblocks"][:46] == 11).all()
    synthetic(pkg, 3, 515, "p05", DEFAULT_CFG, seed=2)
    synthetic(pkg, 3, 515, "p50", DEFAULT_CFG, seed=2)


@gpu
def test_without_audio(pkg):
    rec = synthetic(pkg, 5, 65, "bursts", SMALL_CFG, seed=3, audio=False)
    assert len(rec) and not rec["peak"].any() and not rec["energy"].any()


@gpu
@pytest.mark.parametrize("rows,nbatches,cap", [(3, 65, 7), (65, 3, 1), (1025, 3, 300)])
def test_capacity_short_of_the_total(pkg, rows, nbatches, cap):
    rec = synthetic(pkg, rows, nbatches, "bursts", SMALL_CFG, seed=4, cap=cap)
    assert len(rec) > cap


@gpu
def test_disabled_rows_and_set_rows_between_calls(pkg):
    """rows 1 and 3 sit the second of three calls out: no record, every byte of their state stays, and the third call goes on from it"""
    import torch
    rows, n = 5, 20
    rng = np.random.default_rng(5)
    axc = draw_bursts(rng, rows, 3 * n)
    wave = draw_audio(rng, rows, 3 * n * WAVE_BATCH)
    masks = (np.ones(rows, np.uint8), np.array([1, 0, 1, 0, 1], np.uint8), np.ones(rows, np.uint8))
    tx = pkg.TxSplit(masks[0], max_batches=n, cfg=SMALL_CFG)
    state = fresh_state(rows)
    for i, en in enumerate(masks):
        if i:
            tx.set_rows(en)
        a = np.ascontiguousarray(axc[:, i * n:(i + 1) * n])
        w = np.ascontiguousarray(wave[:, i * n * WAVE_BATCH:(i + 1) * n * WAVE_BATCH])
        want_rec, want_first, after, _, _ = tx_model(a, state, en, w, SMALL_CFG)
        dest = Dest(rows, rows * (n + 1))
        check(f"call {i}", tx_call(tx, to_dev(w), n * WAVE_BATCH, to_dev(a), n, n, dest), dest, rows, want_rec, want_first)
        got = tx.state()
        assert got.tobytes() == after.tobytes()
        if i == 1:
            assert set(want_rec["row"]) <= {0, 2, 4}
            before = state.view(np.uint8).reshape(rows, 32)
            assert np.array_equal(got.reshape(rows, 32)[[1, 3]], before[[1, 3]]) and before[1].any()
        state = after
    assert [int(c) for c in state["clock"]] == [3 * n, 2 * n, 3 * n, 2 * n, 3 * n]
    tx.close()
    with pytest.raises(pkg.MiError) as e:
        bad = np.zeros(32, np.uint8)
        bad[29] = 7
        t = pkg.TxSplit([1], max_batches=2)
        t.set_state(bad)
    assert e.value.code == pkg.MI_ERR_INVALID
    torch.cuda.synchronize()


@gpu
def test_eight_calls_on_a_side_stream_with_the_state_through_the_host_twin(pkg):
    """Eight consecutive calls of unequal length on one object, enqueued on a side stream with no host synchronisation before
    download, equal one run of the model.  The fourth call is made by the host twin instead, from the device's state blob, and its
    state goes back to the device: nothing changes."""
    import torch
    rows, cuts = 5, (1, 66, 3, 17, 64, 9, 30, 10)
    total = sum(cuts)
    rng = np.random.default_rng(6)
    axc = draw_bursts(rng, rows, total)
    wave = draw_audio(rng, rows, total * WAVE_BATCH)
    calls, want_state, file_of, closes = run_in_calls(axc, cuts, DEFAULT_CFG, wave)
    uncut = tx_model(axc, cfg=DEFAULT_CFG)
    assert np.array_equal(uncut[3], file_of) and uncut[2].tobytes() == want_state.tobytes(), "the model itself does not mind the cuts"
    assert any((rec["flags"] & 1).any() for _, rec, _ in calls) and any((rec["nblocks"] == 0).any() for _, rec, _ in calls) and len(closes) > rows
    side = torch.cuda.Stream()
    tx = pkg.TxSplit(np.ones(rows), max_batches=max(cuts), cfg=DEFAULT_CFG)
    torch.cuda.synchronize()
    for i, (n, (done, want_rec, want_first)) in enumerate(zip(cuts, calls)):
        a = np.ascontiguousarray(axc[:, done:done + n])
        w = np.ascontiguousarray(wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH])
        if i == 3:
            rec, first, count, after = pkg.tx_plan_host(np.ones(rows), a, tx.state(), w, DEFAULT_CFG)
            assert rec.tobytes() == want_rec.tobytes() and np.array_equal(first, want_first)
            tx.set_state(after)
            continue
        dest = Dest(rows, rows * (max(cuts) + 1))
        with torch.cuda.stream(side):
            d_w, d_a = to_dev(w), to_dev(a)
        got = tx_call(tx, d_w, n * WAVE_BATCH, d_a, n, n, dest, stream=side.cuda_stream)
        check(f"call {i} at batch {done}", got, dest, rows, want_rec, want_first)
    assert tx.state().tobytes() == want_state.tobytes()
    tx.close()


@gpu
def test_gate_and_splitter_compose(pkg):
    """An MI_GATE_OPEN_TRAIL gate and the splitter over the same buffers on one stream: the gate's packed audio and raw I/Q blocks,
    sliced by the splitter's records, are the model's per-file audio and I/Q."""
    import torch
    rows, nb = 6, 70
    rng = np.random.default_rng(7)
    axc = draw_bursts(rng, rows, nb)
    wave = draw_audio(rng, rows, nb * WAVE_BATCH)
    iq = rng.uniform(-1, 1, (rows, nb * 2 * WAVE_BATCH)).astype(np.float32)
    want_rec, want_first, _, file_of, _ = tx_model(axc, wave=wave, cfg=SMALL_CFG)
    s = torch.cuda.current_stream().cuda_stream
    gate = pkg.OutputGate(np.full(rows, pkg.GATE_OPEN_TRAIL, np.uint8), np.ones(rows), max_batches=nb)
    tx = pkg.TxSplit(np.ones(rows), max_batches=nb, cfg=SMALL_CFG)
    d_wave, d_iq, d_axc = to_dev(wave), to_dev(iq), to_dev(axc)
    blocks = torch.zeros((rows * nb, WAVE_BATCH), dtype=torch.float32, device="cuda")
    iq_blocks = torch.zeros((rows * nb, 2 * WAVE_BATCH), dtype=torch.float32, device="cuda")
    index = torch.zeros((rows * nb, 2), dtype=torch.int32, device="cuda")
    g_first, g_count = torch.zeros(rows + 1, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    dest = Dest(rows, rows * (nb + 1))
    gate.process_device(d_wave.data_ptr(), nb * WAVE_BATCH, d_axc.data_ptr(), nb, nb, blocks.data_ptr(), index.data_ptr(), g_first.data_ptr(),
                        g_count.data_ptr(), d_iq_out=d_iq.data_ptr(), iq_row_stride=nb * 2 * WAVE_BATCH, d_iq_blocks=iq_blocks.data_ptr(), hip_stream=s)
    tx.process_device(d_wave.data_ptr(), nb * WAVE_BATCH, d_axc.data_ptr(), nb, nb, dest.records.data_ptr(), dest.row_first.data_ptr(),
                      dest.count.data_ptr(), hip_stream=s)
    got = tx.download(s)
    check("beside the gate", got, dest, rows, want_rec, want_first)
    h_blocks, h_iq, _, row_first, count = gate.download(s, want_iq=True)
    assert int(count[0]) == int((file_of > 0).sum()) == int(want_rec["nblocks"].sum())
    files = 0
    for rec in got[0]:
        r, lo, n = int(rec["row"]), int(row_first[rec["row"]]) + int(rec["first_block"]), int(rec["nblocks"])
        mine = np.flatnonzero(file_of[r] == rec["seq"])
        assert len(mine) == n
        assert np.array_equal(h_blocks[lo:lo + n], wave[r].reshape(nb, WAVE_BATCH)[mine]), f"row {r} file {rec['seq']}: audio"
        assert np.array_equal(h_iq[lo:lo + n].reshape(n, -1), iq[r].reshape(nb, 2 * WAVE_BATCH)[mine]), f"row {r} file {rec['seq']}: raw I/Q"
        files += 1
    assert files > rows
    gate.close()
    tx.close()


@gpu
def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    tx = pkg.TxSplit([1, 1, 0], max_batches=nb)
    dest = Dest(rows, rows * (nb + 1))
    wave = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    axc = torch.full((rows, nb), 32, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=wave.data_ptr(), row_stride=nb * WAVE_BATCH, d_records=dest.records.data_ptr(), d_axc=axc.data_ptr()):
        tx.process_device(d_wave, row_stride, d_axc, nb, nbatches, d_records, dest.row_first.data_ptr(), dest.count.data_ptr(), hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_axc=None), dict(d_records=None), dict(d_wave=wave.data_ptr() + 4),
                dict(d_records=dest.records.data_ptr() + 4), dict(row_stride=nb * WAVE_BATCH + 2), dict(row_stride=WAVE_BATCH)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        tx.download(s)  # nothing was enqueued yet
    call(d_wave=None)
    call()
    rec, first, count = tx.download(s)
    assert tuple(count) == (0, 0) and not first.any()
    with pytest.raises(pkg.MiError) as e:
        pkg.TxSplit(np.ones(5), max_batches=0)
    assert e.value.code == pkg.MI_ERR_INVALID
    tx.close()


def e2e_setup(pkg, nb):
    centre, chans = pkg.config2_channels()
    dev = pkg.device_cfg(centerfreq=centre)
    carriers = [(c.freq - centre, 0, 2048, k % 2) for k, c in enumerate(chans)]
    nbytes = (bytes_for_batches(dev, nb) + 255) // 256 * 256
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate * E2E_GATE[0] // E2E_GATE[1], carriers=carriers)
    return dev, chans, cfg, nbytes


def e2e_condition(axc):
    """at least two files open and at least one closes, under the reference's own thresholds"""
    rec, _, _, file_of, closes = tx_model(axc, cfg=DEFAULT_CFG)
    print("flags and files per row:", [(bytes(f).decode(), letters(x)) for f, x in zip(axc, file_of)])
    return int(rec["seq"].max(initial=0)) >= 2 and len(closes) >= 1


def test_end_to_end_signal_meets_its_condition_on_the_oracle(pkg):
    """(no GPU) the gated iqgen signal of the end-to-end case below, through the CPU oracle: its flags alone open two files and close one"""
    nb = 24
    dev, chans, cfg, nbytes = e2e_setup(pkg, nb)
    n, _, axc, _ = oracle_run(dev, chans, pkg.iqgen_host(cfg, 0, 0, nbytes // 2), nb)
    assert n == nb and e2e_condition(axc)


@gpu
def test_end_to_end_behind_the_demodulator(pkg):
    """A Demod of the 8-AM-channel plan at fft 512 on the gated iqgen signal, 24 batches in three calls of 8, each followed on the
    same stream by the splitter under the reference's own thresholds: the records equal the model applied to the flags and the audio
    the demodulator itself returned, call by call."""
    import torch
    calls = (8, 8, 8)
    dev, chans, cfg, nbytes = e2e_setup(pkg, sum(calls))
    rows = len(chans)
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, 1, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    tx = pkg.TxSplit(np.ones(rows), max_batches=max(calls))
    outs, done = [], 0
    for n in calls:  # (no host synchronisation between the demodulator and the splitter)
        wo = torch.zeros((rows, n * WAVE_BATCH), dtype=torch.float32, device="cuda")
        ax = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
        dest = Dest(rows, rows * (n + 1))
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, nbytes, n, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        got = tx_call(tx, wo, n * WAVE_BATCH, ax, n, n, dest, stream=s)
        outs.append((got, dest, wo.cpu().numpy(), ax.cpu().numpy()))
        done += n
    d.close()
    axc = np.concatenate([o[3] for o in outs], axis=1)
    assert e2e_condition(axc), "the demodulator's own flags open two files and close one"
    state = None
    for i, (got, dest, wo, ax) in enumerate(outs):
        want_rec, want_first, state, _, _ = tx_model(ax, state, None, wo, DEFAULT_CFG)
        check(f"end to end, call {i}", got, dest, rows, want_rec, want_first)
        assert (got[0]["energy"][got[0]["nblocks"] > 0] > 0).all() and (got[0]["peak"] <= 1.0).all()
    assert tx.state().tobytes() == state.tobytes()
    tx.close()
