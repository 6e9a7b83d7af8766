"""The output gate on the GPU (mi_outgate_*, csrc/outgate.hip) against the numpy restatement of src/output.cpp in gate_model.py.

Everything the gate moves is a copy, so every comparison is bit for bit (float32 buffers travel and are compared as int32) and there
are no tolerances.  Every destination buffer is filled with a sentinel before a call and is longer than the capacity the gate is
told: what the gate must not write -- slots past the count, raw-I/Q slots of rows without raw I/Q, anything behind the capacity --
must still hold the sentinel afterwards."""
import numpy as np
import pytest

from common import AGC_EXTRA, bytes_for_batches
from gate_model import NO_SIGNAL, OPEN_PROBABILITIES, SHAPES, WAVE_BATCH, bits, draw_flags, draw_rules, gate_model

pytestmark = pytest.mark.gpu

SENT = int(np.uint32(0xDEADBEEF).view(np.int32))  # what every destination buffer holds before a call
GUARD = 2  # blocks / entries allocated behind the capacity


def to_dev(a):
    """host array -> device tensor with the same bytes (float32 as int32: no value of it is ever interpreted)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits(a)).copy()).cuda()


def sentinel(shape):
    import torch
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


class Dest:
    """destination buffers of `cap` blocks, GUARD more allocated behind them, all holding the sentinel"""

    def __init__(self, rows, cap, with_iq):
        self.cap = cap
        self.blocks = sentinel((cap + GUARD, WAVE_BATCH))
        self.iq = sentinel((cap + GUARD, WAVE_BATCH, 2)) if with_iq else None
        self.index = sentinel((cap + GUARD, 2))
        self.row_first = sentinel((rows + 1 + GUARD,))
        self.count = sentinel((2 + GUARD,))


def random_planes(rng, rows, row_stride, iq_row_stride):
    wave = rng.integers(0, 2**32, (rows, row_stride), dtype=np.uint32).view(np.int32)
    iq = rng.integers(0, 2**32, (rows, iq_row_stride), dtype=np.uint32).view(np.int32)
    wave[0, :4] = np.array([0x7FC00000, 0x7F800001, 0xFFC00001, 0x80000000], np.uint32).view(np.int32)  # NaN patterns, -0.0
    return wave, iq


def gate_call(gate, d_wave, row_stride, d_iq, iq_row_stride, d_axc, axc_stride, nb, dest, stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    gate.process_device(d_wave.data_ptr(), row_stride, d_axc.data_ptr(), axc_stride, nb, dest.blocks.data_ptr(), dest.index.data_ptr(),
                        dest.row_first.data_ptr(), dest.count.data_ptr(), d_iq_out=None if d_iq is None else d_iq.data_ptr(),
                        iq_row_stride=iq_row_stride, d_iq_blocks=None if dest.iq is None else dest.iq.data_ptr(), hip_stream=s)
    return gate.download(s, want_iq=dest.iq is not None and d_iq is not None)


def check(what, got, dest, rows, rule, has_iq, wave, iq, axc, nb, carried_before):
    """got = download() of a call over host planes wave [rows][row_stride], iq [rows][iq_row_stride] (int32 views) and flags
    axc [rows][axc_stride], of which the first nb batches take part.  Returns the model's carried flags after the call."""
    blocks, iq_blocks, index, row_first, count = got
    want_index, want_first, after = gate_model(rule, axc[:, :nb], carried_before)
    total = len(want_index)
    k = min(total, dest.cap)
    print(f"{what}: {total} of {rows * nb} blocks travel, capacity {dest.cap}")
    assert (int(count[0]), int(count[1])) == (total, k), f"{what}: counts {count}"
    assert np.array_equal(row_first, want_first), f"{what}: row_first"
    assert np.array_equal(index, want_index[:k]), f"{what}: index"
    r, b = want_index[:k, 0].astype(np.int64), want_index[:k, 1].astype(np.int64)
    want_blocks = wave[:, :nb * WAVE_BATCH].reshape(rows, nb, WAVE_BATCH)[r, b]
    assert blocks.shape == (k, WAVE_BATCH)
    assert np.array_equal(bits(blocks), want_blocks), f"{what}: audio blocks"
    # the device buffers themselves: what download() copied is what lies there, and nothing else was written
    d_blocks, d_index = dest.blocks.cpu().numpy(), dest.index.cpu().numpy()
    assert np.array_equal(d_blocks[:k], want_blocks) and (d_blocks[k:] == SENT).all(), f"{what}: audio behind the last block"
    assert np.array_equal(d_index[:k].view(np.uint32), want_index[:k]) and (d_index[k:] == SENT).all(), f"{what}: index behind the last entry"
    assert (dest.row_first.cpu().numpy()[rows + 1:] == SENT).all() and (dest.count.cpu().numpy()[2:] == SENT).all()
    if dest.iq is not None and iq is not None:
        want_iq = iq[:, :nb * 2 * WAVE_BATCH].reshape(rows, nb, WAVE_BATCH, 2)[r, b]
        with_iq = np.asarray(has_iq, bool)[r]
        d_iq = dest.iq.cpu().numpy()
        assert np.array_equal(bits(iq_blocks)[with_iq], want_iq[with_iq]), f"{what}: raw I/Q blocks"
        assert np.array_equal(d_iq[:k][with_iq], want_iq[with_iq]), f"{what}: raw I/Q blocks on the device"
        assert (d_iq[:k][~with_iq] == SENT).all(), f"{what}: raw I/Q slot of a row without raw I/Q was written"
        assert (d_iq[k:] == SENT).all(), f"{what}: raw I/Q behind the last block"
    return after


def synthetic(pkg, rows, nb, p_open, rule_kind, seed, cap=0, layout_batches=None):
    """one gate, one call over random planes; layout_batches: the buffers are laid out for that many batches (padded strides)"""
    lay = layout_batches or nb
    rng = np.random.default_rng([seed, rows, nb, int(p_open * 100)])
    row_stride, iq_row_stride, axc_stride = lay * WAVE_BATCH, lay * 2 * WAVE_BATCH, lay
    wave, iq = random_planes(rng, rows, row_stride, iq_row_stride)
    axc = draw_flags(rng, rows, lay, p_open)
    rule = draw_rules(rng, rows, rule_kind)
    has_iq = (np.arange(rows) % 3 == 1) | (rows == 1)
    carried = rng.integers(0, 2, rows).astype(np.uint8)
    gate = pkg.OutputGate(rule, has_iq, max_batches=max(nb, 2), max_blocks=cap)
    gate.set_state(carried)
    dest = Dest(rows, cap or rows * max(nb, 2), True)
    got = gate_call(gate, to_dev(wave), row_stride, to_dev(iq), iq_row_stride, to_dev(axc), axc_stride, nb, dest)
    what = f"{rows} x {nb} (laid out for {lay}), p {p_open}, rule {rule_kind}"
    after = check(what, got, dest, rows, rule, has_iq, wave, iq, axc, nb, carried)
    assert np.array_equal(gate.state(), after), f"{what}: carried flags"
    gate.close()
    return got


@pytest.mark.parametrize("p_open", OPEN_PROBABILITIES)
@pytest.mark.parametrize("rows,nbatches", SHAPES)
def test_synthetic_planes(pkg, rows, nbatches, p_open):
    """Rows shorter than, equal to and one longer than a wave's 64-batch chunk (1, 64, 65, 130 batches); row counts on both sides of
    the scan's 256-row tile and of the four-rows-per-workgroup packing (1, 3, 65, 1025); every rule on some row."""
    assert rows * nbatches <= 3100
    synthetic(pkg, rows, nbatches, p_open, "mixed", seed=1)


@pytest.mark.parametrize("rule_kind", [0, 1, 2, 3])
def test_one_rule_on_every_row(pkg, rule_kind):
    synthetic(pkg, 65, 3, 0.5, rule_kind, seed=2)
    synthetic(pkg, 3, 65, 0.05, rule_kind, seed=2)


def test_all_closed_moves_nothing_and_all_open_fills_the_capacity(pkg):
    blocks, _, index, row_first, count = synthetic(pkg, 65, 3, 0.0, 1, seed=3)  # (check() asserts every destination still holds the sentinel)
    assert tuple(count) == (0, 0) and len(blocks) == 0 and len(index) == 0 and not row_first.any()
    for rows, nb in ((65, 3), (3, 65)):
        blocks, _, index, row_first, count = synthetic(pkg, rows, nb, 1.0, 1, seed=3, cap=rows * nb)
        assert tuple(count) == (rows * nb, rows * nb) and len(blocks) == rows * nb
        assert np.array_equal(row_first, np.arange(rows + 1) * nb)


@pytest.mark.parametrize("rows,nbatches,cap", [(3, 65, 40), (65, 3, 1), (1025, 3, 700)])
def test_capacity_smaller_than_the_travelling_count(pkg, rows, nbatches, cap):
    """count[0] is the full number, count[1] the capacity; the first count[1] blocks and entries are right and the sentinel behind the
    capacity is intact in every destination buffer (check())."""
    _, _, _, _, count = synthetic(pkg, rows, nbatches, 0.5, "mixed", seed=4, cap=cap)
    assert count[0] > cap and count[1] == cap


@pytest.mark.parametrize("p_open", [0.05, 0.5])
def test_padded_strides(pkg, p_open):
    """a 3-batch call out of buffers laid out for 8: row_stride, iq_row_stride and axc_stride larger than the call"""
    synthetic(pkg, 3, 3, p_open, "mixed", seed=5, layout_batches=8)
    synthetic(pkg, 65, 3, p_open, 2, seed=5, layout_batches=8)


def test_argument_errors(pkg):
    import torch
    rows, nb = 3, 2
    gate = pkg.OutputGate([1, 2, 3], [0, 1, 0], max_batches=nb)
    dest = Dest(rows, rows * nb, True)
    wave, iq, axc = sentinel((rows, nb * WAVE_BATCH)), sentinel((rows, nb * 2 * WAVE_BATCH)), torch.full((rows, nb), 32, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=wave.data_ptr(), row_stride=nb * WAVE_BATCH, d_iq=iq.data_ptr(), d_iq_blocks=dest.iq.data_ptr(), d_blocks=dest.blocks.data_ptr()):
        gate.process_device(d_wave, row_stride, axc.data_ptr(), nb, nbatches, d_blocks, dest.index.data_ptr(), dest.row_first.data_ptr(),
                            dest.count.data_ptr(), d_iq_out=d_iq, iq_row_stride=nb * 2 * WAVE_BATCH, d_iq_blocks=d_iq_blocks, hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_wave=None), dict(d_blocks=None), dict(d_wave=wave.data_ptr() + 4),
                dict(d_blocks=dest.blocks.data_ptr() + 8), dict(row_stride=nb * WAVE_BATCH + 2), dict(d_iq_blocks=None)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    call(d_iq=None, d_iq_blocks=None)  # no raw I/Q handed in: none is packed, and no buffer for it is needed
    call()
    torch.cuda.synchronize()
    with pytest.raises(pkg.MiError) as e:
        pkg.OutputGate([1, 4, 0])
    assert e.value.code == pkg.MI_ERR_INVALID
    with pytest.raises(pkg.MiError) as e:
        gate.set_rules([1, 2, 9])
    assert e.value.code == pkg.MI_ERR_INVALID
    gate.close()


def test_call_boundaries_and_checkpoint(pkg):
    """One gate over three consecutive calls of unequal length; its state after the second call resumes a second gate, which is fed the
    third call: both equal the model's uncut run, per row and in time order.  A change of rules between calls keeps the flags."""
    import torch
    rows, cuts = 5, (1, 66, 3)
    total = sum(cuts)
    rng = np.random.default_rng(6)
    wave, iq = random_planes(rng, rows, total * WAVE_BATCH, total * 2 * WAVE_BATCH)
    axc = draw_flags(rng, rows, total, 0.35)
    axc[1, :2] = [ord("*"), NO_SIGNAL]  # a trailing batch right behind the first boundary ...
    axc[2, 66:68] = [ord(">"), NO_SIGNAL]  # ... and one behind the second
    rule = np.array([2, 2, 2, 1, 3], np.uint8)
    has_iq = np.array([0, 1, 1, 0, 0], np.uint8)
    uncut, uncut_first, uncut_after = gate_model(rule, axc)
    assert (1, 1) in {tuple(x) for x in uncut} and (2, 67) in {tuple(x) for x in uncut}
    side = torch.cuda.Stream()

    def feed(gate, first, n, carried):
        sl = lambda a, per: np.ascontiguousarray(a[:, first * per:(first + n) * per])
        w, z, f = sl(wave, WAVE_BATCH), sl(iq, 2 * WAVE_BATCH), sl(axc, 1)
        dest = Dest(rows, rows * n, True)
        got = gate_call(gate, to_dev(w), n * WAVE_BATCH, to_dev(z), n * 2 * WAVE_BATCH, to_dev(f), n, n, dest, stream=side.cuda_stream)
        after = check(f"calls {cuts}, batches {first} .. {first + n - 1}", got, dest, rows, rule, has_iq, w, z, f, n, carried)
        assert np.array_equal(gate.state(), after)
        return got, after

    gate = pkg.OutputGate(rule, has_iq, max_batches=max(cuts))
    torch.cuda.synchronize()
    pieces, carried, done = [], np.zeros(rows, np.uint8), 0
    for i, n in enumerate(cuts):
        if i == 2:
            saved = gate.state()
            assert np.array_equal(saved, carried)
            gate.set_rules(rule)  # (the same rules again: the flags must survive the call)
            resumed = pkg.OutputGate(rule, has_iq, max_batches=n)
            resumed.set_state(saved)
            twin, _ = feed(resumed, done, n, carried)
            resumed.close()
        got, carried = feed(gate, done, n, carried)
        pieces.append((done, got))
        done += n
    gate.close()
    assert np.array_equal(carried, uncut_after)
    for a, b in zip(twin, pieces[2][1]):
        assert np.array_equal(bits(a), bits(b)), "the resumed gate's third call differs"
    for r in range(rows):
        mine = [(first + int(b), blk) for first, (blocks, _, index, _, _) in pieces for (rr, b), blk in zip(index, blocks) if rr == r]
        want = uncut[uncut_first[r]:uncut_first[r + 1], 1]
        assert [b for b, _ in mine] == [int(b) for b in want], f"row {r}: batches"
        for b, blk in mine:
            assert np.array_equal(bits(blk), wave[r, b * WAVE_BATCH:(b + 1) * WAVE_BATCH]), f"row {r} batch {b}"


def test_end_to_end_behind_the_demodulator(pkg):
    """2 streams x the 8-AM-channel plan (channel 1 with a rawfile output), carriers gated with a period of 1.5 batches, alternating
    phase: two device calls of 4 and 5 batches through mi_demod_process_device, each followed on the same stream by the gate with the
    rules {1, 2, 3, 0} cycled over the rows, against the model applied to the demodulator's own downloaded audio, raw I/Q and flags."""
    import torch
    centre, chans = pkg.config2_channels()
    chans[1].has_iq_outputs = 1
    nch, ns, calls = len(chans), 2, (4, 5)
    rows = ns * nch
    dev = pkg.device_cfg(centerfreq=centre)
    carriers = [(c.freq - centre, 0, 2048, k % 2) for k, c in enumerate(chans)]
    nbytes = (bytes_for_batches(dev, sum(calls)) + 255) // 256 * 256
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate * 3 // 16, carriers=carriers)
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((ns, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, ns, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    rule = np.array([1, 2, 3, 0] * (rows // 4), np.uint8)
    has_iq = np.array([c.has_iq_outputs for c in chans] * ns, np.uint8)
    assert has_iq.sum() == ns and (rule[has_iq == 1] == 2).all(), "the rawfile rows are under the file rule"
    d = pkg.Demod(dev, chans, nstreams=ns, max_batches=max(calls))
    gate = pkg.OutputGate(rule, has_iq, max_batches=max(calls))
    outs, done = [], 0
    for n in calls:  # (no host synchronisation between the demodulator and the gate)
        wo = sentinel((rows, n * WAVE_BATCH))
        zo = sentinel((rows, n * 2 * WAVE_BATCH))
        ax = torch.zeros((rows, n), dtype=torch.uint8, device="cuda")
        dest = Dest(rows, rows * n, True)
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, nbytes, n, wo.data_ptr(), ax.data_ptr(), d_iq_out_ptr=zo.data_ptr(), hip_stream=s)
        got = gate_call(gate, wo, n * WAVE_BATCH, zo, n * 2 * WAVE_BATCH, ax, n, n, dest, stream=s)
        outs.append((n, got, dest, wo.cpu().numpy(), zo.cpu().numpy(), ax.cpu().numpy()))
        done += n
    d.close()
    flags = np.concatenate([o[5] for o in outs], axis=1)
    print("flags per row:", [bytes(f).decode() for f in flags])
    is_open = flags != NO_SIGNAL
    first_n = calls[0]
    closes_inside = (is_open[:, :first_n - 1] & ~is_open[:, 1:first_n]).any(axis=1)
    across = is_open[:, first_n - 1] & is_open[:, first_n]
    assert closes_inside.any(), "no row closes inside the first call"
    assert across.any(), "no row is open across the call boundary"
    assert (closes_inside & (rule == 2)).any() or (closes_inside & (rule == 1)).any()
    carried = np.zeros(rows, np.uint8)
    for i, (n, got, dest, wo, zo, ax) in enumerate(outs):
        carried = check(f"end to end, call {i}", got, dest, rows, rule, has_iq, wo, zo, ax, n, carried)
        assert 0 < got[4][0] < rows * n, "some blocks travel and some do not"
    assert np.array_equal(gate.state(), carried)
    gate.close()
