"""The audio spectrum stage on the GPU (mi_aspec_*, csrc/aspec.hip) against the numpy restatement in aspec_model.py and against its
host twin mi_aspec_plan_host.

Every comparison is bit for bit: records, power rows, row means and row counts travel and are compared as bytes -- the FFT's graph
and the order of every sum are part of the definition.  The index, the row starts and the counts the stage reads are the ones an
output gate wrote on the same stream just before, with no host step between -- or, in run_by_hand, ones uploaded by hand that no
gate writes: more entries than the call's grid has workgroups, entries that are not of the call, row starts that what is stored
cuts.  The destinations are filled with a sentinel before a
call and are longer than the capacity the stage is told; what it must not write must still hold the sentinel afterwards."""
import numpy as np
import pytest

import aspec_model as am
import pcm_model as pm
from aspec_model import BINS, RECORD, WAVE_BATCH, aspec_model, audio
from common import AGC_EXTRA, bytes_for_batches
from gate_model import draw_flags, gate_model

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD = 2  # blocks allocated behind the capacity
GATE_OPEN, GATE_OPEN_TRAIL, GATE_ALL = 1, 2, 3


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def flags_for(rows, nb, seed, p_open=0.6):
    axc = draw_flags(np.random.default_rng(seed), rows, nb, p_open)
    axc[0, 0] = ord("*")  # (some block travels whatever was drawn)
    if rows > 2:
        axc[1, :] = ord(" ")  # (and a row without blocks)
    return axc


class Dest:
    """what the gate and the stage write for a call of rows x nb, the stage's part behind a capacity of `room` blocks"""

    def __init__(self, rows, nb, room, power=True, mean=True):
        import torch
        self.blocks = torch.empty((rows * nb, WAVE_BATCH), dtype=torch.float32, device="cuda")
        self.index = torch.full((rows * nb + GUARD, 2), SENT32, dtype=torch.int32, device="cuda")
        self.row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
        self.count = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.records = torch.full(((room + GUARD) * RECORD.itemsize,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.power = torch.full(((room + GUARD) * BINS * 4,), SENT_BYTE, dtype=torch.uint8, device="cuda") if power else None
        self.mean = torch.full((rows * BINS * 4,), SENT_BYTE, dtype=torch.uint8, device="cuda") if mean else None
        self.row_blocks = torch.full((rows * 4,), SENT_BYTE, dtype=torch.uint8, device="cuda") if mean else None


def run_call(pkg, spec, wave, axc, what, cap=0, pad=0, stream=None, rule=GATE_OPEN_TRAIL, power=True, mean=True, band=(0, 0)):
    """One gate call and one stage call back to back on one stream over buffers laid out for `pad` more batches than the call (filled
    with 0.5, flags open: a stage that read them would see something else); records, power rows, row means and row counts against
    the model over the gate's own index and against the twin, and the sentinels behind what was stored.  Returns the model's
    (records, power, mean, blocks)."""
    import torch
    rows, n = axc.shape
    lay = n + pad
    a = np.full((rows, lay), ord("*"), np.uint8)
    w = np.full((rows, lay * WAVE_BATCH), np.float32(0.5))
    a[:, :n], w[:, :n * WAVE_BATCH] = axc, wave[:, :n * WAVE_BATCH]
    rules = np.full(rows, rule, np.uint8)
    index, row_first, _ = gate_model(rules, axc)
    room = spec.max_blocks
    k = min(len(index), room)
    want = aspec_model(w, index, row_first, *band, nbatches=n, stored=k)
    twin = pkg.aspec_plan_host(rows, w, index[:k], row_first, *band, nbatches=n)
    for name, x, y in zip(("records", "power", "mean", "row counts"), want, twin):
        assert x.tobytes() == y.tobytes(), f"{what}: the twin's {name}"
    gate = pkg.OutputGate(rules, max_batches=n)
    cur = stream if stream is not None else torch.cuda.current_stream()
    s = cur.cuda_stream
    with torch.cuda.stream(cur):
        d_w, d_a = to_dev(w), to_dev(a)
        d = Dest(rows, n, room, power, mean)
    gate.process_device(d_w.data_ptr(), lay * WAVE_BATCH, d_a.data_ptr(), lay, n, d.blocks.data_ptr(), d.index.data_ptr(), d.row_first.data_ptr(),
                        d.count.data_ptr(), hip_stream=s)
    spec.process_device(d_w.data_ptr(), lay * WAVE_BATCH, n, d.index.data_ptr(), d.row_first.data_ptr() if mean else None, d.count.data_ptr(),
                        d.records.data_ptr(), d.power.data_ptr() if power else None, d.mean.data_ptr() if mean else None,
                        d.row_blocks.data_ptr() if mean else None, hip_stream=s)
    records, pw, mn, blocks, count = spec.download(s)
    assert np.array_equal(gate.download(s)[2], index), f"{what}: the gate's index is not the model's"
    gate.close()
    assert (int(count[0]), int(count[1])) == (len(index), k), f"{what}: counts {count}"
    assert records.tobytes() == want[0].tobytes(), f"{what}: records"
    raw = d.records.cpu().numpy()
    assert raw[:k * 32].tobytes() == want[0].tobytes() and (raw[k * 32:] == SENT_BYTE).all(), f"{what}: records on the device, or something behind record {k}"
    if power:
        assert pw.tobytes() == want[1].tobytes(), f"{what}: power rows"
        raw = d.power.cpu().numpy()
        assert raw[:k * BINS * 4].tobytes() == want[1].tobytes() and (raw[k * BINS * 4:] == SENT_BYTE).all(), f"{what}: power rows on the device"
    else:
        assert pw is None
    if mean:
        assert mn.tobytes() == want[2].tobytes(), f"{what}: row means"
        assert blocks.tobytes() == want[3].tobytes(), f"{what}: row counts"
        assert d.mean.cpu().numpy().tobytes() == want[2].tobytes() and d.row_blocks.cpu().numpy().tobytes() == want[3].tobytes()
    else:
        assert mn is None and blocks is None
    return want


@gpu
@pytest.mark.parametrize("rows", [1, 5, 70])
@pytest.mark.parametrize("nb", [1, 4])
def test_device_equals_model_and_twin(pkg, nb, rows):
    """Every builder.  1 row: one builder after the other; 5 rows: the same, every row that builder with its own seed; 70 rows, more
    workgroups than one batch has rows: row r takes builder r mod 13, so one call holds them all.  The index comes straight from
    mi_outgate_process_device under MI_GATE_OPEN_TRAIL with drawn flags; with more than two rows, row 1 has no block."""
    spec = pkg.Aspec(rows, max_batches=nb)
    assert spec.max_blocks == rows * nb
    for name in (["mixed"] if rows > 5 else list(am.BUILDERS)):
        want = run_call(pkg, spec, audio(name, rows, nb), flags_for(rows, nb, seed=rows * 10 + nb), f"{name}, {rows} rows, {nb} batches")
        assert len(want[0]) >= 1 and (rows <= 2 or want[3][1] == 0)
    spec.close()


@gpu
def test_capacity_smaller_than_the_gate_s_count(pkg):
    """max_blocks below what the gate stored: the first max_blocks records and power rows, nothing touched beyond, and a row whose
    slice the capacity cuts averages what was stored of it"""
    rows, nb = 5, 4
    axc = flags_for(rows, nb, seed=7, p_open=0.9)
    index, row_first, _ = gate_model(np.full(rows, GATE_OPEN_TRAIL, np.uint8), axc)
    r = next(r for r in range(2, rows) if row_first[r + 1] - row_first[r] >= 2)
    cap = int(row_first[r]) + 1
    cut = [r]
    assert 3 <= cap < len(index) and row_first[r] < cap < row_first[r + 1], "the capacity should end inside a row's slice"
    spec = pkg.Aspec(rows, max_batches=nb, max_blocks=cap)
    want = run_call(pkg, spec, audio("noise", rows, nb), axc, f"cap {cap} of {len(index)}")
    assert want[3][cut[0]] == cap - row_first[cut[0]] and (want[3][cut[0] + 1:] == 0).all() and want[3].sum() == cap
    spec.close()


@gpu
def test_without_power_rows_and_without_a_row_mean(pkg):
    """d_power NULL is accepted, records alone; power rows without a row mean; a row mean without the power rows, the row starts or
    the row counts is refused"""
    import torch
    rows, nb = 5, 2
    spec = pkg.Aspec(rows, max_batches=nb)
    wave, axc = audio("voice_whistle", rows, nb), flags_for(rows, nb, seed=5)
    both = run_call(pkg, spec, wave, axc, "records, power and mean")
    for power, mean in ((False, False), (True, False)):
        got = run_call(pkg, spec, wave, axc, f"power {power}, mean {mean}", power=power, mean=mean)
        assert got[0].tobytes() == both[0].tobytes()
    d = Dest(rows, nb, rows * nb)
    d_w = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    index, count = to_dev(am.full_index(rows, nb)[0]), to_dev(np.array([rows * nb] * 2, np.uint32))
    s = torch.cuda.current_stream().cuda_stream
    p = dict(d_power=d.power.data_ptr(), d_row_mean=d.mean.data_ptr(), d_row_blocks=d.row_blocks.data_ptr())
    for drop in ("d_power", "d_row_blocks", "d_row_first"):
        kw = {**p, "d_row_first": d.row_first.data_ptr(), drop: None}
        with pytest.raises(pkg.MiError) as e:
            spec.process_device(d_w.data_ptr(), nb * WAVE_BATCH, nb, index.data_ptr(), kw.pop("d_row_first"), count.data_ptr(), d.records.data_ptr(), hip_stream=s,
                                **kw)
        assert e.value.code == pkg.MI_ERR_INVALID and "row mean" in str(e.value), drop
    with pytest.raises(pkg.MiError) as e:  # row counts without a row mean
        spec.process_device(d_w.data_ptr(), nb * WAVE_BATCH, nb, index.data_ptr(), d.row_first.data_ptr(), count.data_ptr(), d.records.data_ptr(),
                            d_power=d.power.data_ptr(), d_row_blocks=d.row_blocks.data_ptr(), hip_stream=s)
    assert e.value.code == pkg.MI_ERR_INVALID
    torch.cuda.synchronize()
    assert (d.records.cpu().numpy() == SENT_BYTE).all() and (d.mean.cpu().numpy() == SENT_BYTE).all()  # a refused call writes nothing
    spec.close()


@gpu
def test_padded_strides_on_a_side_stream_and_another_band(pkg):
    """buffers laid out for three batches more than the call, everything enqueued on a side stream behind the uploads with no
    synchronisation before the download; then the same with a band of 300 .. 3000 Hz, whose bins are 39 and 384"""
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    rows, nb = 5, 3
    spec = pkg.Aspec(rows, max_batches=nb)
    run_call(pkg, spec, audio("voice", rows, nb), flags_for(rows, nb, seed=11), "padded, side stream", pad=3, stream=side)
    spec.close()
    assert pkg.aspec_band(300, 3000) == (39, 384)
    spec = pkg.Aspec(rows, max_batches=nb, lo_hz=300, hi_hz=3000)
    want = run_call(pkg, spec, audio("tone_lo", rows, nb), flags_for(rows, nb, seed=12), "band 300 .. 3000", pad=1, stream=side, band=(300, 3000))
    assert ((want[0]["peak_bin"] >= 39) & (want[0]["peak_bin"] <= 384)).all()  # (a tone below the band: what the band sees is its side lobes)
    spec.close()


@gpu
def test_two_calls_on_one_handle(pkg):
    """The stage is stateless: a call between two identical calls changes nothing in the second, and a shorter call on the same
    handle gives what a fresh handle gives"""
    rows, nb = 5, 4
    spec = pkg.Aspec(rows, max_batches=nb)
    axc = flags_for(rows, nb, seed=21)
    first = run_call(pkg, spec, audio("voice_whistle", rows, nb), axc, "first call")
    run_call(pkg, spec, audio("square", rows, 2), flags_for(rows, 2, seed=22), "a shorter call between")
    again = run_call(pkg, spec, audio("voice_whistle", rows, nb), axc, "the first call again")
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()
    spec.close()


def run_by_hand(pkg, spec, wave, index, count, row_first, stored, want, what, band=(0, 0), power=True, mean=True):
    """One call of FOREIGN_SHAPE's nbatches with an index, row starts and counts uploaded by hand (no gate) over an input laid out
    for the handle's max_batches, the destinations sentinel-filled with guard blocks behind the capacity: records, power rows, row
    means and row counts on the device and as downloaded against the model `want` and the twin over the first `stored` entries."""
    import torch
    rows, nb, mb = pm.FOREIGN_SHAPE
    room = spec.max_blocks
    assert stored == pm.stored_blocks(count, room) <= len(index) and spec.rows == rows and spec.max_batches == mb
    twin = pkg.aspec_plan_host(rows, wave, index[:stored], row_first, *band, nbatches=nb)
    for name, x, y in zip(("records", "power", "mean", "row counts"), want, twin):
        assert x is None or x.tobytes() == y.tobytes(), f"{what}: the twin's {name}"
    s = torch.cuda.current_stream().cuda_stream
    d = Dest(rows, mb, room, power, mean)
    d.index[:len(index)] = to_dev(index.view(np.int32))  # (what lies behind the entries holds the sentinel: of no call either)
    d_w, d_first, d_count = to_dev(wave), to_dev(row_first.view(np.int32)), to_dev(count.view(np.int32))
    spec.process_device(d_w.data_ptr(), mb * WAVE_BATCH, nb, d.index.data_ptr(), d_first.data_ptr() if mean else None, d_count.data_ptr(),
                        d.records.data_ptr(), d.power.data_ptr() if power else None, d.mean.data_ptr() if mean else None,
                        d.row_blocks.data_ptr() if mean else None, hip_stream=s)
    records, pw, mn, blocks, cnt = spec.download(s)
    assert (int(cnt[0]), int(cnt[1])) == (int(count[0]), stored), f"{what}: counts {cnt}"
    raw = d.records.cpu().numpy()
    got = raw[:stored * 32].view(RECORD)
    assert got.tobytes() == want[0].tobytes(), f"{what}: records on the device differ at {np.flatnonzero(got != want[0])}"
    assert (raw[stored * 32:] == SENT_BYTE).all(), f"{what}: something was written behind record {stored}"
    assert records.tobytes() == got.tobytes(), f"{what}: the records download returns"
    if power:
        raw = d.power.cpu().numpy()
        assert raw[:stored * BINS * 4].tobytes() == want[1].tobytes(), f"{what}: power rows on the device"
        assert (raw[stored * BINS * 4:] == SENT_BYTE).all(), f"{what}: something was written behind power row {stored}"
        assert pw.tobytes() == raw[:stored * BINS * 4].tobytes(), f"{what}: the power rows download returns"
    else:
        assert pw is None
    if mean:
        assert d.mean.cpu().numpy().tobytes() == want[2].tobytes(), f"{what}: row means on the device"
        assert d.row_blocks.cpu().numpy().tobytes() == want[3].tobytes(), f"{what}: row counts on the device"
        assert mn.tobytes() == want[2].tobytes() and blocks.tobytes() == want[3].tobytes(), f"{what}: the row means download returns"
    else:
        assert mn is None and blocks is None


@gpu
@pytest.mark.parametrize("lo_hz,hi_hz", [(0, 0), (300, 3000)])
@pytest.mark.parametrize("case", pm.FOREIGN_CASES)
def test_foreign_index_on_a_grid_shorter_than_the_count(pkg, case, lo_hz, hi_hz):
    """pcm_model.foreign_index, uploaded by hand: 3 rows on a handle of 8 batches, a call of 2, so 6 workgroups walk 20 entries (13
    under max_blocks 13; 24 under a count of 40), each making two to four trips over the same LDS with the window, the twiddles and
    the sample places it loaded once, and zero entries of every kind as first, middle and last trips; a row_first that is not a
    gate's, its slices cut by what is stored.  Every builder, three rows at a time; with a row mean, with the power rows alone and
    with records alone."""
    rows, nb, mb = pm.FOREIGN_SHAPE
    cap = pm.foreign_case(case)[3]
    spec = pkg.Aspec(rows, max_batches=mb, lo_hz=lo_hz, hi_hz=hi_hz, max_blocks=0 if cap == rows * mb else cap)
    assert spec.max_blocks == cap
    for group in range(am.FOREIGN_GROUPS):
        wave, index, count, row_first, _, stored, want = am.foreign_reference(case, group, lo_hz, hi_hz)
        assert min(rows * nb, cap) == 6 < stored and (want[0]["peak_bin"] == am.NONE).sum() == sum(k != "V" for k in pm.foreign_kinds(index[:stored], rows, nb, mb))
        for power, mean in ((True, True), (True, False), (False, False)) if group == 0 else ((True, True),):
            run_by_hand(pkg, spec, wave, index, count, row_first, stored, want if mean else want[:2] + (None, None),
                        f"{case}, group {group}, power {power}, mean {mean}", (lo_hz, hi_hz), power, mean)
    spec.close()


@gpu
def test_a_call_shorter_than_the_handle(pkg):
    """the ordinary short last call: 2 batches on a handle of 8 with the full valid index of 6, grid and count the same"""
    rows, nb, mb = pm.FOREIGN_SHAPE
    spec = pkg.Aspec(rows, max_batches=mb)
    index, row_first = am.full_index(rows, nb)
    wave = am.foreign_audio(3, rows, nb, mb)
    want = aspec_model(wave, index, row_first, nbatches=nb)
    run_by_hand(pkg, spec, wave, index, np.array([len(index)] * 2, np.uint32), row_first, len(index), want, "short call")
    spec.close()


@gpu
def test_out_of_range_entries_timing_and_argument_errors(pkg):
    """an index written by hand with entries that are not of the call: their records say so, their power rows are zero, nothing
    out of range is read; the timing calls; every argument check"""
    import torch
    rows, nb = 3, 2
    spec = pkg.Aspec(rows, max_batches=nb)
    wave = audio("noise", rows, nb)
    idx = np.array([[0, 0], [rows, 0], [1, nb], [2, 1], [0xFFFFFFFF, 0xFFFFFFFF], [0, 1]], np.uint32)
    first = np.array([0, 2, 4, 6], np.uint32)
    want = aspec_model(wave, idx, first)
    assert (want[0]["peak_bin"][[1, 2, 4]] == am.NONE).all() and not want[1][[1, 2, 4]].any()
    d = Dest(rows, nb, rows * nb)
    d_w = torch.zeros((rows, nb * WAVE_BATCH + 4), dtype=torch.float32, device="cuda")
    d_w[:, :nb * WAVE_BATCH] = to_dev(wave)
    index, row_first, count = to_dev(idx), to_dev(first), to_dev(np.array([len(idx)] * 2, np.uint32))
    s = torch.cuda.current_stream().cuda_stream

    def call(nbatches=nb, d_wave=d_w.data_ptr(), row_stride=nb * WAVE_BATCH + 4, d_index=index.data_ptr(), d_row_first=row_first.data_ptr(),
             d_count=count.data_ptr(), d_records=d.records.data_ptr(), d_power=d.power.data_ptr(), d_row_mean=d.mean.data_ptr()):
        spec.process_device(d_wave, row_stride, nbatches, d_index, d_row_first, d_count, d_records, d_power, d_row_mean, d.row_blocks.data_ptr(), hip_stream=s)

    for bad in (dict(nbatches=0), dict(nbatches=nb + 1), dict(d_wave=None), dict(d_index=None), dict(d_count=None), dict(d_records=None),
                dict(d_wave=d_w.data_ptr() + 4), dict(d_records=d.records.data_ptr() + 4), dict(d_power=d.power.data_ptr() + 8),
                dict(d_row_mean=d.mean.data_ptr() + 8), dict(d_index=index.data_ptr() + 4), dict(d_count=count.data_ptr() + 2),
                dict(d_row_first=row_first.data_ptr() + 2), dict(row_stride=nb * WAVE_BATCH + 2), dict(row_stride=nb * WAVE_BATCH - 4),
                dict(row_stride=WAVE_BATCH)):
        with pytest.raises(pkg.MiError) as e:
            call(**bad)
        assert e.value.code == pkg.MI_ERR_INVALID, bad
    with pytest.raises(pkg.MiError):
        spec.download(s)  # nothing was enqueued yet
    with pytest.raises(pkg.MiError):
        spec.last_launch_ms()
    spec.set_timing(True)
    call()
    records, pw, mn, blocks, cnt = spec.download(s)
    ms = spec.last_launch_ms()
    print("blocks / rows ms:", ms)
    assert len(ms) == 2 and all(m >= 0 for m in ms) and tuple(cnt) == (6, 6)
    for name, got, x in zip(("records", "power", "mean", "row counts"), (records, pw, mn, blocks), want):
        assert got.tobytes() == x.tobytes(), name
    assert (d.records.cpu().numpy()[6 * 32:] == SENT_BYTE).all() and (d.power.cpu().numpy()[6 * BINS * 4:] == SENT_BYTE).all()
    for kw in (dict(max_batches=0), dict(lo_hz=4000), dict(hi_hz=8000), dict(rows=0), dict(rows=1 << 20), dict(rows=1 << 12, max_batches=1 << 12)):
        with pytest.raises(pkg.MiError) as e:
            pkg.Aspec(**{"rows": 5, "max_batches": 2, **kw})
        assert e.value.code == pkg.MI_ERR_INVALID, kw
    spec.close()


@gpu
def test_behind_the_demodulator_the_vote_finds_the_tone_and_the_notch_removes_it(pkg):
    """1 stream x 1 AM channel x 12 batches of an always-on mi_iqgen AM carrier of kind 0 (a 1 kHz tone at half depth): demodulator,
    gate under MI_GATE_OPEN and the stage back to back on one stream; the vote over the row's mean must find a line within one bin
    of 1000 Hz.  A second demodulator whose channel carries that frequency as its notch (Q 10, the reference's default) over the
    same capture must leave less mean power in the vote's bin.  The size of the drop is printed, not asserted."""
    import torch
    nb, centre, offset = 12, 120000000, 250000
    dev = pkg.device_cfg(centerfreq=centre)
    nbytes = (bytes_for_batches(dev, nb) + 255) // 256 * 256
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=0, carriers=[(offset, 0, 3072, 0)])
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(cfg, 0, 1, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    spec = pkg.Aspec(1, max_batches=nb)

    def chain(notch, notch_q):
        chans = [pkg.channel_cfg(centre + offset, squelch_threshold_dbfs=-45, notch=notch, notch_q=notch_q)]
        dm = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
        gate = pkg.OutputGate(np.array([GATE_OPEN], np.uint8), max_batches=nb)
        wo = torch.zeros((1, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
        ax = torch.zeros((1, nb), dtype=torch.uint8, device="cuda")
        d = Dest(1, nb, nb)
        dm.process_device(d_iq.data_ptr(), nbytes, nb, wo.data_ptr(), ax.data_ptr(), hip_stream=s)  # (no host synchronisation from here to the download)
        gate.process_device(wo.data_ptr(), nb * WAVE_BATCH, ax.data_ptr(), nb, nb, d.blocks.data_ptr(), d.index.data_ptr(), d.row_first.data_ptr(),
                            d.count.data_ptr(), hip_stream=s)
        spec.process_device(wo.data_ptr(), nb * WAVE_BATCH, nb, d.index.data_ptr(), d.row_first.data_ptr(), d.count.data_ptr(), d.records.data_ptr(),
                            d.power.data_ptr(), d.mean.data_ptr(), d.row_blocks.data_ptr(), hip_stream=s)
        records, pw, mn, blocks, count = spec.download(s)
        index, row_first = gate.download(s)[2:4]
        audio_, flags = wo.cpu().numpy(), ax.cpu().numpy()
        dm.close()
        gate.close()
        print("flags:", bytes(flags[0]).decode(), " blocks:", int(blocks[0]))
        want = aspec_model(audio_, index, row_first)
        twin = pkg.aspec_plan_host(1, audio_, index, row_first)
        for name, got, x, y in zip(("records", "power", "mean", "row counts"), (records, pw, mn, blocks), want, twin):
            assert got.tobytes() == x.tobytes() == y.tobytes(), name
        return records, mn[0], int(blocks[0])

    records, mean, blocks = chain(0.0, 0.0)
    vote = pkg.aspec_notch_host(mean, blocks, records)
    model = am.notch_model(mean, blocks, records)
    print(f"vote: found {vote.found} bin {vote.bin} freq {vote.freq_hz:.3f} Hz peak {vote.peak:.6g} floor {vote.floor:.6g} votes {vote.votes} of {vote.blocks}")
    assert (vote.found, vote.bin, vote.freq_hz, vote.peak, vote.floor, vote.votes, vote.blocks) == tuple(model[k] for k in ("found", "bin", "freq_hz", "peak", "floor", "votes", "blocks"))
    assert vote.found == 1 and abs(vote.freq_hz - 1000.0) < am.HZ_PER_BIN
    _, notched, blocks2 = chain(float(vote.freq_hz), 10.0)
    print(f"mean power in bin {vote.bin}: {mean[vote.bin]:.6g} without the notch, {notched[vote.bin]:.6g} with it ({10 * np.log10(notched[vote.bin] / mean[vote.bin]):.1f} dB), "
          f"{blocks2} blocks")
    assert blocks2 >= 1 and notched[vote.bin] < mean[vote.bin]
    spec.close()
