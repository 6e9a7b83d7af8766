"""AFC (rtl_airband.cpp:180-251) on the GPU: every case of tests/afc_cases.py through the C ABI, checked two ways.

Against the oracle, bit for bit: audio, raw I/Q, flags, the counters and squelch levels of the final statistics, and the
device's afc_bin of every row after every call (read from the checkpoint blob).  And directly against the float64 model of
tests/afc_model.py fed the device's own flags: bins and '<' / '>' indicators -- which pins the device to the reference's
rule and not only to the oracle's restatement of it.

Calls of several batches are the default: only they reach the per-batch IQ offset of enqueue_afc and the per-batch offsets into
the output buffers.  That offset is 2100 or 2000 k windows times the hop in bytes: at hop 150 (300 bytes) every batch still starts
on a multiple of 16 and only windows inside a tile do not; at hop 151 (302 bytes) the second and third batch of the handle's
first call start 8 bytes off (2100 x 302 = 16 x 39637 + 8)."""
import ctypes as C

import numpy as np
import pytest

import afc_cases as ac
import afc_model as am
from common import AFC_BIN_OFFSET, AGC_EXTRA, PREV_AXC_OFFSET, WAVE_BATCH, assert_same, blob_rows

pytestmark = pytest.mark.gpu

CUTS = {8: (3, 1, 4), 10: (3, 1, 4, 2), 12: (3, 1, 5, 3)}
COUNTERS = ("open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter")


def read_bins(d):
    """(afc_bin, prev_axc) of every row, [nstreams][nch] each, from the checkpoint blob."""
    blob = d.get_state()
    _, state = blob_rows(blob, d.nstreams)
    rows = blob[32:32 + d.nstreams * d.nch * state].reshape(d.nstreams, d.nch, state)
    word = lambda off: np.ascontiguousarray(rows[:, :, off:off + 4]).view(np.uint32)[:, :, 0].astype(np.int64)
    return word(AFC_BIN_OFFSET), word(PREV_AXC_OFFSET)


class Collected:
    """What a run left, per stream: audio / flags / raw I/Q of the batches it took part in, the bins after each of its calls."""

    def __init__(self, case):
        ns = case.nstreams
        self.audio, self.flags, self.iq = [[] for _ in range(ns)], [[] for _ in range(ns)], [[] for _ in range(ns)]
        self.bins = [[] for _ in range(ns)]  # (batches done, afc_bin [nch])
        self.done = [0] * ns
        self.stats = None

    def take(self, s, k, wo, axc, iqo, bins):
        self.audio[s].append(np.asarray(wo)[:, :k * WAVE_BATCH].copy()), self.flags[s].append(np.asarray(axc).copy())
        self.iq[s].append(np.asarray(iqo).reshape(len(axc), -1).copy())
        self.done[s] += k
        self.bins[s].append((self.done[s], bins[s].copy()))


def host_run(pkg, case, cuts, d=None, got=None, close=True, max_batches=None):
    """mi_demod_process over the case, `cuts` batches per call."""
    dev, chans = case.device(pkg.device_cfg), case.channels(pkg.channel_cfg)
    d = d or pkg.Demod(dev, chans, nstreams=case.nstreams, max_batches=max_batches or max(cuts))
    got = got or Collected(case)
    for k in cuts:
        iqs = [case.capture(s)[ac.batch_pos(d.hop_bytes, got.done[s]):] for s in range(case.nstreams)]
        wo, axc, iqo, st = d.process(iqs, k, want_iq=True)
        bins, _ = read_bins(d)
        for s in range(case.nstreams):
            got.take(s, k, wo[s], axc[s], iqo[s], bins)
        got.stats = st
    if close:
        d.close()
    return d, got


def check(pkg, case, got, streams=None):
    chans = case.channels(pkg.channel_cfg)
    dev = case.device(pkg.device_cfg)
    for s in streams if streams is not None else range(case.nstreams):
        o = ac.oracle(case, s)
        nb = got.done[s]
        what = f"{case.name}, stream {s}"
        flags = np.concatenate(got.flags[s], axis=1)
        assert flags.shape[1] == nb
        # ---- the oracle, bit for bit
        assert_same(flags, o["flags"][:, :nb], f"{what}: flags")
        assert_same(np.concatenate(got.audio[s], axis=1), o["audio"][:, :nb * WAVE_BATCH], f"{what}: audio")
        iq = np.concatenate(got.iq[s], axis=1)
        for c, ch in enumerate(chans):
            if ch.has_iq_outputs:
                assert_same(iq[c], o["iq"][c, :nb * WAVE_BATCH * 2], f"{what}: raw I/Q of channel {c}")
        for done, bins in got.bins[s]:
            assert bins.tolist() == o["bins"][:, done - 1].tolist(), f"{what}: afc_bin after {done} batches"
        if got.stats is not None and nb == case.nbat:
            st = got.stats[s * len(chans):(s + 1) * len(chans)]
            assert [[getattr(x, f) for f in COUNTERS] for x in st] == o["counters"].tolist(), f"{what}: counters"
            assert_same(np.array([x.squelch_level for x in st], np.float32), o["levels"], f"{what}: squelch levels")
        # ---- the float64 model, fed the device's flags
        r = am.run(case.capture(s), dev, chans, flags)
        assert r.min_margin() > ac.MARGIN
        assert np.array_equal(flags, r.flags), f"{what}: flags {[bytes(f) for f in flags]}, model {[bytes(f) for f in r.flags]}"
        for done, bins in got.bins[s]:
            assert bins.tolist() == r.bins[:, done - 1].tolist(), f"{what}: afc_bin after {done} batches against the model"
        for c in range(len(chans)):
            want = case.expect(s, c)
            walks, returns = r.moved(c)
            assert (want == 0 and not walks) or (want != 0 and walks and (returns or nb < case.nbat)), f"{what}: channel {c} walks {walks} returns {returns}"


@pytest.mark.parametrize("name", list(ac.CASES))
def test_case_equals_the_oracle_and_the_model(pkg, name):
    case = ac.CASES[name]
    d, got = host_run(pkg, case, CUTS[case.nbat])
    check(pkg, case, got)


@pytest.mark.parametrize("cuts", [(1,) * 10, (10,)], ids=["one batch per call", "one call"])
def test_walk_rules_other_call_cuts(pkg, cuts):
    case = ac.CASES["walk_rules"]
    d, got = host_run(pkg, case, cuts)
    check(pkg, case, got)


def test_checkpoint_while_bins_are_moved(pkg):
    """get_state after the first 3 batches, where rows sit on moved bins, into a second handle that makes the remaining calls."""
    case = ac.CASES["walk_rules"]
    a, got = host_run(pkg, case, (3,), close=False)
    bins, prev = read_bins(a)
    base = np.array(case.base_bins())
    assert ((bins[0] != base) & (prev[0] != am.NO_SIGNAL)).sum() >= 10, "the checkpoint must be taken while bins are moved"
    blob = a.get_state()
    a.close()
    b = pkg.Demod(case.device(pkg.device_cfg), case.channels(pkg.channel_cfg), nstreams=1, max_batches=4)
    b.set_state(blob)
    assert read_bins(b)[0].tolist() == bins.tolist()
    host_run(pkg, case, (1, 4, 2), d=b, got=got)
    check(pkg, case, got)


def test_every_channel_type_on_the_device_entry(pkg):
    """mi_demod_process_device: IQ, audio, raw I/Q and flags in HBM, three calls of several batches."""
    import torch
    case = ac.CASES["types"]
    dev, chans = case.device(pkg.device_cfg), case.channels(pkg.channel_cfg)
    cuts = CUTS[case.nbat]
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(cuts))
    got = Collected(case)
    raw = case.capture(0)
    for k in cuts:
        part = raw[ac.batch_pos(d.hop_bytes, got.done[0]):][:d.bytes_needed(k)]
        assert part.size == d.bytes_needed(k)
        stride = (part.size + 255) // 256 * 256
        d_iq = torch.zeros(stride, dtype=torch.uint8, device="cuda")
        d_iq[:part.size] = torch.from_numpy(part.copy()).cuda()
        d_wo = torch.zeros((1, d.nch, k * WAVE_BATCH), dtype=torch.float32, device="cuda")
        d_io = torch.zeros((1, d.nch, k * WAVE_BATCH, 2), dtype=torch.float32, device="cuda")
        d_ax = torch.zeros((1, d.nch, k), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        d.process_device(d_iq.data_ptr(), stride, k, d_wo.data_ptr(), d_ax.data_ptr(), d_iq_out_ptr=d_io.data_ptr(),
                         hip_stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got.take(0, k, d_wo.cpu().numpy()[0], d_ax.cpu().numpy()[0], d_io.cpu().numpy()[0], read_bins(d)[0])
    got.stats = d.stats()
    d.close()
    check(pkg, case, got)


def test_every_channel_type_with_three_calls_in_flight(pkg):
    """mi_demod_submit three times, then mi_demod_wait three times."""
    case = ac.CASES["types"]
    dev, chans = case.device(pkg.device_cfg), case.channels(pkg.channel_cfg)
    cuts = (4, 4, 4)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=4)
    raw = case.capture(0)
    for i, k in enumerate(cuts):
        d.submit([raw[ac.batch_pos(d.hop_bytes, 4 * i):]], k, want_iq=True)
    got = Collected(case)
    for i, k in enumerate(cuts):
        wo, axc, iqo, st = d.wait()
        got.audio[0].append(wo[0][:, :k * WAVE_BATCH].copy()), got.flags[0].append(axc[0].copy()), got.iq[0].append(iqo[0].reshape(d.nch, -1).copy())
        got.done[0] += k
        got.stats = st
    got.bins[0].append((case.nbat, read_bins(d)[0][0]))
    d.close()
    check(pkg, case, got)


def test_65_rows_with_a_stream_sitting_calls_out(pkg):
    """5 streams x 13 channels: k_afc's second block.  Stream 2 sits two one-batch calls out: the others' batch 2, and their
    batch 5, in which they walk -- on the spectrum stage 1 left at the handle's index of each stream, not at its place in the
    launch.  Both times its rows sit on moved bins with a previous flag that is not NO_SIGNAL, and keep both, like all else
    they carry."""
    case = ac.CASES["rows65"]
    out, ns = 2, case.nstreams
    base = np.array(case.base_bins())
    lib, vp, sent = pkg.lib(), C.c_void_p, 0xEE
    d, got = host_run(pkg, case, (2,), close=False, max_batches=2)
    for _ in range(2):
        bins0, prev0 = read_bins(d)
        assert (bins0[out] != base).sum() >= 5 and (prev0[out][bins0[out] != base] != am.NO_SIGNAL).all()
        before = blob_rows(d.get_state(), ns)[0][out]
        d.set_active_streams([s != out for s in range(ns)])
        iqs = [None if s == out else case.capture(s)[ac.batch_pos(d.hop_bytes, got.done[s]):] for s in range(ns)]
        wo = np.full((ns, d.nch, WAVE_BATCH + AGC_EXTRA), np.float32(-7.0))
        iqo = np.full((ns, d.nch, WAVE_BATCH, 2), np.float32(-7.0))
        axc = np.full((ns, d.nch, 1), sent, np.uint8)
        ptrs = (C.c_void_p * ns)(*[None if a is None else a.ctypes.data for a in iqs])
        assert lib.mi_demod_process(d._h, ptrs, 1, wo.ctypes.data_as(vp), iqo.ctypes.data_as(vp), axc.ctypes.data_as(vp), None) == pkg.MI_OK, lib.mi_last_error()
        bins1, prev1 = read_bins(d)
        assert bins1[out].tolist() == bins0[out].tolist() and prev1[out].tolist() == prev0[out].tolist()
        assert np.array_equal(blob_rows(d.get_state(), ns)[0][out], before), "the state of the stream that sat out changed"
        assert (wo[out] == np.float32(-7.0)).all() and (iqo[out] == np.float32(-7.0)).all() and (axc[out] == sent).all()
        for s in range(ns):
            if s != out:
                got.take(s, 1, wo[s], axc[s], iqo[s], bins1)
        d.set_active_streams(None)
        host_run(pkg, case, (2,), d=d, got=got, close=False)
    d.close()
    assert got.done == [8 if s != out else 6 for s in range(ns)]
    walked = [b for s in range(ns) if s != out for b in range(8) if (ac.oracle(case, s)["flags"][:, b] == am.AFC_UP).any()]
    assert 5 in walked, "the second call without stream 2 must be one in which the others walk"
    got.stats = None  # (stream 2 has two batches less behind it than the oracle's counters)
    check(pkg, case, got)
