"""The channel finder on the GPU (mi_occupancy_*, csrc/occupancy.hip) against the numpy model of tests/occupancy_model.py and the host
twin mi_occupancy_plan_host.

One pass criterion everywhere: d_bins, d_cands, d_stream_first and d_count equal the model AND the twin byte for byte.  Every output
buffer holds a sentinel before a call and is longer than the call may write: the bytes behind the last stored candidate, behind the
last bin record, behind stream_first and count, and the whole bin region of a disabled stream must still hold it afterwards."""
import numpy as np
import pytest

import occupancy_model as om

pytestmark = pytest.mark.gpu

SENT = int(np.uint32(0xDEADBEEF).view(np.int32))
CENTRE = 120000000
NCELLS = [1, 2, 3, 5, 67, 257]  # 1 .. 5: fewer cells than waves; 67: no multiple of the wave count or the loads in flight; 257: a loop of chunks
SHAPES = {"fft256x1": (8, 1, None), "fft512x3": (9, 3, 1), "fft8192x1": (13, 1, None)}  # log2n, streams, the disabled stream


def dev_for(pkg, log2n):
    return pkg.device_cfg(sample_rate=2560000, centerfreq=CENTRE, fft_size_log=log2n)


class Outputs:
    """sentinel-filled device buffers, each longer than a call may write"""

    def __init__(self, torch, ns, n, slots):
        self.ns, self.n, self.slots = ns, n, slots
        full = lambda words: torch.full((words,), SENT, dtype=torch.int32, device="cuda")
        self.bins = full((ns * n + 2) * 8)
        self.cands = full((slots + 3) * 10)
        self.first = full(ns + 1 + 2)
        self.count = full(2 + 2)

    def host(self, pkg):
        return (self.bins.cpu().numpy().view(pkg.OCC_BIN_DTYPE), self.cands.cpu().numpy().view(pkg.OCC_CAND_DTYPE),
                self.first.cpu().numpy().view(np.uint32), self.count.cpu().numpy().view(np.uint32))


def sentinel(a):
    return (np.ascontiguousarray(a).view(np.uint32) == np.uint32(0xDEADBEEF)).all()


def check(pkg, what, out, want, twin, disabled):
    """out: Outputs after a synchronised call; want: the model's (bins, cands, first, count); twin: the host twin's, or None"""
    bins, cands, first, count = out.host(pkg)
    ns, n = out.ns, out.n
    want_bins, want_cands, want_first, want_count = want
    assert np.array_equal(count[:2], want_count), f"{what}: count {count[:2]} vs the model's {want_count}"
    assert np.array_equal(first[:ns + 1], want_first), f"{what}: stream_first {first[:ns + 1]} vs the model's {want_first}"
    assert sentinel(count[2:]) and sentinel(first[ns + 1:]), f"{what}: written behind count or stream_first"
    stored = int(want_count[1])
    assert stored <= out.slots
    bad = np.flatnonzero((cands[:stored].view(np.uint32) != want_cands[:stored].view(np.uint32)))
    assert bad.size == 0, f"{what}: candidate {bad[0] // 10} differs: {cands[bad[0] // 10]} vs the model's {want_cands[bad[0] // 10]}"
    assert sentinel(cands[stored:]), f"{what}: written behind the last stored candidate"
    for s in range(ns):
        got = bins[s * n:(s + 1) * n]
        if s == disabled:
            assert sentinel(got), f"{what}: a disabled stream's bin region was written"
            continue
        bad = np.flatnonzero(got.view(np.uint32) != want_bins[s].view(np.uint32))
        assert bad.size == 0, f"{what}: stream {s} bin {bad[0] // 8} differs: {got[bad[0] // 8]} vs the model's {want_bins[s][bad[0] // 8]}"
    assert sentinel(bins[ns * n:]), f"{what}: written behind the last bin record"
    if twin is not None:
        t_bins, t_cands, t_first, t_count = twin
        assert np.array_equal(t_count, count[:2]) and np.array_equal(t_first, first[:ns + 1])
        assert t_cands[:stored].tobytes() == cands[:stored].tobytes(), f"{what}: the device's candidates differ from the host twin's"
        for s in range(ns):
            if s != disabled:
                assert t_bins[s].tobytes() == bins[s * n:(s + 1) * n].tobytes(), f"{what}: the device's bin records differ from the host twin's"


def upload(torch, mean, peak):
    return torch.from_numpy(np.array(mean)).cuda(), torch.from_numpy(np.array(peak)).cuda()  # (copies: the shared planes are read-only)


def run_builder(pkg, occ, name, log2n, ncells, ns, disabled, permille=0, stream=None):
    """one call of `occ` (made with the builder's settings) on builder `name`'s planes, checked against the model and the twin"""
    import torch
    n = 1 << log2n
    mean, peak, cfg, cap = om.planes(name, n, ncells, ns)
    want = om.expected(name, n, ncells, ns, permille, disabled)
    enabled = None if disabled is None else [s != disabled for s in range(ns)]
    twin = pkg.occupancy_plan_host(dev_for(pkg, log2n), mean, peak, om.with_permille(cfg, permille), enabled, cap)
    d_mean, d_peak = upload(torch, mean, peak)
    out = Outputs(torch, ns, n, occ.max_candidates)
    torch.cuda.synchronize()
    occ.process_device(d_mean.data_ptr(), d_peak.data_ptr(), ncells, out.bins.data_ptr(), out.cands.data_ptr(), out.first.data_ptr(),
                       out.count.data_ptr(), hip_stream=stream)
    torch.cuda.synchronize()
    check(pkg, f"builder {name}, fft {n}, {ncells} cells, {ns} streams, disabled {disabled}", out, want, twin, disabled)
    return out, want


def handle_for(pkg, name, log2n, ns, disabled, max_cells, permille=0, ncells=1):
    """a handle with the settings and the capacity builder `name` asks for (at `ncells` cells, where they depend on that)"""
    n = 1 << log2n
    _, _, cfg, cap = om.planes(name, n, ncells, ns)
    occ = pkg.Occupancy(dev_for(pkg, log2n), nstreams=ns, max_cells=max_cells, cfg=om.with_permille(cfg, permille) if (cfg or permille) else None,
                        max_candidates=cap)
    if disabled is not None:
        occ.set_streams([s != disabled for s in range(ns)])
    return occ


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name", sorted(om.BUILDERS))
def test_builders_bit_for_bit(pkg, name, shape):
    """builders (a) .. (j) at every shape and every ncells of NCELLS, on one handle per case: the calls of a handle follow each other
    with growing ncells, so nothing of a call may depend on what the one before left in the handle.  Builder (g) runs with
    max_candidates below its count."""
    log2n, ns, disabled = SHAPES[shape]
    occ = None
    for ncells in NCELLS:
        if occ is None or name == "j":  # (j)'s min_cells goes with ncells: a handle per call
            if occ is not None:
                occ.close()
            occ = handle_for(pkg, name, log2n, ns, disabled, max(NCELLS), ncells=ncells)
        _, want = run_builder(pkg, occ, name, log2n, ncells, ns, disabled)
        if name == "g":
            assert want[3][0] > want[3][1] == occ.max_candidates
        if name == "e":
            assert want[3][0] == (ns if disabled is None else ns - 1) and (want[1]["nbins"] == 1 << log2n).all()
    occ.close()


@pytest.mark.parametrize("name,permille", [("c", 500), ("d", 1)])
def test_thousand_cells(pkg, name, permille):
    """1000 cells: 63 cells a wave, many rounds of the loads in flight; fft 512, three streams, stream 1 disabled"""
    occ = handle_for(pkg, name, 9, 3, 1, 1000, permille)
    run_builder(pkg, occ, name, 9, 1000, 3, 1, permille)
    occ.close()


@pytest.mark.parametrize("permille", [1, 500, 1000])
def test_other_order_statistics(pkg, permille):
    """the lowest, the median and the highest element as the floor, on the exponent-spread planes and the low-mantissa-bit planes"""
    for name in ("c", "d"):
        occ = handle_for(pkg, name, 8, 1, None, 67, permille)
        for ncells in (2, 67):
            run_builder(pkg, occ, name, 8, ncells, 1, None, permille)
        occ.close()


def test_side_stream_two_calls_and_timing(pkg):
    """a call on a side stream; then a short call after a long one into fresh buffers (nothing stale from the first: the second's
    outputs equal the model of its own planes); per-launch times are finite and positive; download returns what the buffers hold."""
    import torch
    occ = handle_for(pkg, "a", 9, 3, None, 257)
    side = torch.cuda.Stream()
    run_builder(pkg, occ, "a", 9, 257, 3, None, stream=side.cuda_stream)
    with pytest.raises(pkg.MiError):
        occ.last_launch_ms()  # no timed call yet
    occ.set_timing(True)
    out, want = run_builder(pkg, occ, "a", 9, 5, 3, None, stream=side.cuda_stream)
    ms = occ.last_launch_ms()
    print(f"fft 512, 3 streams x 5 cells: bin records {ms[0]:.4f} ms, run starts {ms[1]:.4f}, scan {ms[2]:.4f}, candidates {ms[3]:.4f}")
    assert len(ms) == 4 and all(np.isfinite(m) and m > 0 for m in ms)
    occ.set_timing(False)
    bins, cands, first, count = occ.download(side.cuda_stream)
    assert np.array_equal(count, want[3]) and np.array_equal(first, want[2])
    assert cands.tobytes() == want[1][:int(count[1])].tobytes() and bins.tobytes() == want[0].tobytes()
    occ.close()


def test_set_streams_between_calls(pkg):
    """all streams, then stream 0 disabled, then all again, on one handle: each call equals the model of its own mask, and a mask that
    enables no stream is refused and changes nothing"""
    occ = handle_for(pkg, "i", 9, 3, None, 67)
    run_builder(pkg, occ, "i", 9, 67, 3, None)
    occ.set_streams([0, 1, 1])
    run_builder(pkg, occ, "i", 9, 67, 3, 0)
    with pytest.raises(pkg.MiError) as e:
        occ.set_streams([0, 0, 0])
    assert e.value.code == pkg.MI_ERR_INVALID and "no stream enabled" in str(e.value)
    run_builder(pkg, occ, "i", 9, 67, 3, 0)
    occ.set_streams(None)
    run_builder(pkg, occ, "i", 9, 67, 3, None)
    occ.close()


def test_refusals_on_the_device(pkg):
    import torch
    occ = handle_for(pkg, "a", 8, 1, None, 4)
    mean, peak, _, _ = om.planes("a", 256, 3, 1)
    d_mean, d_peak = upload(torch, mean, peak)
    out = Outputs(torch, 1, 256, occ.max_candidates)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(mean=d_mean.data_ptr(), peak=d_peak.data_ptr(), ncells=3, bins=out.bins.data_ptr(),
                                                       cands=out.cands.data_ptr(), first=out.first.data_ptr(), count=out.count.data_ptr()).items()]

    def refused(text, **kw):
        with pytest.raises(pkg.MiError) as e:
            occ.process_device(*args(**kw))
        assert e.value.code == pkg.MI_ERR_INVALID and text in str(e.value), str(e.value)

    refused("ncells outside 1 .. max_cells", ncells=0)
    refused("ncells outside 1 .. max_cells", ncells=5)
    refused("16-byte aligned", mean=d_mean.data_ptr() + 4)
    refused("16-byte aligned", peak=d_peak.data_ptr() + 8)
    refused("16-byte aligned", bins=out.bins.data_ptr() + 8)
    refused("8-byte aligned", cands=out.cands.data_ptr() + 4)
    refused("NULL argument", count=None)
    with pytest.raises(pkg.MiError) as e:
        occ.download()
    assert "no mi_occupancy_process_device call" in str(e.value)
    for gpu in (-1, torch.cuda.device_count()):
        with pytest.raises(pkg.MiError) as e:
            pkg.Occupancy(dev_for(pkg, 8), gpu=gpu)
        assert e.value.code == pkg.MI_ERR_INVALID and "gpu index out of range" in str(e.value)
    torch.cuda.synchronize()
    assert all(sentinel(t.cpu().numpy()) for t in (out.bins, out.cands, out.first, out.count)), "a refused call wrote"
    occ.close()


def test_behind_the_survey(pkg):
    """End to end: mi_survey_* on om.e2e_capture (noise and four gated carriers, 2.56 MS/s, fft 512, u8, 16 cells of 200 windows), the
    finder on the survey's planes where they lie in device memory.  Bit-exact: the finder's outputs equal the model fed the downloaded
    planes.  Semantic: one candidate per carrier, each best_bin within one position of round(offset / (rate / N)) -- which the models
    alone give on this capture (tests/test_occupancy_model.py checks that without a GPU)."""
    import torch
    import survey_model as sv
    dev, u8, wpc, ncells = om.e2e_capture(pkg)
    n = 1 << dev.fft_size_log
    survey = pkg.Survey(dev, nstreams=1, max_cells=ncells, windows_per_cell=wpc)
    need = survey.bytes_needed(ncells)
    assert need == 2 * sv.samples_needed(dev, wpc * ncells) == u8.size
    d_iq = torch.from_numpy(u8).cuda()
    d_mean = torch.empty((1, ncells, n), dtype=torch.float32, device="cuda")
    d_peak = torch.empty_like(d_mean)
    occ = pkg.Occupancy(dev, nstreams=1, max_cells=ncells)
    out = Outputs(torch, 1, n, occ.max_candidates)
    torch.cuda.synchronize()
    survey.process_device(d_iq.data_ptr(), need, ncells, d_mean.data_ptr(), d_peak.data_ptr())
    occ.process_device(d_mean.data_ptr(), d_peak.data_ptr(), ncells, out.bins.data_ptr(), out.cands.data_ptr(), out.first.data_ptr(),
                       out.count.data_ptr())
    torch.cuda.synchronize()
    mean, peak = d_mean.cpu().numpy(), d_peak.cpu().numpy()
    want = om.finder(mean, peak)
    check(pkg, "behind the survey", out, want, pkg.occupancy_plan_host(dev, mean, peak), None)
    _, cands, _, count = occ.download()
    print("candidates:", [(int(c["best_bin"]), int(c["lo_bin"]), int(c["hi_bin"]), int(c["active_cells"]), int(c["first_cell"])) for c in cands])
    om.e2e_check(cands, n, dev.sample_rate)
    survey.close()
    occ.close()
