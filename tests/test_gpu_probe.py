"""The channel probe on the GPU (mi_probe_*, csrc/probe.hip) against the model of tests/probe_model.py.

Pass criteria, the same in every case:
  windows, pairs  equal the model's;
  s1, s2          within 4 * wpc * 2^-53 of the model's value, relative.  Derived, not measured: the device adds the same float64 terms
                  in another order (256 strided partial sums and a halving tree, csrc/probe.hip; the model in window order); a float64
                  sum of n non-negative terms errs by at most (n - 1) * 2^-53 of the sum whatever its order, two orders differ by
                  twice that, and the 4 covers the final sums of partials;
  r_re, r_im      within 4 * wpc * 2^-53 * pair_scale absolutely, pair_scale = the sum of m_w * m_p over the cell's pairs: the terms
                  are signed, each at most m_w * m_p in size, and the same reordering bound holds with the sum of their sizes.
The output buffer holds a sentinel before a call and is longer than the call writes: the bytes behind the last record must still hold
it.  mi_probe_bytes_needed is checked against the survey's formula in every case, and the capture is exactly that long per stream."""
import functools

import numpy as np
import pytest

import probe_model as pm
import survey_model as sv

pytestmark = pytest.mark.gpu

SENT = 0xA5
GUARD = 256  # bytes allocated behind the last record
SAMPLE_BYTES = {sv.SFMT_U8: 2, sv.SFMT_S8: 2, sv.SFMT_S16: 4, sv.SFMT_F32: 8}  # one complex sample
EPS = 2.0 ** -53
CARRIERS = [(-700000, 0), (25000, 0), (901000, 0)]


def device(pkg, rate, log2n, sfmt=sv.SFMT_U8, fullscale=127.5):
    return pkg.device_cfg(sample_rate=rate, centerfreq=sv.CENTRE, fft_size_log=log2n, sfmt=sfmt, fullscale=fullscale)


class Run:
    """one handle and one capture in device memory: streams `stride` bytes apart from a base that is only sample-aligned.  raws[s] None:
    the stream has no target, lies last, and its region is 64 bytes of 0xFF -- shorter than any window"""

    def __init__(self, pkg, dev, raws, wpc, ncells, targets, max_targets=None, handle_wpc=None):
        """handle_wpc: what the handle is created with where that is not wpc itself (0 = the default cell, which wpc then states)"""
        import torch
        self.torch, self.dev, self.wpc, self.ncells, self.n = torch, dev, wpc, ncells, 1 << dev.fft_size_log
        self.ns = len(raws)
        sb = SAMPLE_BYTES[dev.sfmt]
        self.probe = pkg.Probe(dev, nstreams=self.ns, max_cells=ncells, windows_per_cell=wpc if handle_wpc is None else handle_wpc,
                               max_targets=max_targets or len(targets))
        need = self.probe.bytes_needed(ncells)
        hop_bytes = sv.hop_samples(dev.sample_rate) * sb
        assert need == (ncells * wpc - 1) * hop_bytes + sb * self.n, "mi_probe_bytes_needed against the survey's formula"
        self.stride = (need + 15) // 16 * 16 + 3 * sb  # no multiple of 16: the streams' bases differ in alignment
        off = sb
        assert all(r is not None for r in raws[:-1])
        last = 64 if raws[-1] is None else need
        host = np.zeros(off + (self.ns - 1) * self.stride + last, np.uint8)
        for s, raw in enumerate(raws):
            if raw is None:
                host[off + s * self.stride:] = 0xFF
                continue
            b = np.ascontiguousarray(raw).view(np.uint8)
            assert b.size >= need
            host[off + s * self.stride:off + s * self.stride + need] = b[:need]
        self.buf = torch.from_numpy(host).cuda()
        self.d_iq = self.buf.data_ptr() + off
        self.set_targets(targets)

    def set_targets(self, targets):
        self.probe.set_targets(targets)
        self.targets = [(int(s), int(b)) for s, b in targets]

    def output(self):
        return self.torch.full((len(self.targets) * self.ncells * 40 + GUARD,), SENT, dtype=self.torch.uint8, device="cuda")

    def call(self, stream=None, out=None):
        out = self.output() if out is None else out
        self.probe.process_device(self.d_iq, self.stride, self.ncells, out.data_ptr(), hip_stream=stream)
        return out

    def host(self, out):
        raw = out.cpu().numpy()
        nrec = len(self.targets) * self.ncells
        assert (raw[nrec * 40:] == SENT).all(), "bytes behind the last record were written"
        return raw[:nrec * 40].view(pm.CELL_DTYPE).reshape(len(self.targets), self.ncells)

    def close(self):
        self.probe.close()


def check(what, run, cells, raws):
    """every record against the model of its stream's capture"""
    worst = dict(s1=0.0, s2=0.0, r_re=0.0, r_im=0.0)
    for s in sorted({t[0] for t in run.targets}):
        idx = [k for k, t in enumerate(run.targets) if t[0] == s]
        want, scale = pm.probe_model(run.dev, raws[s], run.wpc, run.ncells, [run.targets[k][1] for k in idx])
        got = cells[idx]
        assert np.array_equal(got["windows"], want["windows"]) and np.array_equal(got["pairs"], want["pairs"]), f"{what}: stream {s}: windows / pairs"
        for name in ("s1", "s2"):
            tol = 4 * run.wpc * EPS * want[name]
            err = np.abs(got[name] - want[name])
            worst[name] = max(worst[name], float((err / np.maximum(tol, 1e-300)).max()))
            assert (err <= tol).all(), f"{what}: stream {s}: {name} off by {err.max():.3e} at (target, cell) {np.unravel_index(int((err - tol).argmax()), err.shape)}"
        for name in ("r_re", "r_im"):
            tol = 4 * run.wpc * EPS * scale
            err = np.abs(got[name] - want[name])
            worst[name] = max(worst[name], float((err / np.maximum(tol, 1e-300)).max()))
            assert (err <= tol).all(), f"{what}: stream {s}: {name} off by {err.max():.3e} at (target, cell) {np.unravel_index(int((err - tol).argmax()), err.shape)}"
    print(f"{what}: {len(run.targets)} targets x {run.ncells} cells of {run.wpc}: worst error over its tolerance " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert cells["pairs"][:, 0].tolist() == [run.wpc - 1] * len(run.targets), "cell 0 has wpc - 1 pairs"
    assert (cells["pairs"][:, 1:] == run.wpc).all()


@functools.lru_cache(maxsize=None)
def noise_raws(rate, log2n, sfmt, nwin, nstreams):
    """noise plus three carriers per stream (another seed each), in the case's format; read-only and shared"""
    from conftest import load_package
    pkg = load_package()
    dev = device(pkg, rate, log2n, sfmt)
    raws = [sv.as_format(sv.noise_and_carriers(pkg, rate, sv.samples_needed(dev, nwin), CARRIERS, stream=s, seed=0x5EED + 7 * s), sfmt) for s in range(nstreams)]
    for r in raws:
        r.setflags(write=False)
    return tuple(raws)


def noise_run(pkg, what, rate, log2n, sfmt, fullscale, wpc, ncells, nstreams, targets, idle_last=False, max_targets=None, handle_wpc=None):
    dev = device(pkg, rate, log2n, sfmt, fullscale)
    raws = list(noise_raws(rate, log2n, sfmt, wpc * ncells, nstreams))
    run = Run(pkg, dev, raws + ([None] if idle_last else []), wpc, ncells, targets, max_targets, handle_wpc)
    out = run.call()
    run.torch.cuda.synchronize()
    cells = run.host(out)
    check(what, run, cells, raws)
    return run, raws, out, cells


def test_fft256_u8_edge_and_neighbouring_bins(pkg):
    """cells of 40 windows, five of them: 200 windows = a tile of 128 and a short one of 72 (a whole piece and 8 windows), so every
    cell edge but one lies inside a tile and one cell straddles two; bins 0, N / 2 and N - 1, and neighbouring bins"""
    run, *_ = noise_run(pkg, "fft 256 u8", 2560000, 8, sv.SFMT_U8, 127.5, 40, 5, 1, [(0, b) for b in (0, 1, 127, 128, 129, 255)])
    run.close()


def test_fft256_single_target(pkg):
    run, *_ = noise_run(pkg, "fft 256 u8, one target", 2560000, 8, sv.SFMT_U8, 127.5, 40, 5, 1, [(0, 186)])
    run.close()


def test_fft512_u8_three_streams_one_idle_cell67(pkg):
    """cells of 67 windows -- no multiple of the tile or of a piece: tiles 128 + 73, the predecessor of window 128 in another tile and
    the one of window 134 in another cell --, targets on streams 0 and 2 of three, and behind them a fourth stream without a target
    whose region is 64 bytes of 0xFF"""
    targets = [(0, 5), (0, 372), (2, 180), (2, 181), (2, 511)]
    run, *_ = noise_run(pkg, "fft 512 u8, 3 streams + an idle one", 2560000, 9, sv.SFMT_U8, 127.5, 67, 3, 3, targets, idle_last=True)
    run.close()


@pytest.mark.parametrize("sfmt,rate,fullscale", [(sv.SFMT_S8, 2400000, 127.5), (sv.SFMT_S16, 2048000, 32767.0), (sv.SFMT_F32, 2560000, 2.0)],
                         ids=["s8-hop150", "s16-hop128", "f32-hop160"])
def test_fft512_formats_and_hops(pkg, sfmt, rate, fullscale):
    """the other three sample formats once each, with hops of 150, 128 and 160 samples"""
    run, *_ = noise_run(pkg, f"fft 512 format {sfmt}", rate, 9, sfmt, fullscale, 40, 5, 1, [(0, 0), (0, 60), (0, 256), (0, 372)])
    run.close()


def test_fft8192_u8(pkg):
    """1024 lanes to an FFT, twiddles fetched per pass, tiles of 16 windows: 13 of them over 200 windows, the last one short"""
    run, *_ = noise_run(pkg, "fft 8192 u8", 2560000, 13, sv.SFMT_U8, 127.5, 40, 5, 1, [(0, 0), (0, 80), (0, 4096), (0, 8191)])
    run.close()


def test_max_targets_and_set_targets_between_calls(pkg):
    """a handle made for 300 targets: first all 256 bins of stream 0 and 44 of stream 1 (more targets than an FFT has lanes: a lane takes
    up to 8), then, on the same handle, a list of three; the second call's records are the second list's and nothing behind them is
    written; a refused list leaves the one before it"""
    import torch
    full = [(0, b) for b in range(256)] + [(1, b) for b in range(100, 144)]
    run, raws, _, _ = noise_run(pkg, "fft 256 u8, 300 targets", 2560000, 8, sv.SFMT_U8, 127.5, 40, 5, 2, full, max_targets=300)
    few = [(0, 7), (1, 7), (1, 200)]
    run.set_targets(few)
    out = run.call()
    torch.cuda.synchronize()
    cells = run.host(out)
    check("after set_targets", run, cells, raws)
    for bad, text in (([(1, 7), (0, 7)], "strictly ascending"), ([(0, 7), (0, 7)], "strictly ascending"), ([(0, 9), (0, 8)], "strictly ascending"),
                      ([(2, 0)], "out of range"), ([(0, 256)], "out of range"), ([], "ntargets outside"), ([(0, b) for b in range(256)] + [(1, b) for b in range(45)],
                                                                                                            "ntargets outside")):
        with pytest.raises(pkg.MiError) as e:
            run.probe.set_targets(bad)
        assert e.value.code == pkg.MI_ERR_INVALID and text in str(e.value), str(e.value)
    again = run.call()
    torch.cuda.synchronize()
    assert torch.equal(out, again), "a refused list changed the targets"
    assert np.array_equal(run.probe.download(), cells)
    run.close()


def test_two_calls_side_stream_timing_and_refusals(pkg):
    """two calls of one handle into different buffers on a side stream without a host wait in between: byte-identical to each other and
    to a call on the NULL stream (the stage keeps no state, and its sums have a fixed order); download gives the same records;
    per-launch times are finite and positive; refused calls write nothing"""
    import torch
    run, raws, base, cells = noise_run(pkg, "NULL stream", 2560000, 9, sv.SFMT_U8, 127.5, 67, 3, 2, [(0, 5), (1, 180), (1, 372)])
    side = torch.cuda.Stream()
    a, b = run.output(), run.output()
    torch.cuda.synchronize()
    run.call(side.cuda_stream, a)
    run.call(side.cuda_stream, b)
    got = run.probe.download(side.cuda_stream)  # the one place that synchronises
    assert torch.equal(base, a) and torch.equal(a, b)
    assert got.tobytes() == cells.tobytes()
    with pytest.raises(pkg.MiError):
        run.probe.last_launch_ms()  # no timed call yet
    run.probe.set_timing(True)
    run.call(side.cuda_stream, a)
    ms = run.probe.last_launch_ms()
    print(f"fft 512, 3 targets x 3 cells of 67: windows {ms[0]:.4f} ms, reduce {ms[1]:.4f} ms")
    assert len(ms) == 2 and all(np.isfinite(m) and m > 0 for m in ms)
    run.probe.set_timing(False)
    assert torch.equal(a, base)

    fresh = run.output()
    torch.cuda.synchronize()

    def refused(text, fn):
        with pytest.raises(pkg.MiError) as e:
            fn()
        assert e.value.code == pkg.MI_ERR_INVALID and text in str(e.value), str(e.value)

    p = run.probe
    refused("8-byte aligned", lambda: p.process_device(run.d_iq, run.stride, 1, fresh.data_ptr() + 4))
    refused("ncells outside 1 .. max_cells", lambda: p.process_device(run.d_iq, run.stride, 0, fresh.data_ptr()))
    refused("ncells outside 1 .. max_cells", lambda: p.process_device(run.d_iq, run.stride, 4, fresh.data_ptr()))
    refused("one complex sample", lambda: p.process_device(run.d_iq + 1, run.stride, 1, fresh.data_ptr()))
    refused("NULL argument", lambda: p.process_device(None, run.stride, 1, fresh.data_ptr()))
    for gpu in (-1, torch.cuda.device_count()):
        refused("gpu index out of range", lambda: pkg.Probe(run.dev, gpu=gpu))
    unset = pkg.Probe(run.dev, nstreams=2, max_cells=3, windows_per_cell=67, max_targets=3)
    refused("no target list set", lambda: unset.process_device(run.d_iq, run.stride, 1, fresh.data_ptr()))
    refused("no mi_probe_process_device call", lambda: unset.download())
    unset.close()
    torch.cuda.synchronize()
    assert (fresh.cpu().numpy() == SENT).all(), "a refused call wrote"
    run.close()


def test_constant_input(pkg):
    """every byte pair equal: DC only, and all windows identical.  At bin 0 every term of r_im is im * re - re * im = 0 exactly, every
    term of r_re and of s2 is one value, and n equal terms add exactly in any order while n <= 2^29: the sums are n times the term, bit
    for bit -- a dropped or doubled window or pair shows here that a tolerance would hide.  Over cells 1 .. the coherence is 1 up to the
    float32 rounding of m (R_re holds re^2 + im^2 in float64, S2 the square of the float32 m)."""
    constant_input_case(pkg, 67, 3)


def test_constant_input_long_cells(pkg):
    """test_constant_input with cells of 600 windows, two of them: three trips of k_probe_reduce's strided loop, the last one partial
    (lanes 0 .. 87 add three terms, the others two).  The same equalities, bit for bit: a term that a later trip drops, doubles or takes
    from the neighbouring cell changes n.  n * m is exact for any float32 m; m * m and re^2 + im^2 have up to 48 bits, so for them
    "n equal terms add exactly" rests on the capture and the cell length: with every byte 201, adding 600 (in cell 0, 599) times the
    term in the kernel's order -- lane t the terms t, t + 256, t + 512, then the halving tree -- on the host in float64 gives n * term
    bit for bit in every sum this case asserts (worked out when the case was written; at 2000 windows s2 would round on the way)."""
    constant_input_case(pkg, 600, 2)


def constant_input_case(pkg, wpc, ncells):
    import torch
    dev = device(pkg, 2560000, 9)
    raw = np.full(2 * sv.samples_needed(dev, wpc * ncells), 201, np.uint8)
    run = Run(pkg, dev, [raw], wpc, ncells, [(0, 0), (0, 1)])
    out = run.call()
    torch.cuda.synchronize()
    cells = run.host(out)
    check("constant input", run, cells, [raw])
    z = sv.spectra(dev, raw, 0, 1)[0, 0].astype(np.float64)
    m = float(np.sqrt(np.float32(np.float32(z[0]) * np.float32(z[0]) + np.float32(z[1]) * np.float32(z[1]))))
    assert m > 0
    c = cells[0]
    assert (c["r_im"] == 0.0).all()
    assert c["s1"].tolist() == [wpc * m] * ncells and c["s2"].tolist() == [wpc * (m * m)] * ncells
    assert c["r_re"].tolist() == [p * (z[0] * z[0] + z[1] * z[1]) for p in [wpc - 1] + [wpc] * (ncells - 1)]
    f = pkg.probe_features_host(dev, 0, c, [0] + [1] * (ncells - 1))
    later = (ncells - 1) * wpc
    assert f.n == later and f.pairs == later and f.dphi == 0.0 and abs(f.coherence - 1.0) < 2.0 ** -22 and abs(f.cv2) < 1e-12
    run.close()


# ---- cells longer than k_probe_reduce's block: lane t adds the windows t, t + 256, ... of a cell, so from 257 windows on a lane adds more than one

@pytest.mark.parametrize("wpc", [256, 257, 600])
def test_fft256_long_cells(pkg, wpc):
    """cells of 256 windows (every lane one term, none a second), 257 (lane 0 alone takes a second term, the cell's last window) and
    600 (three trips, the last of 88 lanes), two cells each, so that a later trip of cell 0 that strays reads cell 1's windows and
    cell 1's first pair reaches back into cell 0; bins 0, N / 2, N - 1 and an inner one"""
    run, *_ = noise_run(pkg, f"fft 256 u8, cells of {wpc}", 2560000, 8, sv.SFMT_U8, 127.5, wpc, 2, 1, [(0, b) for b in (0, 77, 128, 255)])
    run.close()


def test_fft256_default_cell_is_2000_windows(pkg):
    """windows_per_cell = 0 is MI_WAVE_BATCH = 2000 windows, what a caller gets who asks for nothing: eight trips of the strided loop,
    the last of 208 lanes.  mi_probe_bytes_needed (checked in Run against the formula) and every record's `windows` say 2000."""
    run, _, _, cells = noise_run(pkg, "fft 256 u8, the default cell", 2560000, 8, sv.SFMT_U8, 127.5, 2000, 2, 1, [(0, 5), (0, 186)], handle_wpc=0)
    assert run.probe.windows_per_cell == 2000 and run.probe.bytes_needed(2) == (2 * 2000 - 1) * 160 * 2 + 2 * 256
    assert (cells["windows"] == 2000).all() and cells["pairs"].tolist() == [[1999, 2000]] * 2
    run.close()


# ---- cells of one window: every sum is one term, so nothing is reordered and the device gives the model's bits

ONE_LOG2N, ONE_CELLS, ONE_BINS = 9, 140, (0, 1, 180, 256, 511)  # (bin 180 holds the carrier at +901 kHz)


def test_single_window_cells_are_bit_exact(pkg):
    """fft 512, 140 cells of one window -- tiles 128 + 12, so cell 128's predecessor lies in another tile.  Each of s1, s2, r_re and
    r_im is 0.0 + one term: (double)m and its square with m = sqrtf(re * re + im * im) in float32, and cr * pr + ci * pi and
    ci * pr - cr * pi of float32 values in float64 -- exact products, one rounding.  The expected values are stated here from the
    oracle's spectra in exactly these forms and compared byte for byte; tests/probe_model.py forms them the same way and must agree
    byte for byte too.  Cell 0 has no pair and r_re = r_im = 0.0; every other cell has one, and its predecessor lies in the cell before.
    The same capture through a survey of one-window cells: its peak is the float32 m that s1 holds, bit for bit."""
    import torch
    n = 1 << ONE_LOG2N
    dev = device(pkg, 2560000, ONE_LOG2N)
    raw, = noise_raws(2560000, ONE_LOG2N, sv.SFMT_U8, ONE_CELLS, 1)
    run = Run(pkg, dev, [raw], 1, ONE_CELLS, [(0, b) for b in ONE_BINS])
    out = run.call()
    torch.cuda.synchronize()
    cells = run.host(out)

    z = sv.spectra(dev, raw, 0, ONE_CELLS)[:, list(ONE_BINS), :]  # float32 [window][target][2]
    re, im = np.ascontiguousarray(z[..., 0].T), np.ascontiguousarray(z[..., 1].T)  # [target][window]
    m = np.sqrt(re * re + im * im)
    assert m.dtype == np.float32 and (m > 0).all()
    md, cr, ci = m.astype(np.float64), re.astype(np.float64), im.astype(np.float64)
    pr, pi = np.roll(cr, 1, axis=1), np.roll(ci, 1, axis=1)
    want = np.zeros((len(ONE_BINS), ONE_CELLS), pm.CELL_DTYPE)
    want["s1"] = 0.0 + md
    want["s2"] = 0.0 + md * md
    want["r_re"] = 0.0 + (cr * pr + ci * pi)
    want["r_im"] = 0.0 + (ci * pr - cr * pi)
    want["r_re"][:, 0] = want["r_im"][:, 0] = 0.0
    want["windows"] = 1
    want["pairs"] = 1
    want["pairs"][:, 0] = 0
    model, _ = pm.probe_model(dev, raw, 1, ONE_CELLS, list(ONE_BINS))
    assert model.tobytes() == want.tobytes(), "tests/probe_model.py forms a term otherwise than this test states it"
    for name in ("windows", "pairs", "s1", "s2", "r_re", "r_im"):
        bad = np.argwhere(cells[name].view(np.uint64 if name[0] in "sr" else np.uint32) != want[name].view(np.uint64 if name[0] in "sr" else np.uint32))
        print(f"one-window cells: {name}: {len(bad)} of {want[name].size} records differ from the expected bits")
        assert len(bad) == 0, f"{name} differs first at (target, cell) {tuple(bad[0])}: {cells[name][tuple(bad[0])]!r} vs {want[name][tuple(bad[0])]!r}"
    assert cells.tobytes() == want.tobytes()
    assert (cells["pairs"][:, 0] == 0).all() and (cells["r_re"][:, 0] == 0.0).all() and (cells["r_im"][:, 0] == 0.0).all()
    assert (cells["pairs"][:, 1:] == 1).all() and (cells["r_re"][:, 1:] != 0.0).all()
    run.close()

    survey = pkg.Survey(dev, nstreams=1, max_cells=ONE_CELLS, windows_per_cell=1)
    assert survey.bytes_needed(ONE_CELLS) == raw.size
    iq = torch.from_numpy(np.array(raw)).cuda()
    mean = torch.zeros((ONE_CELLS, n), dtype=torch.float32, device="cuda")
    peak = torch.zeros_like(mean)
    survey.process_device(iq.data_ptr(), raw.size, ONE_CELLS, mean.data_ptr(), peak.data_ptr())
    torch.cuda.synchronize()
    peak_h = peak.cpu().numpy()[:, list(ONE_BINS)].T  # [target][cell]
    assert np.array_equal(peak_h.view(np.uint32), cells["s1"].astype(np.float32).view(np.uint32)), "the survey's peak is not the probe's m"
    assert np.array_equal(cells["s1"].astype(np.float32).astype(np.float64), cells["s1"]), "s1 of one window is a float32 value"
    survey.close()


def test_two_window_cells(pkg):
    """cells of two windows, 70 of them: every sum has two terms (cell 0's pair sums one), the tile edge at window 128 is a cell edge"""
    run, *_ = noise_run(pkg, "fft 512 u8, cells of 2", 2560000, ONE_LOG2N, sv.SFMT_U8, 127.5, 2, ONE_CELLS // 2, 1, [(0, b) for b in ONE_BINS])
    run.close()


# ---- the FFT sizes between 512 and 8192, each with its own tile length, and the fourth format at the largest size

PROBE_TILE_PIECES = 2  # kProbeTilePieces (csrc/probe.hip): a tile of k_probe is this many pieces of FftGeom::TW windows
SIZES_WPC, SIZES_CELLS = 70, 3


def tiles_of(log2n, wpc, ncells):
    """(tile length, length of the last tile, cells whose windows lie in more than one tile) of a call of k_probe"""
    tile = PROBE_TILE_PIECES * sv.fft_geom(log2n)["TW"]
    nwin = wpc * ncells
    return tile, nwin - (nwin - 1) // tile * tile, [c for c in range(ncells) if c * wpc // tile != ((c + 1) * wpc - 1) // tile]


def sizes_case(pkg, what, rate, log2n, sfmt, fullscale, nstreams, targets, want_tiles):
    assert tiles_of(log2n, SIZES_WPC, SIZES_CELLS) == want_tiles
    tile, last, straddling = want_tiles
    assert last < tile and straddling, "the case needs a short last tile and a cell that straddles two tiles"
    run, *_ = noise_run(pkg, what, rate, log2n, sfmt, fullscale, SIZES_WPC, SIZES_CELLS, nstreams, targets)
    run.close()


def test_fft1024_s16_hop128_every_bin_of_a_stream(pkg):
    """log2n 10: two FFTs to a workgroup, each over two waves, so the exchange is fenced by the workgroup's barrier.  210 windows =
    a tile of 128 and a short one of 82 (a whole piece and 18 windows); cell 1 (windows 70 .. 139) straddles the two.  Stream 0 has all
    1024 bins as targets: 128 lanes to an FFT, so every lane walks 8 of them; stream 1 has three."""
    targets = [(0, b) for b in range(1024)] + [(1, 0), (1, 513), (1, 1023)]
    sizes_case(pkg, "fft 1024 s16 hop 128, 1027 targets", 2048000, 10, sv.SFMT_S16, 32767.0, 2, targets, (128, 82, [1]))


def test_fft2048_s8_hop150(pkg):
    """log2n 11: the last size with the twiddles in registers, pieces of 32 windows.  210 windows = three tiles of 64 and a short one of
    18; every one of the three cells straddles a tile edge (64, 128, 192).  Hop 150: window starts that are only 4-byte aligned."""
    sizes_case(pkg, "fft 2048 s8 hop 150", 2400000, 11, sv.SFMT_S8, 127.5, 1, [(0, b) for b in (0, 1, 375, 1024, 1450, 2047)], (64, 18, [0, 1, 2]))


def test_fft4096_u8(pkg):
    """log2n 12: the first size that fetches its twiddles pass by pass, pieces of 16 windows.  210 windows = six tiles of 32 and a short
    one of 18; every cell straddles tile edges."""
    sizes_case(pkg, "fft 4096 u8", 2560000, 12, sv.SFMT_U8, 127.5, 1, [(0, b) for b in (0, 40, 1442, 2048, 2976, 4095)], (32, 18, [0, 1, 2]))


def test_fft8192_f32(pkg):
    """log2n 13 with 8-byte samples: the largest LDS the probe asks for at 2.56 MS/s (64 KB of span and 7 hops, 72 KB of exchange
    slot).  210 windows = thirteen tiles of 16 and a short one of 2."""
    assert sv.lds_bytes("probe", 13, sv.SFMT_F32, 160) == 149264 == max(sv.lds_bytes("probe", l, f, 160) for l in range(8, 14) for f in sv.COMPLEX_BYTES)
    sizes_case(pkg, "fft 8192 f32", 2560000, 13, sv.SFMT_F32, 2.0, 1, [(0, b) for b in (0, 80, 2883, 4096, 8191)], (16, 2, [0, 1, 2]))


# ---- the largest hop whose span still fits the LDS

def test_fft256_s16_largest_accepted_hop(pkg):
    """mi_probe_create accepts a geometry whose workgroup needs at most 160 KiB of LDS.  At fft 256 with s16 the largest such hop is
    568 samples (9.088 MS/s): 163 632 of 163 840 bytes.  The handle is made, the kernel launches with that much, and the records
    agree with the model; one hop more is refused at create."""
    hop = sv.largest_hop("probe", 8, sv.SFMT_S16)
    assert hop == 568 and sv.lds_bytes("probe", 8, sv.SFMT_S16, hop) == 163632
    run, *_ = noise_run(pkg, f"fft 256 s16 hop {hop}", hop * sv.WAVE_RATE, 8, sv.SFMT_S16, 32767.0, 70, 2, 1, [(0, b) for b in (0, 20, 128, 255)])
    run.close()
    with pytest.raises(pkg.MiError) as e:
        pkg.Probe(device(pkg, (hop + 1) * sv.WAVE_RATE, 8, sv.SFMT_S16, 32767.0), max_cells=2, windows_per_cell=70, max_targets=4)
    assert e.value.code == pkg.MI_ERR_INVALID and "over the limit of 163840" in str(e.value), str(e.value)


# ---- end to end: survey -> finder -> targets -> probe -> features -> classification -> plan, on one device-generated capture

E2E_LOG2N, E2E_WPC, E2E_CELLS, E2E_GATE_CELLS, E2E_AMP = 9, 200, 16, 4, 3072
# |carrier_hz - the generator's carrier| of the float64-DFT model on this capture (tools/probe_classes.py --fft 9 --amps 3072 --wpc 200
# --cells 16 --gate-cells 4): measured 57.75 Hz at most, on an NFM carrier (the mean of a frequency that swings 2.5 kHz either way, seen
# through a 5 kHz bin, over the windows of the active cells; the two AM carriers are within 1.8 Hz).  The margin is twice that.
E2E_F64_ERR_HZ = 58.0
E2E_MARGIN_HZ = 2 * E2E_F64_ERR_HZ


def test_end_to_end_classifies_and_plans(pkg):
    import torch
    n, hop = 1 << E2E_LOG2N, sv.hop_samples(pm.GATED_RATE)
    dev = device(pkg, pm.GATED_RATE, E2E_LOG2N)
    survey = pkg.Survey(dev, nstreams=1, max_cells=E2E_CELLS, windows_per_cell=E2E_WPC)
    need = survey.bytes_needed(E2E_CELLS)
    iq = torch.empty(need, dtype=torch.uint8, device="cuda")
    cfg = pkg.iqgen_cfg(sample_rate=pm.GATED_RATE, seed=0x5EED, noise_q8_mul=111, gate_samples=E2E_GATE_CELLS * E2E_WPC * hop,
                        carriers=[(off, kind, E2E_AMP, ph) for off, kind, ph in pm.GATED_CARRIERS])
    pkg.iqgen_device(cfg, 0, 1, need, 0, need // 2, iq.data_ptr())
    mean = torch.empty((1, E2E_CELLS, n), dtype=torch.float32, device="cuda")
    peak = torch.empty_like(mean)
    survey.process_device(iq.data_ptr(), need, E2E_CELLS, mean.data_ptr(), peak.data_ptr())
    occ = pkg.Occupancy(dev, nstreams=1, max_cells=E2E_CELLS)
    d_bins = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    d_cands = torch.empty(occ.max_candidates * 40, dtype=torch.uint8, device="cuda")
    d_first = torch.empty(2, dtype=torch.int32, device="cuda")
    d_count = torch.empty(2, dtype=torch.int32, device="cuda")
    occ.process_device(mean.data_ptr(), peak.data_ptr(), E2E_CELLS, d_bins.data_ptr(), d_cands.data_ptr(), d_first.data_ptr(), d_count.data_ptr())
    bins, cands, _, count = occ.download()
    want = sorted(pm.GATED_CARRIERS)
    assert count[0] == count[1] == len(want), f"{count[0]} candidates for {len(want)} carriers"
    targets = pkg.probe_targets_from_candidates(cands)
    probe = pkg.Probe(dev, nstreams=1, max_cells=E2E_CELLS, windows_per_cell=E2E_WPC, max_targets=len(targets))
    assert probe.bytes_needed(E2E_CELLS) == need
    probe.set_targets(targets)
    d_cells = torch.empty(len(targets) * E2E_CELLS * 40, dtype=torch.uint8, device="cuda")
    probe.process_device(iq.data_ptr(), need, E2E_CELLS, d_cells.data_ptr())
    cells = probe.download()
    mean_h = mean.cpu().numpy()[0]
    by_bin = {(round(off / (pm.GATED_RATE / n))) % n: (off, kind) for off, kind, _ in want}
    assert sorted(int(t["bin"]) for t in targets) == sorted(by_bin), "best_bin of every candidate is its carrier's strongest FFT bin"
    chans = []
    for k, t in enumerate(targets):
        b = int(t["bin"])
        off, kind = by_bin[b]
        mask = mean_h[:, b] > bins[0, b]["threshold"]
        assert 7 <= mask.sum() <= 9
        f = pkg.probe_features_host(dev, b, cells[k], mask)
        mod = pkg.probe_classify_host(f)
        print(f"carrier {off:+8d} Hz kind {kind} bin {b:3d}: coherence {f.coherence:.5f} cv2 {f.cv2:.5f} carrier_hz error {f.carrier_hz - sv.CENTRE - off:+8.2f} Hz "
              f"-> {'NFM' if mod else 'AM'}")
        assert mod == (pkg.MOD_AM if kind == 0 else pkg.MOD_NFM), f"carrier at {off} Hz of kind {kind} classified {mod}"
        assert abs(f.carrier_hz - (sv.CENTRE + off)) <= E2E_MARGIN_HZ
        chans.append(pkg.channel_cfg(int(round(f.carrier_hz)), modulation=mod, bandwidth=12500 if mod == pkg.MOD_NFM else 0))
    plan = pkg.Plan(dev, chans)
    for k, t in enumerate(targets):
        d = plan.channel(k)
        assert d.bin == int(t["bin"]) and d.modulation == chans[k].modulation
    plan.close()
    for h in (survey, occ, probe):
        h.close()
