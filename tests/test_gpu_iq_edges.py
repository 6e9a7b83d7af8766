"""What the I/Q span load (csrc/iq_front.hpp load_span, and the probe's own copy of it) promises at its edges: the result does not
depend on the alignment of the caller's base, and no byte outside [base, base + bytes_needed) reaches it.

The same I/Q is run twice.  First at a 16-byte-aligned base with zeros around it.  Then at a base one complex sample (2 bytes)
further into a buffer whose bytes in front of and behind the readable range are 0xFF: every 16-byte line the load takes whole then
starts 2 bytes early (mis = 2), and the first and the last line of the call hold bytes that are not the call's.  The two outputs
must be byte-equal.

Survey and probe: fft 256, u8, one stream, two cells of TW + 1 = 65 windows, so a tile walks a second piece of a single window
and the call ends in a short line.  Stage 1 on the exchange kernels (MI_OPT_LANE_FFT = 0): fft 512, the full graph and the pruned
one, one batch; mi_demod_process_device takes a base that is aligned to one complex sample, so stage 1 is part of the pin."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = 64  # bytes behind the readable range


def two_bases(torch, raw):
    """(aligned buffer, its base), (0xFF-filled buffer, a base 2 bytes past a 16-byte line) holding the same bytes"""
    flat = torch.zeros(raw.size + PAD, dtype=torch.uint8, device="cuda")
    flat[:raw.size] = torch.from_numpy(raw).cuda()
    host = np.full(2 + raw.size + PAD, 0xFF, np.uint8)
    host[2:2 + raw.size] = raw
    shifted = torch.from_numpy(host).cuda()
    assert flat.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 0
    return (flat, flat.data_ptr()), (shifted, shifted.data_ptr() + 2)


def capture(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes, dtype=np.uint8)


def test_survey_base_alignment_and_bytes_outside(pkg):
    import torch
    dev = pkg.device_cfg(sample_rate=2560000, fft_size_log=8)
    ncells, wpc, n = 2, 65, 256
    survey = pkg.Survey(dev, nstreams=1, max_cells=ncells, windows_per_cell=wpc)
    need = survey.bytes_needed(ncells)
    assert need == (ncells * wpc - 1) * 320 + 2 * n  # (a multiple of 16: from the shifted base the call ends 2 bytes into a line)
    out = []
    for buf, base in two_bases(torch, capture(need, 1)):
        mean = torch.zeros(ncells * n, dtype=torch.float32, device="cuda")
        peak = torch.zeros_like(mean)
        survey.process_device(base, need + 2, ncells, mean.data_ptr(), peak.data_ptr())
        torch.cuda.synchronize()
        out.append((mean.cpu().numpy().tobytes(), peak.cpu().numpy().tobytes()))
    survey.close()
    assert any(out[0][1]), "the survey wrote nothing"
    assert out[0] == out[1]


def test_probe_base_alignment_and_bytes_outside(pkg):
    import torch
    dev = pkg.device_cfg(sample_rate=2560000, fft_size_log=8)
    ncells, wpc, n = 2, 65, 256
    targets = [(0, 0), (0, 1), (0, 100), (0, 255)]
    probe = pkg.Probe(dev, nstreams=1, max_cells=ncells, windows_per_cell=wpc, max_targets=len(targets))
    probe.set_targets(targets)
    need = probe.bytes_needed(ncells)
    assert need == (ncells * wpc - 1) * 320 + 2 * n
    out = []
    for buf, base in two_bases(torch, capture(need, 2)):
        cells = torch.zeros(len(targets) * ncells * 40, dtype=torch.uint8, device="cuda")
        probe.process_device(base, need + 2, ncells, cells.data_ptr())
        out.append(probe.download().tobytes())
    probe.close()
    assert any(out[0]), "the probe wrote nothing"
    assert out[0] == out[1]


@pytest.mark.parametrize("prune", [0, 1])
def test_exchange_stage1_base_alignment_and_bytes_outside(pkg, prune):
    import torch
    centre, chans = pkg.config2_channels()
    dev = pkg.device_cfg(sample_rate=2560000, centerfreq=centre, fft_size_log=9)
    nb = 1
    raw = None
    out = []
    for which in range(2):
        demod = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)  # (a fresh handle each: a call leaves state behind)
        demod.set_option(pkg.OPT_LANE_FFT, 0)
        demod.set_option(pkg.OPT_PRUNE_FFT, prune)
        need = demod.bytes_needed(nb)
        raw = capture(need, 3) if raw is None else raw
        buf, base = two_bases(torch, raw)[which]
        wave = torch.zeros((len(chans), nb * 2000), dtype=torch.float32, device="cuda")
        axc = torch.zeros((len(chans), nb), dtype=torch.uint8, device="cuda")
        demod.process_device(base, need + 2, nb, wave.data_ptr(), axc.data_ptr())
        torch.cuda.synchronize()
        assert demod.last_stage1() == prune, "the exchange kernel asked for did not run"
        # stage 1's own output, the magnitude planes of the call's windows: audio behind a closed squelch would hide a difference
        planes = b"".join(demod.read_planes(0, ch, 0, nb * 2000)[0].tobytes() for ch in range(len(chans)))
        out.append((planes, wave.cpu().numpy().tobytes(), axc.cpu().numpy().tobytes()))
        demod.close()
    assert any(out[0][0]), "stage 1 wrote nothing"
    assert out[0] == out[1]
