"""What the handle classes of the Python binding share: close() twice on every class, and the per-launch timing of the output gate, the
transmission splitter, the tone finder, the PCM stage, the voice band stage and the limiter stage (set_timing / last_launch_ms), at 5 rows
x 3 batches."""
import math

import numpy as np
import pytest

from gate_model import WAVE_BATCH

gpu = pytest.mark.gpu
ROWS, NB = 5, 3


def closes_twice(h):
    assert h._h
    h.close()
    assert h._h is None
    h.close()
    assert h._h is None


def test_plan_closes_twice(pkg):
    centre, chans = pkg.config2_channels()
    closes_twice(pkg.Plan(pkg.device_cfg(centerfreq=centre), chans))


@gpu
@pytest.mark.parametrize("make", [
    lambda pkg: pkg.Demod(pkg.device_cfg(centerfreq=pkg.config2_channels()[0]), pkg.config2_channels()[1]),
    lambda pkg: pkg.Gather(None, 0, 1, 0, [1], ROWS, NB),
    lambda pkg: pkg.Mixer([(0, 1.0, 0.0), (1, 0.5, -0.5)]),
    lambda pkg: pkg.OutputGate(np.full(ROWS, pkg.GATE_OPEN, np.uint8), max_batches=NB),
    lambda pkg: pkg.TxSplit(np.ones(ROWS), max_batches=NB),
    lambda pkg: pkg.Tones(np.ones(ROWS), max_batches=NB),
    lambda pkg: pkg.Pcm(np.ones(ROWS), max_batches=NB),
    lambda pkg: pkg.Aspec(ROWS, max_batches=NB),
    lambda pkg: pkg.Vband(np.ones(ROWS), max_batches=NB),
    lambda pkg: pkg.Limit(np.ones(ROWS), max_batches=NB),
    lambda pkg: pkg.Survey(pkg.device_cfg(fft_size_log=8), nstreams=1, max_cells=1),
    lambda pkg: pkg.Occupancy(pkg.device_cfg(fft_size_log=8), nstreams=1, max_cells=1),
    lambda pkg: pkg.Probe(pkg.device_cfg(fft_size_log=8), nstreams=1, max_cells=1),
], ids=["Demod", "Gather", "Mixer", "OutputGate", "TxSplit", "Tones", "Pcm", "Aspec", "Vband", "Limit", "Survey", "Occupancy", "Probe"])
def test_handle_closes_twice(pkg, make):
    closes_twice(make(pkg))


@gpu
@pytest.mark.parametrize("stage,launches", [("OutputGate", 3), ("TxSplit", 4), ("Tones", 3), ("Pcm", 2), ("Vband", 2), ("Limit", 2)])
def test_launch_timing(pkg, stage, launches):
    import torch
    rng = np.random.default_rng(launches)
    wave = torch.from_numpy(rng.standard_normal((ROWS, NB * WAVE_BATCH)).astype(np.float32)).cuda()
    axc = torch.from_numpy(np.where(rng.random((ROWS, NB)) < 0.5, ord("*"), ord(" ")).astype(np.uint8)).cuda()
    row_first = torch.zeros(ROWS + 1, dtype=torch.int32, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if stage == "OutputGate":
        h = pkg.OutputGate(np.full(ROWS, pkg.GATE_OPEN, np.uint8), max_batches=NB)
        blocks = torch.zeros((ROWS * NB, WAVE_BATCH), dtype=torch.float32, device="cuda")
        index = torch.zeros((ROWS * NB, 2), dtype=torch.int32, device="cuda")

        def call():
            h.process_device(wave.data_ptr(), NB * WAVE_BATCH, axc.data_ptr(), NB, NB, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(),
                             count.data_ptr(), hip_stream=s)
            return h.download(s)[4]
    elif stage == "Tones":
        h = pkg.Tones(np.ones(ROWS), max_batches=NB)
        records = torch.zeros(h.max_records * pkg.TONE_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

        def call():
            h.process_device(wave.data_ptr(), NB * WAVE_BATCH, axc.data_ptr(), NB, NB, records.data_ptr(), row_first.data_ptr(), count.data_ptr(),
                             hip_stream=s)
            return h.download(s)[3]
    elif stage == "Pcm":
        h = pkg.Pcm(np.ones(ROWS), max_batches=NB)
        index, _, n, _ = pkg.gate_plan_host(np.full(ROWS, pkg.GATE_OPEN, np.uint8), axc.cpu().numpy())
        d_index = torch.from_numpy(np.ascontiguousarray(index).view(np.int32)).cuda()
        d_n = torch.from_numpy(n.view(np.int32)).cuda()
        blocks = torch.zeros(ROWS * NB * h.block_bytes, dtype=torch.uint8, device="cuda")

        def call():
            h.process_device(wave.data_ptr(), NB * WAVE_BATCH, NB, d_index.data_ptr(), d_n.data_ptr(), blocks.data_ptr(), hip_stream=s)
            return h.download(s)[1]
    elif stage in ("Vband", "Limit"):
        h = getattr(pkg, stage)(np.ones(ROWS), max_batches=NB)
        plane = torch.zeros_like(wave)

        def call():
            h.process_device(wave.data_ptr(), NB * WAVE_BATCH, NB, plane.data_ptr(), NB * WAVE_BATCH, hip_stream=s)
    else:
        h = pkg.TxSplit(np.ones(ROWS), max_batches=NB)
        records = torch.zeros(ROWS * (NB + 1) * pkg.TX_RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")

        def call():
            h.process_device(wave.data_ptr(), NB * WAVE_BATCH, axc.data_ptr(), NB, NB, records.data_ptr(), row_first.data_ptr(), count.data_ptr(),
                             hip_stream=s)
            return h.download(s)[2]
    with pytest.raises(pkg.MiError):  # no call at all
        h.last_launch_ms()
    call()
    with pytest.raises(pkg.MiError):  # a call, but not a timed one
        h.last_launch_ms()
    h.set_timing(True)
    call()
    ms = h.last_launch_ms()
    assert len(ms) == launches and all(math.isfinite(x) and x >= 0 for x in ms), ms
    h.set_timing(False)
    call()  # (still succeeds)
    with pytest.raises(pkg.MiError):
        h.last_launch_ms()
    closes_twice(h)
