"""What the handle classes of the Python binding share: close() twice on every class, and the per-launch timing of the output gate and
the transmission splitter (set_timing / last_launch_ms), at 5 rows x 3 batches."""
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
], ids=["Demod", "Gather", "Mixer", "OutputGate", "TxSplit"])
def test_handle_closes_twice(pkg, make):
    closes_twice(make(pkg))


@gpu
@pytest.mark.parametrize("stage,launches", [("OutputGate", 3), ("TxSplit", 4)])
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
