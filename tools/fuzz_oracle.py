"""Fuzz against the oracle over any seed range: the random plans and captures of tests/fuzz_plans.py mixed_plan (every channel type, odd
thresholds, carriers from under the squelch level to clipping, fft 256 .. 2048), product vs oracle: audio, flags, raw I/Q bit for bit.
Seeds 0-19 run in the suite (test_fuzz_mixed_plans_equal_the_oracle)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
from common import AGC_EXTRA, WAVE_BATCH, oracle_run  # noqa: E402
from fuzz_plans import mixed_plan  # noqa: E402  (the generator the suite runs: tests/test_bench_geometry.py)

pkg = conftest.load_package()
bad = 0
first, last = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (0, 40)
for seed in range(first, last):
    dev, chans, iq, nbat, per_call = mixed_plan(pkg, seed)
    nb, owo, oaxc, oiq = oracle_run(dev, chans, iq, nbat, want_iq=True)
    d = pkg.Demod(dev, chans, max_batches=per_call)
    outs, flags, zs = [], [], []
    for call in range(nbat // per_call):
        pos = 0 if call == 0 else (call * per_call * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        wo, ax, zo, _ = d.process([iq[pos:]], per_call, want_iq=True)
        outs.append(wo[:, :, :per_call * WAVE_BATCH].copy())
        flags.append(ax.copy())
        zs.append(zo.copy())
    d.close()
    wo = np.concatenate(outs, axis=2)
    ax = np.concatenate(flags, axis=2)
    zo = np.concatenate(zs, axis=2)
    same = nb == nbat and np.array_equal(ax[0], oaxc) and np.array_equal(wo[0], owo)
    for c, ch in enumerate(chans):
        if ch.has_iq_outputs:
            same = same and np.array_equal(zo[0, c].reshape(-1), oiq[c])
    if not same:
        bad += 1
        print("seed", seed, "MISMATCH", flush=True)
    if seed % 50 == 49:
        print("... seed", seed, "failures so far:", bad, flush=True)
print("oracle fuzz done, failures:", bad)
