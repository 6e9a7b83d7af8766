#!/usr/bin/env python3
"""Where the noise reduction stage's default `over` comes from and what the defaults do: mi_denoise_plan_host
on the seeded signals of tests/denoise_model.py.  No GPU.

  1. mean(S) / mean(m) on white Gaussian noise of --seconds seconds at three levels.  The twin runs one batch a call; the last row of
     the state blob behind a call is that batch's M, and m is the minimum over the eight rows that end with it.  S is restated here in
     float64 (numpy.fft.rfft of the windowed frames); its mean runs over every frame from the second on, m's over every batch from
     the eighth on.  The default `over` is the mean of the three ratios, rounded up to the next 0.5.
  2. the steady-state reduction of that noise at the default row: output over input level in the last second of three.
  3. the change in level of a 1 kHz tone 10 dB above the noise in its bin, by float64 projections over the same second.
  4. the reconstruction error at reduction_db 0 and at over 0: the largest |out[n] - x[n - 250]| over the largest |x|.
Prints a table and one JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import denoise_model as dm  # noqa: E402
from rate_common import load_package  # noqa: E402

WAVE_BATCH = dm.WAVE_BATCH
SECOND = 8  # batches


def floor_ratio(pkg, wave):
    """mean(S) / mean(m) of one row"""
    nb = wave.shape[1] // WAVE_BATCH
    state, floors = None, []
    for b in range(nb):
        _, state = pkg.denoise_plan_host([1], wave[:, b * WAVE_BATCH:(b + 1) * WAVE_BATCH], None, state)
        floors.append(state.view(pkg.DENOISE_STATE_DTYPE)["m"][0, -1].astype(np.float64))
    floors = np.array(floors)
    m = np.array([floors[b - dm.DEPTH + 1:b + 1].min(axis=0) for b in range(dm.DEPTH - 1, nb)])
    x = np.concatenate([np.zeros(dm.FRAME), wave[0].astype(np.float64)])
    X = np.fft.rfft(dm._frames(x[None], nb)[0] * dm.window64(), dm.FFT, axis=-1)
    P = X.real ** 2 + X.imag ** 2
    T = P[:, dm.LOWER] + P + P[:, dm.UPPER]
    S = T[1:-1] + T[2:]  # (from the second frame on: the first holds the zeros before the signal)
    return float(S.mean() / m.mean())


def last_second(x):
    return x[-SECOND * WAVE_BATCH:]


def measure(pkg, seconds=20, seed=0):
    ratios = [floor_ratio(pkg, dm.gaussian(1, seconds * SECOND * WAVE_BATCH, sigma, 9000 + 10 * seed + i)) for i, sigma in enumerate(dm.NOISE_SIGMAS)]
    over = math.ceil(2.0 * float(np.mean(ratios))) / 2.0
    noise = dm.noise_at(1)(1, 3 * SECOND, seed)
    out, _ = pkg.denoise_plan_host([1], noise)
    reduction = dm.level_db(last_second(out[0])) - dm.level_db(last_second(noise[0]))
    tone = dm.tone_in_noise(1, 3 * SECOND, seed)
    out, _ = pkg.denoise_plan_host([1], tone)
    tone_db = 20.0 * math.log10(dm.tone_level(last_second(out[0])) / dm.tone_level(last_second(tone[0])))
    errs = {}
    for name, cfg in (("reduction_db 0", (0.0, pkg.denoise_default_row()[1])), ("over 0", (pkg.denoise_default_row()[0], 0.0))):
        errs[name] = 0.0
        for builder in ("noise_mid", "voice_in_noise", "square"):
            x = dm.audio(builder, 1, SECOND)
            out, _ = pkg.denoise_plan_host([1], x, cfg)
            errs[name] = max(errs[name], float(np.abs(out[0, dm.HOP:].astype(np.float64) - x[0, :-dm.HOP]).max() / np.abs(x).max()))
    return dict(ratios=ratios, over=over, reduction_db=reduction, tone_db=tone_db, reconstruction=errs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    pkg = load_package()
    r = measure(pkg, args.seconds, args.seed)
    print(f"default row {pkg.denoise_default_row()}; synthetic signals only")
    for sigma, ratio in zip(dm.NOISE_SIGMAS, r["ratios"]):
        print(f"  white noise, sigma {sigma:5.3f}, {args.seconds} s: mean(S) / mean(m) = {ratio:.3f}")
    print(f"  mean of the three {np.mean(r['ratios']):.3f} -> over = {r['over']:.1f}")
    print(f"  white noise, sigma {dm.NOISE_SIGMAS[1]}, last second of three: {r['reduction_db']:+.2f} dB")
    print(f"  1 kHz tone 10 dB above the noise in its bin, last second of three: {r['tone_db']:+.2f} dB")
    for name, e in r["reconstruction"].items():
        print(f"  {name}: largest |out[n] - x[n - 250]| / max |x| = {e:.3e}")
    print(json.dumps(dict(tool="denoise_classes", seconds=args.seconds, seed=args.seed, **r)))


if __name__ == "__main__":
    main()
