#!/usr/bin/env python3
"""What the ELT detector stage's default settings rest on.  No GPU: everything runs through the host twin
mi_elt_plan_host, which is the device's bytes.

Prints, for the defaults:
  - decode probability against tone-to-noise ratio (the beacon's power over white noise's, full band) from +12 dB down in 2 dB steps
    to where onsets stop, --seeds seeds each, on the 3 Hz beacon of tests/elt_model.py over 5 s;
  - false events per hour on white noise, voice-like audio, SELCAL-like tone pairs and ACARS-like bursts (1200 / 2400 Hz MSK keyed in
    bursts of 0.7 s), --minutes minutes each;
  - onset latency in seconds at 2, 3 and 4 Hz (a clean beacon from sample 0);
  - what a beacon behind the AM demodulator's AGC looks like: the tonal share of frames over the end-to-end capture of
    tests/elt_model.py through the CPU oracle (skipped where the oracle is not built).
Synthetic signals only: no off-air beacon has been through the stage.
"""
import argparse
import os
import sys

import numpy as np

from rate_common import WAVE_BATCH, load_package

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

RATE = 16000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    ap.add_argument("--minutes", type=float, default=10.0)
    args = ap.parse_args()
    from elt_model import NONE8, ONSET, beacon, e2e_setup, tone, voice_like
    pkg = load_package()

    def run(x, state=None):
        return pkg.elt_plan_host([1], np.asarray(x, np.float32)[None, :], state=state)

    n = 40 * WAVE_BATCH
    amp = 0.3
    print("tone-to-noise dB   onsets / seeds   tonal share of frames")
    for db in range(12, -14, -2):
        sigma = amp / np.sqrt(2.0) / 10 ** (db / 20.0)
        hits, share = 0, []
        for seed in range(args.seeds):
            events, frames, _, _, _ = run(beacon(n, amp=amp, sigma=sigma, seed=100 + seed))
            hits += int((events["kind"] == ONSET).any())
            share.append((frames["bin"] != NONE8).mean())
        print(f"  {db:+4d}              {hits:3d} / {args.seeds}        {np.mean(share):.3f}")
        if hits == 0:
            break
    nb = int(args.minutes * 60 * RATE / WAVE_BATCH)
    part = 600  # batches a piece

    def selcal_like(m, seed):
        rng = np.random.default_rng(seed)
        x = np.zeros(m)
        for s0 in range(0, m - 3 * RATE, 4 * RATE):
            for k in range(2):
                fa, fb = rng.choice([312.6, 384.6, 473.2, 582.1, 716.1, 881.0, 1083.9, 1333.5], 2, replace=False)
                a = s0 + k * 19200
                x += tone(m, fa, 0.2, a, a + RATE) + tone(m, fb, 0.2, a, a + RATE)
        return x

    def acars_like(m, seed):
        rng = np.random.default_rng(seed)
        x = np.zeros(m)
        length = int(0.7 * RATE)
        for s0 in range(RATE, m - RATE, 3 * RATE):
            bits = rng.integers(0, 2, int(0.7 * 2400) + 1)
            f = np.where(bits[np.arange(length) * 2400 // RATE], 1200.0, 2400.0)
            x[s0:s0 + length] = 0.3 * np.sin(2.0 * np.pi * np.cumsum(f) / RATE)
        return x

    kinds = (("white noise", lambda m, seed: np.random.default_rng(seed).normal(0.0, 0.2, m)), ("voice-like", voice_like), ("SELCAL-like pairs", selcal_like),
             ("ACARS-like bursts", acars_like))
    print(f"false events per hour over {args.minutes:g} minutes each")
    for name, make in kinds:
        state, total, tonal = None, 0, []
        for p in range(0, nb, part):
            m = min(part, nb - p) * WAVE_BATCH
            events, frames, _, _, state = run(make(m, 200 + p), state)
            total += len(events)
            tonal.append((frames["bin"] != NONE8).mean())
        print(f"  {name:20s} {total * 60.0 / args.minutes:6.1f}   (tonal share of frames {np.mean(tonal):.3f})")
    print("onset latency, a clean beacon from sample 0")
    for rate in (2.0, 3.0, 4.0):
        events = run(beacon(n, rate))[0]
        print(f"  {rate:g} Hz: {0.005 * (int(events[0]['frame']) + 1):.3f} s" if len(events) else f"  {rate:g} Hz: no onset")
    try:
        from common import oracle_run
        dev, chans, iq, nbat = e2e_setup(pkg)
        _, wo, axc, _ = oracle_run(dev, chans, iq, nbat)
        events, frames, _, _, _ = pkg.elt_plan_host([1], wo[:1])
        print(f"behind the AM demodulator's AGC (80 % modulation, 3 Hz): tonal share {(frames['bin'] != NONE8).mean():.3f}, peak |audio| {np.abs(wo[0]).max():.2f}, "
              f"events {[pkg.elt_event_text(e) for e in events]}")
    except Exception as e:  # the oracle is a build product
        print(f"behind the AM demodulator's AGC: skipped ({e})")


if __name__ == "__main__":
    main()
