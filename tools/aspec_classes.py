#!/usr/bin/env python3
"""Where mi_aspec_notch_host's ratio lies: peak / floor of the vote on the audio builders of
tests/aspec_model.py, with the numpy model alone.  No GPU.

One row of --blocks blocks per case and seed: the voice-like signal with a steady 1000 Hz whistle at several levels relative to the
voice's mean power, the voice-like signal alone, uniform noise alone, and a constant (a DC offset, whose side lobes are what the
band sees).  Printed per case: the vote's bin and frequency, peak, floor, peak / floor and whether the default rule (8 blocks, ratio
16) finds a line; then a JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import aspec_model as am  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--levels", type=float, nargs="+", default=[0.0, -6.0, -10.0, -14.0, -20.0, -30.0])
    args = ap.parse_args()
    nb = args.blocks
    index, first = am.full_index(1, nb)
    cases = [(f"voice + whistle {db:+.0f} dB", lambda seed, db=db: am.voice(1, nb, seed, whistle_db=db)) for db in args.levels]
    cases += [("voice alone", lambda seed: am.voice(1, nb, seed)), ("noise alone", lambda seed: am.noise(1, nb, seed)),
              ("constant 0.5", lambda seed: am.constant(1, nb, seed))]
    result = dict(tool="aspec_classes", blocks=nb, cases=[])
    print(f"{nb} blocks a row, default rule: min_blocks {am.DEFAULT_MIN_BLOCKS}, ratio {am.DEFAULT_RATIO}")
    print("  case                      seed   bin   freq Hz        peak       floor   peak / floor  votes  found")
    for name, build in cases:
        for seed in range(args.seeds):
            wave = build(seed)
            records, _, mean, blocks = am.aspec_model(wave, index, first)
            v = am.notch_model(mean[0], int(blocks[0]), records)
            ratio = v["peak"] / v["floor"] if v["floor"] > 0 else float("inf")
            result["cases"].append(dict(case=name, seed=seed, peak_over_floor=ratio, **v))
            print(f"  {name:24s}  {seed:4d}  {v['bin']:4d}  {v['freq_hz']:8.2f}  {v['peak']:10.4g}  {v['floor']:10.4g}   {ratio:12.2f}  {v['votes']:5d}  {v['found']:5d}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
