#!/usr/bin/env python3
"""What the pager decoder stage's settings buy.  Needs no GPU: the host twin mi_pocsag_plan_host computes
what the device computes, byte for byte.

Three sweeps at one baud (--baud, default 1200), each over --trials seeded transmissions of the model's modulator (levels +-0.3, a
short preamble, one alphanumeric page of 21 words that crosses into a second group):
  - against the SNR (level power over full-band white noise), for correct none / 1 / 2: pages whose address came out, pages whose
    every word came out right, and WRONG words accepted as good (a stored word, not flagged bad, that is not the word sent);
  - against a DC offset, in units of the level, with the lanes of slicer 0 and of slicer 1: which slicer the sync chose and whether
    the page came out;
  - against the clock offset in ppm, with and without timing moves: the largest offset at which every trial's page comes out whole.
Prints the tables and one JSON line; --out writes the line to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

from rate_common import load_package

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baud", type=int, default=1200)
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import pocsag_model as m
    pkg = load_package()
    baud, L = args.baud, m.GEOM[args.baud][0]
    words = m.alpha_words(m.LONG_TEXT)
    bits = m.transmission([(0x1555D, 3, words)], preamble=64)
    nb = -(-(len(bits) * L + 40000) // m.TWELFTHS) + 1
    n = nb * m.WAVE_BATCH
    result = dict(tool="pocsag_classes", baud=baud, trials=args.trials, snr=[], dc=[], ppm=[])

    def run(x, **cfg):
        return pkg.pocsag_plan_host(np.ones(len(x)), np.asarray(x, np.float32), pkg.pocsag_cfg(baud=baud, **cfg))[0]

    print(f"{baud} baud, {args.trials} trials a point, a page of {len(words)} words")
    print("  SNR dB   correct   addressed   whole   wrong words accepted   words flagged bad")
    for snr in (20, 10, 4, 2, 0, -2, -4, -6, -8, -10):  # (a bit's sum of 13 samples gains 11 dB: the pages go between 0 and -8 dB)
        sigma = 0.3 / 10 ** (snr / 20.0)
        x = np.stack([m.render(bits, 5000 + 37 * t, n, baud, noise=sigma, seed=1000 * (snr + 20) + t) for t in range(args.trials)])
        for name, correct in (("none", pkg.POCSAG_CORRECT_NONE), ("1", 1), ("2", 2)):
            msgs = run(x, correct=correct)
            mine = msgs[msgs["address"] == 0x1555D]
            whole = sum(1 for r in mine if r["nwords"] == len(words) and r["nbad"] == 0 and list(r["words"][:len(words)]) == words)
            wrong = sum(1 for r in mine for i in range(min(int(r["nwords"]), len(words))) if not r["bad"][i // 32] >> (i % 32) & 1 and r["words"][i] != words[i])
            result["snr"].append(dict(snr_db=snr, correct=name, addressed=len(mine), whole=whole, wrong_words=wrong, bad_words=int(mine["nbad"].sum())))
            print(f"  {snr:6d}   {name:>7s}   {len(mine):9d}   {whole:5d}   {wrong:20d}   {int(mine['nbad'].sum()):17d}")
    print("  DC / level   pages   on slicer 1")
    for dc in (0.0, 0.25, 0.5, 0.9, 1.5, 3.0):
        x = np.stack([m.render(bits, 5000 + 37 * t, n, baud, dc=0.3 * dc, noise=0.03, seed=t) for t in range(args.trials)])
        msgs = run(x)
        mine = msgs[(msgs["address"] == 0x1555D) & (msgs["nbad"] == 0) & (msgs["nwords"] == len(words))]
        s1 = int((mine["lane_sync"] >= m.GEOM[baud][2]).sum())
        result["dc"].append(dict(dc_over_level=dc, pages=len(mine), on_slicer_1=s1))
        print(f"  {dc:10.2f}   {len(mine):5d}   {s1:11d}")
    print("  ppm     whole with moves   whole held")
    for ppm in (50, 100, 200, 400, 800, 1600, 3200):
        x = np.stack([m.render(bits, 5000 + 37 * t, n, baud, ppm=ppm * (1 if t % 2 else -1)) for t in range(args.trials)])
        got = []
        for hold in (False, True):
            msgs = run(x, hold_timing=hold)
            got.append(int(((msgs["address"] == 0x1555D) & (msgs["nbad"] == 0) & (msgs["nwords"] == len(words))).sum()))
        result["ppm"].append(dict(ppm=ppm, whole_moves=got[0], whole_held=got[1]))
        print(f"  {ppm:5d}   {got[0]:16d}   {got[1]:10d}")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
