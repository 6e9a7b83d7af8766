#!/usr/bin/env python3
"""What the SELCAL stage's four thresholds separate, on synthetic audio, through the host twin (no GPU).

Classes: codes in white noise at falling SNR; twist (one tone of a pulse weaker than the other) up to what the voice band stage with a
300 Hz edge does to tone A; voice-like audio; CTCSS plus voice; a 1 kHz tone; square waves.  For each it prints how many windows named
a pair, the longest run of one pair, the codes decoded, and the three ratios the thresholds cut (tonality = (p1 + p2) / (c E),
twist = p1 / p2, separation = p2 / p3) so that the margins of the defaults can be read off.  DESIGN.md 5n quotes this output.

    python3 tools/selcal_classes.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import selcal_model as m  # noqa: E402

pkg = load_package()
HZ = m.table(m.MODE_16)[0].astype(np.float64)
C = float(pkg.selcal_settings()[1])


def run(x, cfg=None):
    codes, win, _, _, _ = pkg.selcal_plan_host([1], np.asarray(x, np.float32)[None, :], cfg)
    return codes, win[0]


def ratios(win):
    live = win[win["energy"] >= 1e-3]
    if not len(live):
        return dict(tonality=0.0, twist=0.0, separation=0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(tonality=float(np.max((live["p_best"] + live["p_second"]) / (C * live["energy"]))),
                    twist=float(np.min(live["p_best"] / live["p_second"])), separation=float(np.max(live["p_second"] / live["p_third"])))


def longest_run(pairs):
    best = cur = 0
    last = 0
    for p in pairs:
        cur = cur + 1 if p and p == last else (1 if p else 0)
        last, best = p, max(best, cur)
    return best


def describe(name, x):
    codes, win = run(x)
    r = ratios(win)
    print(f"{name:44s} windows {len(win):4d} named {int((win['pair'] != 0).sum()):4d} longest run {longest_run(win['pair']):3d} codes {len(codes)}  "
          f"max tonality {r['tonality']:.3f}  min twist {r['twist']:.2f}  max separation {r['separation']:.1f}")


def main():
    n = m.NB * m.WAVE_BATCH
    print(f"c = {C:.3f}; defaults {m.DEFAULTS}")
    print("-- codes in white noise: SNR = both tones' power over the noise's, full band (8 kHz); 16 codes per step")
    pairs = [((a, (a + 5) % 16), ((a + 2) % 16, (a + 9) % 16)) for a in range(16)]
    for snr in (20, 12, 6, 3, 2, 1, 0, -1, -2, -3):
        sigma = math.sqrt(0.25 ** 2 / 10 ** (snr / 10))
        ok = 0
        for k, (p1, p2) in enumerate(pairs):
            p1, p2 = tuple(sorted(p1)), tuple(sorted(p2))
            codes, _ = run(m.code_row(p1, p2, HZ, seed=100 + k) + m.noise(n, sigma, 200 + k))
            ok += len(codes) == 1 and tuple(codes[0]["tone"]) == (*p1, *p2)
        print(f"   SNR {snr:3d} dB: {ok:2d} / 16 decoded")
    print("-- twist: tone A of the first pulse lowered against tone K")
    for db in (0, 3, 6, 8, 9, 10, 12):
        codes, win = run(m.code_row((0, 9), (3, 8), HZ, seed=51, amp2=0.25 * 10 ** (-db / 20)))
        mid = win[8]
        print(f"   {db:2d} dB: codes {len(codes)}  p1 / p2 in mid-pulse {mid['p_best'] / mid['p_second']:.2f}")
    x = m.code_row((0, 9), (3, 8), HZ, seed=51).astype(np.float32)[None, :]
    y = pkg.vband_plan_host([1], x, rows_cfg=[(300, 3400)])[0]
    codes, win = run(y[0])
    mid = win[10]
    print(f"   through the voice band stage (300, 3400): codes {len(codes)}  p1 / p2 in mid-pulse {mid['p_best'] / mid['p_second']:.2f} "
          f"({10 * math.log10(mid['p_best'] / mid['p_second']):.1f} dB)")
    print("-- what must not decode (60 s each where seeded)")
    long_n = 60 * m.RATE
    t = np.arange(long_n) / m.RATE
    voice = np.concatenate([m.voice_like(n, 300 + k) for k in range(long_n // n)])
    describe("voice-like", voice)
    describe("CTCSS 100.0 Hz plus voice", voice + 0.1 * np.sin(2 * np.pi * 100.0 * t))
    describe("white noise, sigma 0.2", m.noise(long_n, 0.2, 400))
    describe("a 1 kHz tone", 0.5 * np.sin(2 * np.pi * 1000.0 * t[:n]))
    describe("tone M alone (977.2 Hz)", 0.5 * np.sin(2 * np.pi * 977.2 * t[:n]))
    describe("a square wave, 400 Hz, full scale", m.square(n, 400.0))
    describe("a square wave, 1 kHz, full scale", m.square(n, 1000.0))
    describe("a square wave at tone A (312.6 Hz)", m.square(n, 312.6))


if __name__ == "__main__":
    main()
