#!/usr/bin/env python3
"""What the packet stage decodes and what it does not, on synthetic audio, through the host twin and the host oracle (no GPU).

1. Tilt: a carrier frequency-modulated at one deviation by a 1200 Hz and then a 2200 Hz tone, through the oracle's NFM demodulator:
   the power ratio of the two tones in the audio.  It is the default of gain[2]; gain[1] is its square root.
2. Sensitivity: 20 seeded short frames (random start) per level of tone power over full-band white noise, flat and with the space
   tone down by the tilt: the share decoded per slicer alone (the other two gains pushed out of reach) and by the three together.
3. False frames on 10 minutes of white noise and of voice-like audio, with strict and without.
4. Clock offset: the largest of 0, 50, 100 .. 1000 ppm at which the short and the longest frame decode at all four start times,
   fast and slow.
DESIGN.md 5r quotes this output.

    python3 tools/ax25_classes.py
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import ax25_model as m  # noqa: E402

pkg = load_package()
AMP = 0.3
OFF = 1e30  # a gain no bit reaches: the slicer says space always and decodes nothing


def decode(rows, cfg=None):
    """frames per row of float32 [rows][n]"""
    plane = np.asarray(rows, np.float32)
    frames, _, first, _, _ = pkg.ax25_plan_host(np.ones(len(plane)), plane, cfg)
    return [frames[first[r]:first[r + 1]] for r in range(len(plane))]


def is_sent(frames, f):
    return any(bytes(x["bytes"][:x["nbytes"]]) == bytes(f) for x in frames)


def tilt():
    from common import AGC_EXTRA, oracle_run
    rate, centre, nb = 2560000, 144000000, 6
    dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9)
    chans = [pkg.channel_cfg(centre + 25000, modulation=pkg.MOD_NFM)]
    hop = rate // 16000
    n_audio = nb * m.WAVE_BATCH + AGC_EXTRA + 8
    t = np.arange(n_audio * hop) / rate
    half = t.size // 2
    audio = np.where(np.arange(t.size) < half, np.sin(2 * np.pi * 1200.0 * t), np.sin(2 * np.pi * 2200.0 * t))
    dphi = 2.0 * np.pi * (25000.0 + 3000.0 * audio) / rate
    z = 30.0 * np.exp(1j * np.cumsum(dphi)).astype(np.complex64)
    iq = np.empty(2 * t.size, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    iq += np.random.default_rng(73).normal(0.0, 1.5, iq.size).astype(np.float32)
    iq = np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8)
    got, wo, _, _ = oracle_run(dev, chans, iq, nb)
    assert got == nb
    x = np.asarray(wo[0, :nb * m.WAVE_BATCH], np.float64)
    ts = np.arange(x.size) / 16000.0
    n = x.size
    seg = {1200.0: slice(n // 8, 3 * n // 8), 2200.0: slice(5 * n // 8, 7 * n // 8)}  # 4000 samples each: whole cycles of both tones
    power = {f: abs(np.sum(x[s] * np.exp(-2j * np.pi * f * ts[s])) / (s.stop - s.start)) ** 2 for f, s in seg.items()}
    ratio = power[1200.0] / power[2200.0]
    print(f"  power at 1200 Hz over power at 2200 Hz behind the NFM path: {ratio:.4f} ({10 * math.log10(ratio):+.2f} dB); its root {math.sqrt(ratio):.4f}")
    return dict(power_ratio=ratio, db=10 * math.log10(ratio))


def sensitivity():
    n = 8 * m.WAVE_BATCH
    f = m.ui_frame(**m.SHORT)
    d = pkg.ax25_settings()
    cfgs = {"slicer 0": (d.gain[0], OFF, OFF), "slicer 1": (OFF, d.gain[1], OFF), "slicer 2": (OFF, OFF, d.gain[2]), "all three": None}
    out = {}
    for what, sg in (("flat", 1.0), ("space down by the tilt", 1.0 / math.sqrt(d.gain[2]))):
        for db in range(4, 26, 2):
            sigma = AMP / math.sqrt(2.0) / 10 ** (db / 20.0)
            rows = []
            for seed in range(20):
                start = 3000 + int(np.random.default_rng(seed).integers(0, 9000))
                rows.append(m.modulate(m.burst_bits([f]), start, n, amp=AMP, space_gain=sg, noise=sigma, seed=1000 * db + seed))
            res = {k: sum(is_sent(r, f) for r in decode(rows, pkg.ax25_cfg(gain=g))) / 20 for k, g in cfgs.items()}
            out[f"{what}, {db} dB"] = res
            print(f"  {what}, {db:2d} dB: " + ", ".join(f"{k} {v:.2f}" for k, v in res.items()))
    return out


def false_frames():
    n = 4800 * m.WAVE_BATCH
    out = {}
    for what, x in (("noise", np.random.default_rng(11).normal(0, 0.1, n)), ("voice", m.voice_like(n, 12))):
        for strict in (True, False):
            out[f"{what}, strict {int(strict)}"] = len(decode([x], pkg.ax25_cfg(strict=strict))[0])
            print(f"  10 minutes of {what}, strict {int(strict)}: {out[f'{what}, strict {int(strict)}']} frames")
    return out


def clock_offset():
    out = {}
    for what, kw in (("short", m.SHORT), ("longest", m.LONGEST)):
        f = m.ui_frame(**kw)
        n = 24 * m.WAVE_BATCH
        for sign in (1.0, -1.0):
            best = None
            for ppm in range(0, 1050, 50):
                rows = [m.modulate(m.burst_bits([f]), 3000 + 197 * i, n, amp=AMP, ppm=sign * ppm) for i in range(4)]
                if all(is_sent(r, f) for r in decode(rows)):
                    best = ppm
                else:
                    break
            out[f"{what}, {'fast' if sign > 0 else 'slow'}"] = best
            print(f"  the {what} frame, clock {'fast' if sign > 0 else 'slow'}: decodes at all four start times up to {best} ppm")
    return out


def main():
    result = dict(tool="ax25_classes")
    print("tilt")
    result["tilt"] = tilt()
    if "--tilt" not in sys.argv:
        print("sensitivity")
        result["sensitivity"] = sensitivity()
        print("false frames")
        result["false"] = false_frames()
        print("clock offset")
        result["clock"] = clock_offset()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
