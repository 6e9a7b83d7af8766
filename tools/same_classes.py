#!/usr/bin/env python3
"""What the SAME stage decodes and what it does not, on synthetic audio, through the host twin (no GPU).

1. Sensitivity: 10 seeded alerts (three header bursts, random start) per level of tone power over full-band white noise, 6 .. 30 dB
   in steps of 2: the share whose voted message is the header sent, and the share of single bursts (the same audio cut behind the
   first burst) whose unvoted message is.
2. False messages on 10 minutes of white noise and of voice-like audio: messages closed, and those with fields_ok.
3. Clock offset: whether the longest header decodes at +-200 ppm with the timing moves and with hold_timing, at four start times.
4. With --capture (needs a GPU): the mark / space level ratio in the audio the NFM demodulator returns for the capture of
   tests/test_gpu_same.py, whose modulator sends both tones at one level.
DESIGN.md 5p quotes this output.

    python3 tools/same_classes.py
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import same_model as m  # noqa: E402

pkg = load_package()
AMP = 0.3


def decode(rows, cfg=None):
    """messages per row of float32 [rows][n]"""
    plane = np.asarray(rows, np.float32)
    msgs, _, _, first, _, _ = pkg.same_plan_host(np.ones(len(plane)), plane, cfg)
    return [msgs[first[r]:first[r + 1]] for r in range(len(plane))]


def is_sent(msgs, text):
    return any(bytes(x["bytes"][:x["nbytes"]]) == text for x in msgs)


def sensitivity():
    n = 64 * m.WAVE_BATCH
    out = {}
    for db in range(6, 32, 2):
        sigma = AMP / math.sqrt(2.0) / 10 ** (db / 20.0)
        three, one = [], []
        for seed in range(10):
            start = 20000 + int(np.random.default_rng(seed).integers(0, 50000))
            bursts = m.train([m.HEADER_TEXT] * 3, start=start, amp=AMP)[0]
            x = m.modulate(n, bursts, noise=sigma, seed=1000 * db + seed)
            three.append(x)
            y = x.copy()
            y[(bursts[1][1] - m.GAP // 2) // 25:] = 0.0
            one.append(y)
        out[db] = dict(voted=sum(is_sent([x for x in r if x["voted"]], m.HEADER_TEXT) for r in decode(three)) / 10,
                       unvoted=sum(is_sent(r, m.HEADER_TEXT) for r in decode(one)) / 10)
        print(f"  {db:2d} dB: voted {out[db]['voted']:.1f}, one burst {out[db]['unvoted']:.1f}")
    return out


def false_messages():
    n = 4800 * m.WAVE_BATCH
    out = {}
    for what, x in (("noise", np.random.default_rng(11).normal(0, 0.1, n)), ("voice", m.voice_like(n, 12))):
        msgs = decode([x])[0]
        out[what] = dict(messages=len(msgs), fields_ok=int((msgs["fields_ok"] == 1).sum()))
        print(f"  10 minutes of {what}: {out[what]}")
    return out


def clock_offset():
    n = 64 * m.WAVE_BATCH
    out = {}
    for ppm in (200.0, -200.0):
        rows = [m.modulate(n, m.train([m.LONGEST], start=30000 + 197 * i, ppm=ppm, amp=AMP)[0]) for i in range(4)]
        for hold in (False, True):
            got = sum(is_sent(r, m.LONGEST) for r in decode(rows, pkg.same_cfg(hold_timing=hold)))
            out[f"{ppm:+.0f} ppm, hold_timing {int(hold)}"] = got
            print(f"  {ppm:+.0f} ppm, hold_timing {int(hold)}: {got} of 4 decode")
    return out


def capture():
    from test_gpu_same import e2e_setup
    dev, chans, iq, nb = e2e_setup(pkg)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=nb)
    wo = d.process([iq], nb)[0]
    d.close()
    x = np.asarray(wo[0][0, :nb * m.WAVE_BATCH], np.float64)
    t = np.arange(x.size) / 16000.0
    seg = slice(25 * 8000 // 25 + 200, 25 * 8000 // 25 + 200 + 14000)  # inside the first burst
    level = {f: abs(np.sum(x[seg] * np.exp(-2j * np.pi * f * t[seg]))) for f in (2083.3333, 1562.5)}
    # the header's bits are not half marks: count them
    bits = np.array(m.burst_bits(m.HEADER_TEXT))
    marks = bits.mean()
    ratio = (level[2083.3333] / marks) / (level[1562.5] / (1 - marks))
    print(f"  mark / space level behind the NFM demodulator: {ratio:.3f} ({20 * math.log10(ratio):+.2f} dB), marks {marks:.3f} of the bits")
    return dict(mark_over_space=ratio)


def main():
    result = dict(tool="same_classes")
    print("sensitivity")
    result["sensitivity"] = sensitivity()
    print("false messages")
    result["false"] = false_messages()
    print("clock offset")
    result["clock"] = clock_offset()
    if "--capture" in sys.argv:
        print("capture")
        result["capture"] = capture()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
