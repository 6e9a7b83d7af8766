#!/usr/bin/env python3
"""What the ACARS stage decodes and what it does not, on synthetic audio, through the host twin (no GPU).

1. Sensitivity: 20 seeded frames (20 characters of text, random start) per level of tone power over full-band white noise, in steps
   of 1 dB: frames decoded per level, and the lowest level at which 20 of 20 decode.
2. False syncs and frames on 10 minutes of white noise and of voice-like audio, for sync_errors 0 .. 4: slots at which some
   hypothesis hits (counted on every slot, idle or not, from the twin's change bits), frames under keep_bad, and frames whose checksum
   holds.
3. Clock offset: the largest offset in ppm, in steps of 10, up to which the longest frame decodes at four start times and both signs,
   with the timing moves and with hold_timing.
DESIGN.md 5o quotes this output; tests/acars_model.py takes MIN_SNR_DB and TRACK_LIMIT_PPM from it.

    python3 tools/acars_classes.py
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import acars_model as m  # noqa: E402

pkg = load_package()
AMP = 0.3


def decode(rows, cfg=None):
    """frames per row of float32 [rows][n]"""
    plane = np.asarray(rows, np.float32)
    frames, _, _, first, _, _ = pkg.acars_plan_host(np.ones(len(plane)), plane, cfg)
    return [frames[first[r]:first[r + 1]] for r in range(len(plane))]


def sensitivity():
    n = 4 * m.WAVE_BATCH
    out = {}
    for snr in range(20, -1, -1):
        sigma = math.sqrt(AMP ** 2 / 2 / 10 ** (snr / 10))
        rows, sent = [], []
        for k in range(20):
            rng = np.random.default_rng(1000 + k)
            f = dict(mode="2", address=".N123AB", ack="\x15", label="H1", block_id="3", text=m.random_text(rng, 20), end=m.ETX)
            rows.append(m.modulate(m.burst_bits([m.frame_bytes(**f)]), 600 + rng.uniform(0, 600), n, amp=AMP) + m.noise(n, sigma, 2000 + 100 * snr + k))
            sent.append(f["text"])
        got = decode(rows)
        out[snr] = sum(1 for g, t in zip(got, sent) if len(g) == 1 and m.frame_fields(g[0])["text"] == t)
    return out, min(snr for snr, k in out.items() if k == 20)


def sync_hits(bits):
    """slots at which some hypothesis is within 0 .. 4 mismatches of the pattern: bits uint32 [nb][20][10] of one row"""
    nb = bits.shape[0]
    c = ((bits[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(nb, m.NTAU, 320)[..., :m.NBITS]
    stream = np.transpose(c, (1, 0, 2)).reshape(m.NTAU, -1).astype(np.float64) * 2 - 1
    pat = m.sync_pattern().astype(np.float64) * 2 - 1
    mism = np.stack([(m.SYNC_BITS - np.correlate(s, pat, "valid")) / 2 for s in stream]).min(0)
    return [int((mism <= e).sum()) for e in range(5)]


def false_alarms(minutes=10):
    nb = minutes * 60 * 8
    n = nb * m.WAVE_BATCH
    out = {}
    for name, x in (("white noise", m.noise(n, 0.2, 3000)), ("voice-like", m.voice_like(n, 3001))):
        plane = np.asarray(x, np.float32)[None, :]
        hits = None
        per = {}
        for e in range(5):
            frames, bits, _, _, _, _ = pkg.acars_plan_host([1], plane, pkg.acars_cfg(sync_errors=e or pkg.ACARS_SYNC_EXACT, keep_bad=True))
            if hits is None:
                hits = sync_hits(bits[0])
            per[e] = dict(sync_hits_per_min=hits[e] / minutes, frames_kept_bad_per_min=len(frames) / minutes,
                          crc_valid_frames=int(frames["crc_ok"].sum()))
        out[name] = per
    return out


def clock_limit(hold):
    cfg = pkg.acars_cfg(hold_timing=hold)
    n = 9 * m.WAVE_BATCH
    f = dict(mode="2", address=".N123AB", ack="\x15", label="H1", block_id="3", text=m.LONG_TEXT, end=m.ETX)
    bits = m.burst_bits([m.frame_bytes(**f)])
    limit = 0
    for ppm in range(0, 1001, 10):
        rows = [m.modulate(bits, 900 + s, n, amp=AMP, ppm=sign * ppm) for s in (0, 3.5, 7, 13) for sign in (1, -1)]
        if not all(len(g) == 1 and m.frame_fields(g[0])["text"] == m.frame_fields(dict(bytes=np.array(m.frame_bytes(**f)), nbytes=240))["text"] for g in decode(rows, cfg)):
            break
        limit = ppm
    return limit


def main():
    levels, floor = sensitivity()
    res = dict(decoded_of_20_by_snr_db=levels, lowest_level_20_of_20_db=floor, false=false_alarms(),
               clock_limit_ppm=dict(tracking=clock_limit(False), hold_timing=clock_limit(True)))
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
