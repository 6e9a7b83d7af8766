#!/usr/bin/env python3
"""What the ELT detector stage costs beside the demodulator call it follows and the SELCAL stage's call.  Needs
a GPU.

At 64 x 32 = 2048 rows x 16 batches (the benchmark's config4: 64 streams of 32 mixed channels) the demodulator runs its steady-state
call over a generated capture, and mi_elt_process_device runs over an audio plane of the same shape, at its defaults, on two kinds of
content: the 3 Hz beacon of tests/elt_model.py over white noise of deviation 0.03 on every row (no block is closed: the bank's full
cost, rows that raise alarms), and the same plane with fifteen rows in sixteen zeroed (closed channels: their blocks write 25 silent
records and skip the sums).  Beside it, in the same run and on the same planes, mi_selcal_process_device at its defaults.  HIP events
over --reps repetitions after --warmup warm-up ones give the time of each call, taken --takes times: the median and the spread (lowest
.. highest) are printed; mi_elt_last_launch_ms and mi_selcal_last_launch_ms say where each stage's time sits (bank, walk, scan, store,
tails).  The stages' state carries from one repetition to the next as in a replay.  Prints one table and one JSON line; --out writes
the line to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

from rate_common import WAVE_BATCH, load_package, timed as timed_on

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

SAMPLE_RATE, AGC_EXTRA = 2560000, 100
NSTREAMS, FFT_LOG, NB = 64, 9, 16
SIGMA = 0.03


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--takes", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from elt_model import beacon
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("elt_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def timed(fn):
        return sorted(timed_on(torch, stream, fn, args.warmup, args.reps) for _ in range(args.takes))

    def mid(ms):
        return float(np.median(ms))

    result = dict(tool="elt_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, warmup=args.warmup, takes=args.takes, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.takes} takes of {args.reps} repetitions after {args.warmup}")
    centre, chans = pkg.config3_channels()
    rows, nsteps, hop = NSTREAMS * len(chans), NB * WAVE_BATCH, 2 * (SAMPLE_RATE // 16000)
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=FFT_LOG)
    nbytes = ((nsteps + AGC_EXTRA) * hop + 2 * (1 << FFT_LOG) + 255) // 256 * 256
    gcfg = pkg.iqgen_cfg(sample_rate=SAMPLE_RATE, gate_samples=SAMPLE_RATE, carriers=pkg.carriers_for(centre, chans, amp_q8=1024))
    d_iq = torch.empty((NSTREAMS, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(gcfg, 0, NSTREAMS, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    wo = torch.empty((rows, nsteps), dtype=torch.float32, device="cuda")
    ax = torch.empty((rows, NB), dtype=torch.uint8, device="cuda")
    demod = pkg.Demod(dev, chans, nstreams=NSTREAMS, max_batches=NB)
    demod.process_device(d_iq.data_ptr(), nbytes, NB, wo.data_ptr(), ax.data_ptr(), hip_stream=s)  # (the first call takes AGC_EXTRA more windows)
    base = d_iq.data_ptr() + AGC_EXTRA * hop

    def run_demod():
        demod.process_device(base, nbytes, NB, wo.data_ptr(), ax.data_ptr(), hip_stream=s)

    demod_ms = timed(run_demod)
    stream.synchronize()
    demod.close()
    del d_iq, wo
    result["demod_ms"] = demod_ms
    tone = torch.from_numpy(beacon(nsteps, amp=0.1).astype(np.float32)).cuda()
    sounding = ((torch.randn((rows, nsteps), dtype=torch.float32, device="cuda") * SIGMA) + tone[None, :]).clamp_(-1.0, 1.0).contiguous()
    sparse = sounding.clone()
    sparse[torch.arange(rows, device="cuda") % 16 != 0] = 0.0
    print(f"  demodulator, {rows} rows x {NB} batches: median {mid(demod_ms):.4f} ms ({demod_ms[0]:.4f} .. {demod_ms[-1]:.4f})")
    print("  plane                 stage    ms median (lowest .. highest)      (bank / walk / scan / store / tails)          records   / demod   us / block")
    for name, plane in (("all rows sounding", sounding), ("1 row in 16 sounding", sparse)):
        case = dict(plane=name, rows=rows, batches=NB, sigma=SIGMA)
        for stage in ("elt", "selcal"):
            h = pkg.Elt(np.ones(rows), max_batches=NB) if stage == "elt" else pkg.Selcal(np.ones(rows), max_batches=NB)
            out = torch.empty(((h.max_events if stage == "elt" else h.max_codes) * 32,), dtype=torch.uint8, device="cuda")
            first = torch.empty((rows + 1,), dtype=torch.int32, device="cuda")
            count = torch.empty((2,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def run():
                h.process_device(plane.data_ptr(), nsteps, NB, out.data_ptr(), first.data_ptr(), count.data_ptr(), hip_stream=s)

            ms = timed(run)
            h.set_timing(True)
            parts, nrec = np.zeros(5), 0
            for _ in range(args.reps):
                run()
                parts += h.last_launch_ms()
                nrec += int(h.download(s)[3][0])
            parts /= args.reps
            h.close()
            over_demod, us_block = mid(ms) / mid(demod_ms), 1000.0 * mid(ms) / (rows * NB)
            case[stage] = dict(ms=ms, bank_ms=parts[0], walk_ms=parts[1], scan_ms=parts[2], store_ms=parts[3], tails_ms=parts[4], records_per_call=nrec / args.reps,
                               over_demod=over_demod, us_per_block=us_block)
            print(f"  {name:20s}  {stage:7s}  {mid(ms):.4f} ({ms[0]:.4f} .. {ms[-1]:.4f})   ({' / '.join(f'{p:.4f}' for p in parts)})   {nrec / args.reps:7.1f}   "
                  f"{over_demod:7.3f}   {us_block:10.3f}")
        case["elt_bank_over_selcal_bank"] = case["elt"]["bank_ms"] / case["selcal"]["bank_ms"]
        print(f"  {name:20s}  ELT bank / SELCAL bank = {case['elt_bank_over_selcal_bank']:.3f} (dependent steps per block: 13 x 256 / 2000 = 1.66)")
        result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
