#!/usr/bin/env python3
"""What the SAME decoder stage costs beside the demodulator call it follows and beside the ACARS stage.
Needs a GPU.

At 64 x 32 = 2048 rows x 16 batches (the benchmark's config4: 64 streams of 32 mixed channels) the demodulator runs its steady-state
call over a generated capture, and mi_same_process_device runs over an audio plane of the same shape, at its defaults, on three
kinds of content: white Gaussian noise of deviation 0.03 on every row (no block is silent: the bank's full cost, every row idle),
the same plane with three rows in four zeroed (closed channels: their blocks are silent and skip the sums), and a plane whose rows
repeat one header burst (rows that walk a burst through the call).  Beside it on the noise plane, in the same job:
mi_acars_process_device at its defaults, as tools/acars_rate.py times it.  HIP events over --reps repetitions after --warmup warm-up
ones give the time of each call, taken twice to show the spread; mi_same_last_launch_ms says where the stage's time sits (bits, walk,
scan, store, tails).  The stage's state carries from one repetition to the next as in a replay.  Prints one table and one JSON line;
--out writes the line to a file.  Whether the bank is bound by LDS or by issue is not measured here: that takes a counter run of its
own.
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
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    import same_model as m
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("same_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="same_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, warmup=args.warmup, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.reps} repetitions after {args.warmup}")
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

    demod_ms = [timed(run_demod), timed(run_demod)]  # (twice: the spread of the same measurement)
    stream.synchronize()
    demod.close()
    del d_iq, wo
    noise = (torch.randn((rows, nsteps), dtype=torch.float32, device="cuda") * SIGMA).clamp_(-1.0, 1.0).contiguous()
    quarter = noise.clone()
    quarter[torch.arange(rows, device="cuda") % 4 != 0] = 0.0
    burst = m.modulate(nsteps, m.train([m.HEADER_TEXT], start=25 * 1500 + 7)[0])
    bursts_plane = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(burst, (rows, nsteps)))).cuda()
    print(f"  demodulator, {rows} rows x {NB} batches: {demod_ms[0]:.4f} {demod_ms[1]:.4f} ms")
    print("  plane                 same ms           (bits / walk / scan / store / tails)              messages   same / demod   us / block")
    for name, plane in (("noise", noise), ("noise, 3 of 4 closed", quarter), ("a burst on every row", bursts_plane)):
        sa = pkg.Same(np.ones(rows), max_batches=NB)
        recs = torch.empty((sa.max_messages * 304,), dtype=torch.uint8, device="cuda")
        first = torch.empty((rows + 1,), dtype=torch.int32, device="cuda")
        count = torch.empty((2,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def run_same():
            sa.process_device(plane.data_ptr(), nsteps, NB, recs.data_ptr(), first.data_ptr(), count.data_ptr(), hip_stream=s)

        ms = [timed(run_same), timed(run_same)]
        sa.set_timing(True)
        parts, nmsgs = np.zeros(5), 0
        for _ in range(args.reps):
            run_same()
            parts += sa.last_launch_ms()
            nmsgs += int(sa.download(s)[2][0])
        parts /= args.reps
        sa.close()
        over_demod, us_block = min(ms) / min(demod_ms), 1000.0 * min(ms) / (rows * NB)
        result["cases"].append(dict(plane=name, rows=rows, batches=NB, demod_ms=demod_ms, sigma=SIGMA, same_ms=ms, bits_ms=parts[0], walk_ms=parts[1],
                                    scan_ms=parts[2], store_ms=parts[3], tails_ms=parts[4], messages_per_call=nmsgs / args.reps, same_over_demod=over_demod,
                                    us_per_block=us_block))
        print(f"  {name:20s}  {ms[0]:.4f} {ms[1]:.4f}   ({' / '.join(f'{p:.4f}' for p in parts)})   {nmsgs / args.reps:7.1f}   {over_demod:14.3f}   {us_block:10.3f}")
    ac = pkg.Acars(np.ones(rows), max_batches=NB)
    frames = torch.empty((ac.max_frames * 272,), dtype=torch.uint8, device="cuda")
    first = torch.empty((rows + 1,), dtype=torch.int32, device="cuda")
    count = torch.empty((2,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def run_acars():
        ac.process_device(noise.data_ptr(), nsteps, NB, frames.data_ptr(), first.data_ptr(), count.data_ptr(), hip_stream=s)

    acars_ms = [timed(run_acars), timed(run_acars)]
    ac.set_timing(True)
    parts = np.zeros(5)
    for _ in range(args.reps):
        run_acars()
        parts += ac.last_launch_ms()
    ac.close()
    result["acars_ms"], result["acars_parts_ms"] = acars_ms, list(parts / args.reps)
    print(f"  ACARS stage on the noise plane: {acars_ms[0]:.4f} {acars_ms[1]:.4f} ms   ({' / '.join(f'{p:.4f}' for p in parts / args.reps)})")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
