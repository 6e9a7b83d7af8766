#!/usr/bin/env python3
"""What the packet decoder stage costs beside the demodulator call it follows and beside the ACARS and SAME stages (DESIGN.md
section 5r).  Needs a GPU.

At 64 x 32 = 2048 rows x 16 batches (the benchmark's config4: 64 streams of 32 mixed channels) the demodulator runs its steady-state
call over a generated capture, and mi_ax25_process_device runs over an audio plane of the same shape, at its defaults, on three
kinds of content: white Gaussian noise of deviation 0.03 on every row (no block is silent: the bank's full cost, every deframer at
work on random bits), the same plane with three rows in four zeroed (closed channels: their blocks are silent and skip the sums),
and a plane whose rows repeat one frame (30 lanes that collect its bytes and close it).  Beside it on the noise plane, in the same
job: mi_acars_process_device and mi_same_process_device at their defaults.  HIP events over --reps repetitions after --warmup warm-up
ones give the time of each call, taken twice to show the spread; mi_ax25_last_launch_ms says where the stage's time sits (bits, walk,
scan, store, tails), and the walk's time per slot (150 * 16 slots a call) stands beside the ACARS walk's per slot (300 * 16).  The
stage's state carries from one repetition to the next as in a replay.  Prints one table and one JSON line; --out writes the line to
a file.  Whether the bank is bound by LDS or by issue is not measured here: that takes a counter run of its own.
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
    import ax25_model as m
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("ax25_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="ax25_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, warmup=args.warmup, cases=[])
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
    burst = m.modulate(m.burst_bits([m.ui_frame(**m.SHORT)]), 3 * 1500 + 7, nsteps).astype(np.float32)
    bursts_plane = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(burst, (rows, nsteps)))).cuda()
    print(f"  demodulator, {rows} rows x {NB} batches: {demod_ms[0]:.4f} {demod_ms[1]:.4f} ms")
    print("  plane                 ax25 ms           (bits / walk / scan / store / tails)              frames   ax25 / demod   us / block   walk ns / slot")
    for name, plane in (("noise", noise), ("noise, 3 of 4 closed", quarter), ("a frame on every row", bursts_plane)):
        sa = pkg.Ax25(np.ones(rows), max_batches=NB)
        recs = torch.empty((sa.max_frames * 352,), dtype=torch.uint8, device="cuda")
        first = torch.empty((rows + 1,), dtype=torch.int32, device="cuda")
        count = torch.empty((2,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

        def run_ax25():
            sa.process_device(plane.data_ptr(), nsteps, NB, recs.data_ptr(), first.data_ptr(), count.data_ptr(), hip_stream=s)

        ms = [timed(run_ax25), timed(run_ax25)]
        sa.set_timing(True)
        parts, nmsgs = np.zeros(5), 0
        for _ in range(args.reps):
            run_ax25()
            parts += sa.last_launch_ms()
            nmsgs += int(sa.download(s)[2][0])
        parts /= args.reps
        sa.close()
        over_demod, us_block = min(ms) / min(demod_ms), 1000.0 * min(ms) / (rows * NB)
        ns_slot = 1e6 * parts[1] / (150 * NB)
        result["cases"].append(dict(plane=name, rows=rows, batches=NB, demod_ms=demod_ms, sigma=SIGMA, ax25_ms=ms, bits_ms=parts[0], walk_ms=parts[1],
                                    scan_ms=parts[2], store_ms=parts[3], tails_ms=parts[4], frames_per_call=nmsgs / args.reps, ax25_over_demod=over_demod,
                                    us_per_block=us_block, walk_ns_per_slot=ns_slot))
        print(f"  {name:20s}  {ms[0]:.4f} {ms[1]:.4f}   ({' / '.join(f'{p:.4f}' for p in parts)})   {nmsgs / args.reps:7.1f}   {over_demod:12.3f}   {us_block:10.3f}   {ns_slot:10.1f}")
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
    result["acars_walk_ns_per_slot"] = 1e6 * parts[1] / args.reps / (300 * NB)
    print(f"  ACARS stage on the noise plane: {acars_ms[0]:.4f} {acars_ms[1]:.4f} ms   ({' / '.join(f'{p:.4f}' for p in parts / args.reps)}), "
          f"walk {result['acars_walk_ns_per_slot']:.1f} ns / slot")
    sa = pkg.Same(np.ones(rows), max_batches=NB)
    recs = torch.empty((sa.max_messages * 304,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def run_same():
        sa.process_device(noise.data_ptr(), nsteps, NB, recs.data_ptr(), first.data_ptr(), count.data_ptr(), hip_stream=s)

    same_ms = [timed(run_same), timed(run_same)]
    sa.set_timing(True)
    parts = np.zeros(5)
    for _ in range(args.reps):
        run_same()
        parts += sa.last_launch_ms()
    sa.close()
    result["same_ms"], result["same_parts_ms"] = same_ms, list(parts / args.reps)
    print(f"  SAME stage on the noise plane: {same_ms[0]:.4f} {same_ms[1]:.4f} ms   ({' / '.join(f'{p:.4f}' for p in parts / args.reps)})")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
