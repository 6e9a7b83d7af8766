#!/usr/bin/env python3
"""What the voice band stage costs beside the demodulator call it follows.  Needs a GPU.

For each shape -- 8 rows x 64 batches (the benchmark's config2: one stream of 8 AM channels), 32 rows x 64 batches (config3: one
stream of 32 mixed channels) and 64 x 32 rows x 16 batches (config4: 64 such streams) -- the demodulator runs its steady-state call
over a generated capture, and mi_vband_process_device runs over an audio plane of the same shape at duty cycles 0, 0.5 and 1: the
share of (row, batch) blocks that hold audio (uniform noise of +-0.9; open runs of 6 batches on average), the others digital silence
as a closed channel leaves it.  Rows take the default settings (100, 2500), or with --classes N one of N settings in turn.  HIP events
over --reps repetitions after --warmup warm-up ones give the time of either call; mi_vband_last_launch_ms says where the stage's time
sits (filter, tail copy).  The stage's state carries from one repetition to the next as in a replay.  Prints one table and one JSON
line; --out writes the line to a file.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, draw, load_package, timed as timed_on

SAMPLE_RATE, AGC_EXTRA = 2560000, 100
SHAPES = {"config2": (1, 9, 64), "config3": (1, 11, 64), "config4": (64, 9, 16)}  # streams, fft_size_log, batches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=list(SHAPES))
    ap.add_argument("--duty", type=float, nargs="+", default=[0.0, 0.5, 1.0])
    ap.add_argument("--classes", type=int, default=1)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("vband_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(1)

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="vband_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, classes=args.classes, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.reps} repetitions, {args.classes} class(es) of settings")
    print("  shape     rows  batches   demod ms   duty   open blocks   vband ms         (filter / tails)    vband / demod   us per open block")
    for shape in args.shapes:
        nstreams, fft_log, nb = SHAPES[shape]
        centre, chans = pkg.config2_channels() if shape == "config2" else pkg.config3_channels()
        rows, nsteps, hop = nstreams * len(chans), nb * WAVE_BATCH, 2 * (SAMPLE_RATE // 16000)
        dev = pkg.device_cfg(centerfreq=centre, fft_size_log=fft_log)
        nbytes = ((nsteps + AGC_EXTRA) * hop + 2 * (1 << fft_log) + 255) // 256 * 256
        amp = {} if shape == "config2" else {"amp_q8": 1024}
        gcfg = pkg.iqgen_cfg(sample_rate=SAMPLE_RATE, gate_samples=SAMPLE_RATE, carriers=pkg.carriers_for(centre, chans, **amp))
        d_iq = torch.empty((nstreams, nbytes), dtype=torch.uint8, device="cuda")
        pkg.iqgen_device(gcfg, 0, nstreams, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
        wo = torch.empty((rows, nsteps), dtype=torch.float32, device="cuda")
        ax = torch.empty((rows, nb), dtype=torch.uint8, device="cuda")
        demod = pkg.Demod(dev, chans, nstreams=nstreams, max_batches=nb)
        demod.process_device(d_iq.data_ptr(), nbytes, nb, wo.data_ptr(), ax.data_ptr(), hip_stream=s)  # (the first call takes AGC_EXTRA more windows)
        base = d_iq.data_ptr() + AGC_EXTRA * hop

        def run_demod():
            demod.process_device(base, nbytes, nb, wo.data_ptr(), ax.data_ptr(), hip_stream=s)

        demod_ms = [timed(run_demod), timed(run_demod)]  # (twice: the spread of the same measurement)
        stream.synchronize()
        demod.close()
        settings = [(100 + 50 * (r % args.classes), 2500 + 100 * (r % args.classes)) for r in range(rows)]
        out = torch.empty((rows, nsteps), dtype=torch.float32, device="cuda")
        for duty in args.duty:
            open_blocks = draw(rng, rows, nb, duty, burst=None if duty >= 1.0 or duty <= 0.0 else 6.0) == ord("*")
            noise = (torch.rand((rows, nb, WAVE_BATCH), dtype=torch.float32, device="cuda") * 2.0 - 1.0) * 0.9
            wave = (noise * torch.from_numpy(open_blocks).cuda()[:, :, None]).reshape(rows, nsteps).contiguous()
            vb = pkg.Vband(np.ones(rows), settings, max_batches=nb)
            torch.cuda.synchronize()

            def run_vband():
                vb.process_device(wave.data_ptr(), nsteps, nb, out.data_ptr(), nsteps, hip_stream=s)

            vband_ms = [timed(run_vband), timed(run_vband)]
            vb.set_timing(True)
            parts = np.zeros(2)
            for _ in range(args.reps):
                run_vband()
                parts += vb.last_launch_ms()
            parts /= args.reps
            vb.close()
            nopen = int(open_blocks.sum())
            share = min(vband_ms) / min(demod_ms)
            per_block = 1e3 * min(vband_ms) / nopen if nopen else 0.0
            result["cases"].append(dict(shape=shape, rows=rows, batches=nb, demod_ms=demod_ms, duty=duty, open_blocks=nopen, vband_ms=vband_ms,
                                        filter_ms=parts[0], tails_ms=parts[1], vband_over_demod=share, us_per_open_block=per_block))
            print(f"  {shape:8s} {rows:5d}  {nb:7d}   {min(demod_ms):8.4f}   {duty:4.2f}   {nopen:11d}   {vband_ms[0]:.4f} {vband_ms[1]:.4f}   "
                  f"({parts[0]:.4f} / {parts[1]:.4f})   {share:10.3f}   {per_block:14.3f}")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
