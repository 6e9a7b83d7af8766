#!/usr/bin/env python3
"""What the noise reduction stage costs beside the demodulator call it follows.  Needs a GPU.

For each shape -- 8 rows x 64 batches (the benchmark's config2: one stream of 8 AM channels) and 64 x 32 = 2048 rows x 16 batches
(config4: 64 streams of 32 mixed channels) -- the demodulator runs its steady-state call over a generated capture, and
mi_denoise_process_device runs over an audio plane of the same shape holding white Gaussian noise of deviation 0.03, at its default
row.  Beside it on the same plane: mi_vband_process_device at its default settings, and a plain device-to-device copy of the plane.
HIP events over --reps repetitions after --warmup warm-up ones give the time of each call, taken twice to show the spread;
mi_denoise_last_launch_ms says where the stage's time sits (floor, apply, tails).  The stage's state carries from one repetition to
the next as in a replay.  Prints one table and one JSON line; --out writes the line to a file.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, load_package, timed as timed_on

SAMPLE_RATE, AGC_EXTRA = 2560000, 100
SHAPES = {"config2": (1, 9, 64), "config4": (64, 9, 16)}  # streams, fft_size_log, batches
SIGMA = 0.03


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("denoise_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="denoise_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, warmup=args.warmup, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.reps} repetitions after {args.warmup}")
    print("  shape     rows  batches   demod ms   denoise ms       (floor / apply / tails)       copy ms          vband ms         denoise / demod   us / block")
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
        del d_iq
        out = torch.empty((rows, nsteps), dtype=torch.float32, device="cuda")
        wave = (torch.randn((rows, nsteps), dtype=torch.float32, device="cuda") * SIGMA).clamp_(-1.0, 1.0).contiguous()
        dn = pkg.Denoise(np.ones(rows), max_batches=nb)
        vb = pkg.Vband(np.ones(rows), max_batches=nb)
        torch.cuda.synchronize()

        def run_denoise():
            dn.process_device(wave.data_ptr(), nsteps, nb, out.data_ptr(), nsteps, hip_stream=s)

        def run_vband():
            vb.process_device(wave.data_ptr(), nsteps, nb, out.data_ptr(), nsteps, hip_stream=s)

        def run_copy():
            with torch.cuda.stream(stream):
                out.copy_(wave, non_blocking=True)

        denoise_ms = [timed(run_denoise), timed(run_denoise)]
        copy_ms = [timed(run_copy), timed(run_copy)]
        vband_ms = [timed(run_vband), timed(run_vband)]
        dn.set_timing(True)
        parts = np.zeros(3)
        for _ in range(args.reps):
            run_denoise()
            parts += dn.last_launch_ms()
        parts /= args.reps
        dn.close()
        vb.close()
        over_demod, us_block = min(denoise_ms) / min(demod_ms), 1000.0 * min(denoise_ms) / (rows * nb)
        result["cases"].append(dict(shape=shape, rows=rows, batches=nb, demod_ms=demod_ms, sigma=SIGMA, denoise_ms=denoise_ms, floor_ms=parts[0],
                                    apply_ms=parts[1], tails_ms=parts[2], copy_ms=copy_ms, vband_ms=vband_ms, denoise_over_demod=over_demod,
                                    us_per_block=us_block))
        print(f"  {shape:8s} {rows:5d}  {nb:7d}   {min(demod_ms):8.4f}   {denoise_ms[0]:.4f} {denoise_ms[1]:.4f}   ({parts[0]:.4f} / {parts[1]:.4f} / {parts[2]:.4f})   "
              f"{copy_ms[0]:.4f} {copy_ms[1]:.4f}   {vband_ms[0]:.4f} {vband_ms[1]:.4f}   {over_demod:15.3f}   {us_block:10.3f}")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
