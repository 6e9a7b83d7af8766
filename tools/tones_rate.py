#!/usr/bin/env python3
"""What the CTCSS tone finder costs beside the demodulator call it follows.  Needs a GPU.

For each row count (8 NFM channels x 1, 32 and 256 streams by default) a generated capture goes through one mi_demod_process_device
call of --batches batches; mi_tones_process_device then runs over the audio and flags that call wrote, and once more with every flag
open (the most work the finder can have).  HIP events over --reps repetitions after --warmup warm-up ones give the time of either
call; mi_tones_last_launch_ms says where the finder's time sits (walk, scan, bank).  The finder's state carries from one repetition to
the next as in a replay.  Prints one table and one JSON line.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, load_package, timed as timed_on

AGC_EXTRA = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("tones_rate.py needs a GPU")
    nb, window = args.batches, args.window or 6400
    centre, am = pkg.config2_channels()
    chans = [pkg.channel_cfg(c.freq, modulation=pkg.MOD_NFM, bandwidth=12500) for c in am]
    nch = len(chans)
    dev = pkg.device_cfg(centerfreq=centre)
    # carriers with and without the 100 Hz tone, off and on every 8 batches in two phases
    carriers = [(c.freq - centre, 2 if k % 2 == 0 else 1, 3072, k // 2 % 2) for k, c in enumerate(chans)]
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate, carriers=carriers)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="tones_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, batches=nb, window=window, reps=args.reps, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {nb} batches, window {window}, {args.reps} repetitions")
    print("   rows  flags     records   tones ms   (walk / scan / bank)            demod ms    tones / demod")
    for nstreams in args.streams:
        rows = nstreams * nch
        d = pkg.Demod(dev, chans, nstreams=nstreams, max_batches=nb)
        nbytes = (d.bytes_needed(nb) + 255) // 256 * 256
        d_iq = torch.zeros((nstreams, nbytes), dtype=torch.uint8, device="cuda")
        pkg.iqgen_device(cfg, 0, nstreams, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
        wave = torch.zeros((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
        axc = torch.zeros((rows, nb), dtype=torch.uint8, device="cuda")
        most = rows * pkg.tones_max_windows(window, nb)
        records = torch.empty((most * 40,), dtype=torch.uint8, device="cuda")
        powers = torch.empty((most, 64), dtype=torch.float32, device="cuda")
        row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
        count = torch.empty(2, dtype=torch.int32, device="cuda")
        state = d.get_state()

        def demod():  # (every repetition from the same state, so that each does the same work)
            d.process_device(d_iq.data_ptr(), nbytes, nb, wave.data_ptr(), axc.data_ptr(), hip_stream=s)

        demod()
        torch.cuda.synchronize()
        demod_ms = []
        for _ in range(2):
            d.set_state(state)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record()
                demod()
                b.record()
            b.synchronize()
            demod_ms.append(a.elapsed_time(b))
        open_share = float((axc != ord(" ")).float().mean().item())
        all_open = torch.full_like(axc, ord("*"))
        for name, flags in (("demod's", axc), ("all open", all_open)):
            tn = pkg.Tones(np.ones(rows), max_batches=nb, window=window)
            torch.cuda.synchronize()

            def tones():
                tn.process_device(wave.data_ptr(), nb * WAVE_BATCH, flags.data_ptr(), nb, nb, records.data_ptr(), row_first.data_ptr(), count.data_ptr(),
                                  d_powers=powers.data_ptr(), hip_stream=s)

            tones_ms = [timed(tones), timed(tones)]  # (twice: the spread of the same measurement)
            tn.set_timing(True)
            parts = np.zeros(3)
            for _ in range(args.reps):
                tones()
                parts += tn.last_launch_ms()
            parts /= args.reps
            nrec = int(tn.download(s)[3][0])
            tn.close()
            share = min(tones_ms) / min(demod_ms)
            result["cases"].append(dict(rows=rows, streams=nstreams, flags=name, open_share=open_share if flags is axc else 1.0, records=nrec,
                                        tones_ms=tones_ms, walk_ms=parts[0], scan_ms=parts[1], bank_ms=parts[2], demod_ms=demod_ms,
                                        tones_over_demod=share))
            print(f"  {rows:5d}  {name:8s}  {nrec:7d}   {tones_ms[0]:.4f} {tones_ms[1]:.4f}   ({parts[0]:.4f} / {parts[1]:.4f} / {parts[2]:.4f})   "
                  f"{demod_ms[0]:.3f} {demod_ms[1]:.3f}   {share:7.4f}")
        d.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
