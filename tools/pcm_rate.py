#!/usr/bin/env python3
"""What the PCM stage costs beside the output gate call it follows.  Needs a GPU.

For each geometry (rows x batches; 2048 x 16 is gate_rate.py's, 256 x 64 has tones_rate.py's batches) and open fraction, audio already
in HBM goes through mi_outgate_process_device (rule MI_GATE_OPEN_TRAIL on every row) and then, for each of the four rate x format
pairs, through mi_pcm_process_device on the index and counts the gate left on the device.  HIP events over --reps repetitions after
--warmup warm-up ones give the time of either call; mi_pcm_last_launch_ms says where the stage's time sits (encoder, tail copy).  The
stage's state carries from one repetition to the next as in a replay.  Beside the times: the bytes a download of the travelling blocks
moves without the stage (float32 blocks) and with it.  Prints one table and one JSON line.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, draw, load_package, timed as timed_on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", type=str, nargs="+", default=["2048x16", "256x64"])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.35, 1.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("pcm_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(1)

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="pcm_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.reps} repetitions")
    print("   rows  batches  open   blocks   gate ms   rate   format   pcm ms   (encode / tails)    pcm / gate   float32 MB -> encoded MB")
    for geometry in args.geometries:
        rows, nb = (int(x) for x in geometry.split("x"))
        nblocks = rows * nb
        wave = (torch.rand((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda") * 2.0 - 1.0) * 0.9
        blocks = torch.empty((nblocks, WAVE_BATCH), dtype=torch.float32, device="cuda")
        index = torch.empty((nblocks, 2), dtype=torch.int32, device="cuda")
        row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
        count = torch.empty(2, dtype=torch.int32, device="cuda")
        out = torch.empty((nblocks * 2 * WAVE_BATCH,), dtype=torch.uint8, device="cuda")
        for frac in args.fractions:
            axc = torch.from_numpy(draw(rng, rows, nb, frac, burst=None if frac >= 1.0 else 6.0)).cuda()
            gate = pkg.OutputGate(np.full(rows, pkg.GATE_OPEN_TRAIL, np.uint8), None, max_batches=nb)
            torch.cuda.synchronize()

            def run_gate():
                gate.process_device(wave.data_ptr(), nb * WAVE_BATCH, axc.data_ptr(), nb, nb, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(),
                                    count.data_ptr(), hip_stream=s)

            gate_ms = [timed(run_gate), timed(run_gate)]  # (twice: the spread of the same measurement)
            stream.synchronize()
            travelling = int(count.cpu()[1])  # (stored = travelling: the gate has room for every block)
            for rate in (8000, 16000):
                for fmt, fmt_name in ((pkg.PCM_S16, "s16"), (pkg.PCM_IMA4, "ima4")):
                    pcm = pkg.Pcm(np.ones(rows), max_batches=nb, rate=rate, fmt=fmt)

                    def run_pcm():
                        pcm.process_device(wave.data_ptr(), nb * WAVE_BATCH, nb, index.data_ptr(), count.data_ptr(), out.data_ptr(), hip_stream=s)

                    pcm_ms = [timed(run_pcm), timed(run_pcm)]
                    pcm.set_timing(True)
                    parts = np.zeros(2)
                    for _ in range(args.reps):
                        run_pcm()
                        parts += pcm.last_launch_ms()
                    parts /= args.reps
                    raw_mb, enc_mb = travelling * WAVE_BATCH * 4 / 1e6, travelling * pcm.block_bytes / 1e6
                    pcm.close()
                    share = min(pcm_ms) / min(gate_ms)
                    result["cases"].append(dict(rows=rows, batches=nb, open_fraction=frac, blocks=travelling, gate_ms=gate_ms, rate=rate, format=fmt_name,
                                                pcm_ms=pcm_ms, encode_ms=parts[0], tails_ms=parts[1], pcm_over_gate=share, float32_mb=raw_mb,
                                                encoded_mb=enc_mb))
                    print(f"  {rows:5d}  {nb:7d}  {frac:4.2f}  {travelling:7d}   {min(gate_ms):7.4f}  {rate:5d}   {fmt_name:6s}  {pcm_ms[0]:.4f} {pcm_ms[1]:.4f}   "
                          f"({parts[0]:.4f} / {parts[1]:.4f})   {share:7.2f}      {raw_mb:8.2f} -> {enc_mb:7.2f}")
            gate.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
