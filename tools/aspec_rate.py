#!/usr/bin/env python3
"""What the audio spectrum stage costs beside the output gate call it follows.  Needs a GPU.

For each geometry (rows x batches; 2048 x 16 is gate_rate.py's, 256 x 64 has tones_rate.py's batches) and open fraction, audio already
in HBM goes through mi_outgate_process_device (rule MI_GATE_OPEN_TRAIL on every row) and then through mi_aspec_process_device on the
index, row starts and counts the gate left on the device, in three forms: records alone, records and power rows, and those with the
row means.  HIP events over --reps repetitions after --warmup warm-up ones give the time of either call; mi_aspec_last_launch_ms
says where the stage's time sits (blocks, rows).  Prints one table and one JSON line; --out writes the JSON to a file as well.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, draw, load_package, timed as timed_on

BINS = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", type=str, nargs="+", default=["2048x16", "256x64"])
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.35, 1.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("aspec_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(1)

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="aspec_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.reps} repetitions")
    print("   rows  batches  open   blocks   gate ms   outputs                aspec ms        (blocks / rows)    aspec / gate   us per block")
    for geometry in args.geometries:
        rows, nb = (int(x) for x in geometry.split("x"))
        nblocks = rows * nb
        wave = (torch.rand((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda") * 2.0 - 1.0) * 0.9
        blocks = torch.empty((nblocks, WAVE_BATCH), dtype=torch.float32, device="cuda")
        index = torch.empty((nblocks, 2), dtype=torch.int32, device="cuda")
        row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
        count = torch.empty(2, dtype=torch.int32, device="cuda")
        records = torch.empty((nblocks, 8), dtype=torch.int32, device="cuda")
        power = torch.empty((nblocks, BINS), dtype=torch.float32, device="cuda")
        mean = torch.empty((rows, BINS), dtype=torch.float32, device="cuda")
        row_blocks = torch.empty(rows, dtype=torch.int32, device="cuda")
        for frac in args.fractions:
            axc = torch.from_numpy(draw(rng, rows, nb, frac, burst=None if frac >= 1.0 else 6.0)).cuda()
            gate = pkg.OutputGate(np.full(rows, pkg.GATE_OPEN_TRAIL, np.uint8), None, max_batches=nb)
            spec = pkg.Aspec(rows, max_batches=nb)
            torch.cuda.synchronize()

            def run_gate():
                gate.process_device(wave.data_ptr(), nb * WAVE_BATCH, axc.data_ptr(), nb, nb, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(),
                                    count.data_ptr(), hip_stream=s)

            gate_ms = [timed(run_gate), timed(run_gate)]  # (twice: the spread of the same measurement)
            stream.synchronize()
            travelling = int(count.cpu()[1])  # (stored = travelling: the gate has room for every block)
            forms = (("records", None, None, None), ("records, power", power.data_ptr(), None, None),
                     ("records, power, mean", power.data_ptr(), mean.data_ptr(), row_blocks.data_ptr()))
            for name, d_power, d_mean, d_row_blocks in forms:
                def run_spec():
                    spec.process_device(wave.data_ptr(), nb * WAVE_BATCH, nb, index.data_ptr(), row_first.data_ptr(), count.data_ptr(), records.data_ptr(),
                                        d_power, d_mean, d_row_blocks, hip_stream=s)

                spec.set_timing(False)
                spec_ms = [timed(run_spec), timed(run_spec)]
                spec.set_timing(True)
                parts = np.zeros(2)
                for _ in range(args.reps):
                    run_spec()
                    parts += spec.last_launch_ms()
                parts /= args.reps
                share = min(spec_ms) / min(gate_ms)
                per_block = 1e3 * min(spec_ms) / max(travelling, 1)
                result["cases"].append(dict(rows=rows, batches=nb, open_fraction=frac, blocks=travelling, gate_ms=gate_ms, outputs=name, aspec_ms=spec_ms,
                                            blocks_ms=parts[0], rows_ms=parts[1], aspec_over_gate=share, us_per_block=per_block))
                print(f"  {rows:5d}  {nb:7d}  {frac:4.2f}  {travelling:7d}   {min(gate_ms):7.4f}   {name:21s}  {spec_ms[0]:.4f} {spec_ms[1]:.4f}   "
                      f"({parts[0]:.4f} / {parts[1]:.4f})   {share:7.2f}        {per_block:7.3f}")
            spec.close()
            gate.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
