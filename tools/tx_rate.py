#!/usr/bin/env python3
"""What the transmission splitter costs beside the output gate.  Needs a GPU.

For each open fraction, HIP events over --reps repetitions after --warmup warm-up ones, on rows x batches of audio already in HBM:
  split   mi_txsplit_process_device alone, and from its per-launch events where the time sits (walk, scan, block statistics, combine)
  gate    mi_outgate_process_device alone under MI_GATE_OPEN_TRAIL on every row: the same travelling blocks, copied
Flags are transmissions of a geometric length (mean --burst batches) placed so that the wanted fraction of batches is open; the state
carries from one repetition to the next as in a replay.  Prints one table and one JSON line.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, draw, load_package, timed as timed_on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=float, default=6.0)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.05, 0.5])
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("tx_rate.py needs a GPU")
    rows, nb = args.rows, args.batches
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(1)
    wave = torch.rand((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda") * 2 - 1
    blocks = torch.empty((rows * nb, WAVE_BATCH), dtype=torch.float32, device="cuda")
    index = torch.empty((rows * nb, 2), dtype=torch.int32, device="cuda")
    records = torch.empty((rows * (nb + 1) * 40,), dtype=torch.uint8, device="cuda")
    row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    count = torch.empty(2, dtype=torch.int32, device="cuda")

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="tx_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, rows=rows, batches=nb, reps=args.reps, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {rows} rows x {nb} batches, {args.reps} repetitions")
    print("  open   blocks  records   split ms   (walk / scan / stats / combine)        gate ms   (rank / scan / copy)       split / gate")
    for frac in args.fractions:
        flags = draw(rng, rows, nb, frac, args.burst)
        axc = torch.from_numpy(flags).cuda()
        tx = pkg.TxSplit(np.ones(rows), max_batches=nb)
        gate = pkg.OutputGate(np.full(rows, pkg.GATE_OPEN_TRAIL, np.uint8), None, max_batches=nb)
        torch.cuda.synchronize()

        def split():
            tx.process_device(wave.data_ptr(), nb * WAVE_BATCH, axc.data_ptr(), nb, nb, records.data_ptr(), row_first.data_ptr(), count.data_ptr(), hip_stream=s)

        def copy():
            gate.process_device(wave.data_ptr(), nb * WAVE_BATCH, axc.data_ptr(), nb, nb, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(),
                                count.data_ptr(), hip_stream=s)

        split_ms, gate_ms = timed(split), timed(copy)
        split_ms2, gate_ms2 = timed(split), timed(copy)  # (alternated once more: the spread of the same measurement)
        tx.set_timing(True)
        gate.set_timing(True)
        sp, gp = np.zeros(4), np.zeros(3)
        for _ in range(args.reps):
            split()
            sp += tx.last_launch_ms()
            copy()
            gp += gate.last_launch_ms()
        sp, gp = sp / args.reps, gp / args.reps
        fresh = np.zeros(rows * 32, np.uint8)
        tx.set_state(fresh)
        gate.set_state(np.zeros(rows, np.uint8))
        copy()
        travelling = int(gate.download(s)[4][0])
        split()
        nrec = int(tx.download(s)[2][0])
        tx.close()
        gate.close()
        result["cases"].append(dict(open_fraction=frac, blocks=travelling, records=nrec, split_ms=[split_ms, split_ms2], gate_ms=[gate_ms, gate_ms2],
                                    walk_ms=sp[0], scan_ms=sp[1], stats_ms=sp[2], combine_ms=sp[3], gate_rank_ms=gp[0], gate_scan_ms=gp[1],
                                    gate_copy_ms=gp[2]))
        print(f"  {frac:4.2f}  {travelling:7d}  {nrec:7d}   {split_ms:.4f} {split_ms2:.4f}   ({sp[0]:.4f} / {sp[1]:.4f} / {sp[2]:.4f} / {sp[3]:.4f})   "
              f"{gate_ms:.4f} {gate_ms2:.4f}   ({gp[0]:.4f} / {gp[1]:.4f} / {gp[2]:.4f})   {min(split_ms, split_ms2) / min(gate_ms, gate_ms2):5.2f}x")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
