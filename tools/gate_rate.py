#!/usr/bin/env python3
"""What the output gate costs beside a plain copy.  Needs a GPU.

For each open fraction, HIP events over --reps repetitions after --warmup warm-up ones:
  gate      mi_outgate_process_device alone on rows x batches of audio already in HBM (rule MI_GATE_OPEN on every row)
  d2d       hipMemcpyAsync device-to-device of the same audio (rows * batches * 8000 bytes): "moves no more than a copy does"
  download  mi_outgate_download of the packed blocks into pinned memory (host clock: it synchronises)
  d2h       hipMemcpyAsync device-to-host of the whole audio into pinned memory
and, from the gate's per-launch events, where its time sits (rank pass, scan, block copy).  Prints one table and one JSON line.
"""
import argparse
import ctypes as C
import json
import time

import numpy as np

from rate_common import WAVE_BATCH, draw, load_package, timed as timed_on

D2H, D2D = 2, 3  # hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice


def hip_runtime():
    """the HIP runtime this process already has (torch's): the one libmi_airband.so is bound to"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64.so" in line:
                rt = C.CDLL(line.split()[-1])
                rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
                return rt
    raise RuntimeError("no HIP runtime loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.05, 0.35, 1.0])
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("gate_rate.py needs a GPU")
    rt = hip_runtime()
    rows, nb = args.rows, args.batches
    nblocks, nbytes = rows * nb, rows * nb * WAVE_BATCH * 4
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(1)
    wave = torch.randn((rows, nb * WAVE_BATCH), dtype=torch.float32, device="cuda")
    copy = torch.empty_like(wave)
    blocks = torch.empty((nblocks, WAVE_BATCH), dtype=torch.float32, device="cuda")
    index = torch.empty((nblocks, 2), dtype=torch.int32, device="cuda")
    row_first = torch.empty(rows + 1, dtype=torch.int32, device="cuda")
    count = torch.empty(2, dtype=torch.int32, device="cuda")
    pinned = pkg.PinnedBuffer(nbytes)
    h_index = pkg.PinnedBuffer(nblocks * 8)
    h_first = np.empty(rows + 1, np.uint32)
    h_count = np.zeros(2, np.uint32)

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    def check(rc):
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed: {rc}")

    d2d_ms = timed(lambda: check(rt.hipMemcpyAsync(copy.data_ptr(), wave.data_ptr(), nbytes, D2D, s)))
    d2h_ms = timed(lambda: check(rt.hipMemcpyAsync(pinned.ptr, wave.data_ptr(), nbytes, D2H, s)))
    result = dict(tool="gate_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, rows=rows, batches=nb, audio_mb=nbytes / 1e6,
                  reps=args.reps, d2d_ms=d2d_ms, d2h_ms=d2h_ms, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {rows} rows x {nb} batches = {nbytes / 1e6:.1f} MB of audio, {args.reps} repetitions")
    print(f"  hipMemcpyAsync device-to-device {d2d_ms:.4f} ms ({nbytes / d2d_ms / 1e6:.0f} GB/s), device-to-host pinned {d2h_ms:.4f} ms "
          f"({nbytes / d2h_ms / 1e6:.1f} GB/s)")
    print("  open   blocks   gate ms   (rank / scan / copy)        vs d2d   download ms   vs d2h")
    for frac in args.fractions:
        flags = draw(rng, rows, nb, frac)
        axc = torch.from_numpy(flags).cuda()
        gate = pkg.OutputGate(np.full(rows, pkg.GATE_OPEN, np.uint8), None, max_batches=nb)
        torch.cuda.synchronize()

        def run():
            gate.process_device(wave.data_ptr(), nb * WAVE_BATCH, axc.data_ptr(), nb, nb, blocks.data_ptr(), index.data_ptr(), row_first.data_ptr(),
                                count.data_ptr(), hip_stream=s)

        gate_ms = timed(run)
        gate.set_timing(True)
        parts = np.zeros(3)
        for _ in range(args.reps):
            run()
            parts += gate.last_launch_ms()
        parts /= args.reps
        gate.set_timing(False)

        def download():
            pkg._check(pkg.lib().mi_outgate_download(gate._h, s, pinned.ptr, None, h_index.ptr, h_first.ctypes.data_as(C.c_void_p),
                                                     h_count.ctypes.data_as(C.c_void_p)))

        run()
        for _ in range(args.warmup):
            download()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            download()
        down_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        travelling = int(h_count[0])
        assert travelling == int((flags != ord(" ")).sum())
        gate.close()
        result["cases"].append(dict(open_fraction=frac, blocks=travelling, gate_ms=gate_ms, rank_ms=parts[0], scan_ms=parts[1], copy_ms=parts[2],
                                    gate_over_d2d=gate_ms / d2d_ms, download_ms=down_ms, download_over_d2h=down_ms / d2h_ms))
        print(f"  {frac:4.2f}  {travelling:7d}   {gate_ms:7.4f}   ({parts[0]:.4f} / {parts[1]:.4f} / {parts[2]:.4f})   {gate_ms / d2d_ms:6.2f}x   "
              f"{down_ms:9.4f}    {down_ms / d2h_ms:5.2f}x")
    pinned.free()
    h_index.free()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
