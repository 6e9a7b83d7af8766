#!/usr/bin/env python3
"""What the channel probe costs beside the band survey (figures in section 6).  Needs a GPU.

For each geometry (streams x fft size x targets per stream, --seconds of 2.56 MS/s u8 signal already in HBM, cells of one audio batch),
on the same capture:
  probe   mi_probe_process_device, per launch from the stage's own HIP events (windows, reduce): median, min and max over --reps calls
          after --warmup warm-up ones.  The targets are spread evenly over the bins.
  survey  mi_survey_process_device, the same way (windows, fold).  It runs the same windows and keeps every bin.
Prints one table and one JSON line; with --out DIR also writes them to DIR/probe_rate.txt and DIR/probe_rate.json.
"""
import argparse
import json
import os

import numpy as np

from rate_common import WAVE_BATCH, load_package


def spread(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))


def timed_calls(handle, call, warmup, reps):
    handle.set_timing(True)
    parts = []
    for i in range(warmup + reps):
        call()
        ms = handle.last_launch_ms()
        if i >= warmup:
            parts.append(ms)
    parts = np.array(parts)
    return spread(parts[:, 0]), spread(parts[:, 1]), spread(parts.sum(axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", nargs="+", default=["1x9x8", "1x9x64", "64x9x8", "1x11x8", "1x13x8"], help="streams x log2(fft size) x targets per stream")
    ap.add_argument("--seconds", type=float, default=64.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for probe_rate.txt and probe_rate.json")
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("probe_rate.py needs a GPU")
    rate = 2560000
    ncells = int(round(args.seconds * pkg.WAVE_RATE / WAVE_BATCH))
    centre, chans = pkg.config2_channels()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    result = dict(tool="probe_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, sample_rate=rate, seconds=args.seconds,
                  cells=ncells, reps=args.reps, cases=[])
    lines = [f"{result['device']}, HIP {result['hip']}: {args.seconds:g} s of {rate / 1e6:g} MS/s u8 per stream = {ncells} cells of {WAVE_BATCH} windows, "
             f"{args.reps} repetitions",
             "  streams   fft  targets   probe ms: windows (min .. max)   reduce (min .. max)   scratch MB    survey ms: windows   fold    probe / survey"]
    print("\n".join(lines))
    for geo in args.geometries:
        ns, log2n, per = (int(v) for v in geo.split("x"))
        dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=log2n)
        n = 1 << log2n
        targets = [(st, b) for st in range(ns) for b in sorted({(k * n) // per for k in range(per)})]
        survey = pkg.Survey(dev, nstreams=ns, max_cells=ncells)
        probe = pkg.Probe(dev, nstreams=ns, max_cells=ncells, max_targets=len(targets))
        probe.set_targets(targets)
        need = survey.bytes_needed(ncells)
        assert probe.bytes_needed(ncells) == need
        stride = (need + 255) // 256 * 256
        iq = torch.empty(ns * stride, dtype=torch.uint8, device="cuda")
        cfg = pkg.iqgen_cfg(sample_rate=rate, carriers=pkg.carriers_for(centre, chans))
        pkg.iqgen_device(cfg, 0, ns, stride, 0, need // 2, iq.data_ptr(), hip_stream=s)
        mean = torch.empty((ns, ncells, n), dtype=torch.float32, device="cuda")
        peak = torch.empty_like(mean)
        cells = torch.empty(len(targets) * ncells * 40, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        pw, pr, pt = timed_calls(probe, lambda: probe.process_device(iq.data_ptr(), stride, ncells, cells.data_ptr(), hip_stream=s), args.warmup, args.reps)
        sw, sf, st_ = timed_calls(survey, lambda: survey.process_device(iq.data_ptr(), stride, ncells, mean.data_ptr(), peak.data_ptr(), hip_stream=s),
                                  args.warmup, args.reps)
        scratch_mb = 8.0 * len(targets) * ncells * WAVE_BATCH / 1e6
        case = dict(streams=ns, fft_size=n, targets=len(targets), iq_mb=ns * need / 1e6, scratch_mb=scratch_mb, probe_windows_ms=pw, probe_reduce_ms=pr,
                    probe_ms=pt, survey_windows_ms=sw, survey_fold_ms=sf, survey_ms=st_, probe_over_survey=pt["median"] / st_["median"],
                    windows_per_s=ns * ncells * WAVE_BATCH / (pt["median"] * 1e-3))
        line = (f"  {ns:7d}  {n:4d}  {len(targets):7d}   {pw['median']:9.4f} ({pw['min']:.4f} .. {pw['max']:.4f})   {pr['median']:.4f} ({pr['min']:.4f} .. "
                f"{pr['max']:.4f})   {scratch_mb:10.1f}    {sw['median']:9.4f}   {sf['median']:.4f}   {case['probe_over_survey']:6.2f}x")
        print(line)
        lines.append(line)
        result["cases"].append(case)
        survey.close()
        probe.close()
        del iq, mean, peak, cells
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "probe_rate.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(args.out, "probe_rate.json"), "w") as f:
            f.write(json.dumps(result) + "\n")


if __name__ == "__main__":
    main()
