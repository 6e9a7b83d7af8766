#!/usr/bin/env python3
"""What the channel finder costs (figures in section 6).  Needs a GPU.

Part 1, synthetic planes in HBM -- noise around 1 with a few raised stretches of bins x cells per stream, so that there are floors to
select, activity to count and candidates to write -- for every streams x fft size x cells geometry of --geometries.  A geometry whose
two planes would take more than --plane-gb is shrunk to the streams that fit, and the table says so.
  finder   mi_occupancy_process_device, per launch from the stage's own HIP events (bin records, run starts, scan, candidates): median,
           min and max over --reps calls after --warmup warm-up ones
Part 2, beside the survey: --seconds of 2.56 MS/s u8 signal per stream at fft 512 (cells of one audio batch: 64 s = 512 cells), the
survey's two launches and then the finder on the planes the survey wrote, each from its own events.
Prints one table per part and one JSON line.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, load_package


def spread(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))


def synthetic(torch, ns, ncells, n, seed):
    """(mean, peak) float32 [ns][ncells][n] on the device"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    mean = torch.empty((ns, ncells, n), dtype=torch.float32, device="cuda")
    for s in range(ns):  # (a stream at a time: no second plane-sized temporary)
        mean[s].uniform_(0.9, 1.1, generator=g)
    rng = np.random.default_rng(seed)
    for s in range(ns):
        for _ in range(8):
            b0, width = int(rng.integers(0, n - 13)), int(rng.integers(1, 14))
            c0 = int(rng.integers(0, ncells))
            c1 = min(ncells, c0 + 1 + int(rng.integers(0, max(1, ncells // 4))))
            mean[s, c0:c1, b0:b0 + width] *= float(rng.uniform(5, 40))
    peak = mean * 2.0
    return mean, peak


def time_finder(pkg, torch, stream, occ, d_mean, d_peak, ncells, ns, n, warmup, reps):
    bins = torch.empty(ns * n * 8, dtype=torch.int32, device="cuda")
    cands = torch.empty(occ.max_candidates * 10, dtype=torch.int32, device="cuda")
    first = torch.empty(ns + 1, dtype=torch.int32, device="cuda")
    count = torch.empty(2, dtype=torch.int32, device="cuda")
    stream.synchronize()
    occ.set_timing(True)
    parts = []
    for i in range(warmup + reps):
        occ.process_device(d_mean.data_ptr(), d_peak.data_ptr(), ncells, bins.data_ptr(), cands.data_ptr(), first.data_ptr(), count.data_ptr(),
                           hip_stream=stream.cuda_stream)
        ms = occ.last_launch_ms()
        if i >= warmup:
            parts.append(ms)
    parts = np.array(parts)
    _, _, _, cnt = occ.download(stream.cuda_stream)
    names = ("bins_ms", "starts_ms", "scan_ms", "candidates_ms")
    res = {k: spread(parts[:, i]) for i, k in enumerate(names)}
    res["total_ms"] = spread(parts.sum(axis=1))
    res["candidates"] = int(cnt[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", nargs="+", default=["1x9x512", "64x9x512", "1x13x512", "64x13x512", "1x9x28800", "64x9x28800", "1x13x28800",
                                                        "64x13x28800"], help="streams x log2(fft size) x cells")
    ap.add_argument("--plane-gb", type=float, default=16.0, help="most memory the two planes of a geometry may take")
    ap.add_argument("--seconds", type=float, default=64.0, help="part 2: signal per stream")
    ap.add_argument("--survey-streams", nargs="+", type=int, default=[1, 64])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("occupancy_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    result = dict(tool="occupancy_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, synthetic=[], beside_survey=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.reps} repetitions, ms as median (min .. max)")
    print("  streams   fft   cells   planes GB   bin records            run starts   scan     candidates   total                 found")
    for geo in args.geometries:
        want_ns, log2n, ncells = (int(v) for v in geo.split("x"))
        n = 1 << log2n
        per_stream = 2 * ncells * n * 4
        ns = max(1, min(want_ns, int(args.plane_gb * 2**30 // per_stream)))
        dev = pkg.device_cfg(fft_size_log=log2n)
        d_mean, d_peak = synthetic(torch, ns, ncells, n, seed=log2n * 100003 + ncells)
        occ = pkg.Occupancy(dev, nstreams=ns, max_cells=ncells)
        r = time_finder(pkg, torch, stream, occ, d_mean, d_peak, ncells, ns, n, args.warmup, args.reps)
        occ.close()
        r.update(streams=ns, streams_asked=want_ns, fft_size=n, cells=ncells, planes_gb=ns * per_stream / 2**30)
        result["synthetic"].append(r)
        b, t = r["bins_ms"], r["total_ms"]
        print(f"  {ns:7d}  {n:4d}  {ncells:6d}   {r['planes_gb']:9.3f}   {b['median']:8.4f} ({b['min']:.4f} .. {b['max']:.4f})   {r['starts_ms']['median']:.4f}   "
              f"{r['scan_ms']['median']:.4f}   {r['candidates_ms']['median']:.4f}   {t['median']:8.4f} ({t['min']:.4f} .. {t['max']:.4f})   {r['candidates']}"
              + (f"   (asked for {want_ns} streams)" if ns != want_ns else ""))
        del d_mean, d_peak
        torch.cuda.empty_cache()

    rate, log2n = 2560000, 9
    n = 1 << log2n
    ncells = int(round(args.seconds * pkg.WAVE_RATE / WAVE_BATCH))
    centre, chans = pkg.config2_channels()
    print(f"beside the survey: {args.seconds:g} s of {rate / 1e6:g} MS/s u8 per stream, fft {n}, {ncells} cells of {WAVE_BATCH} windows")
    print("  streams   survey ms (min .. max)        finder ms (min .. max)       finder / survey   found")
    for ns in args.survey_streams:
        dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=log2n)
        survey = pkg.Survey(dev, nstreams=ns, max_cells=ncells)
        need = survey.bytes_needed(ncells)
        stride = (need + 255) // 256 * 256
        iq = torch.empty(ns * stride, dtype=torch.uint8, device="cuda")
        cfg = pkg.iqgen_cfg(sample_rate=rate, carriers=pkg.carriers_for(centre, chans))
        pkg.iqgen_device(cfg, 0, ns, stride, 0, need // 2, iq.data_ptr(), hip_stream=stream.cuda_stream)
        d_mean = torch.empty((ns, ncells, n), dtype=torch.float32, device="cuda")
        d_peak = torch.empty_like(d_mean)
        stream.synchronize()
        survey.set_timing(True)
        sv = []
        for i in range(args.warmup + args.reps):
            survey.process_device(iq.data_ptr(), stride, ncells, d_mean.data_ptr(), d_peak.data_ptr(), hip_stream=stream.cuda_stream)
            ms = survey.last_launch_ms()
            if i >= args.warmup:
                sv.append(sum(ms))
        survey.close()
        occ = pkg.Occupancy(dev, nstreams=ns, max_cells=ncells)
        r = time_finder(pkg, torch, stream, occ, d_mean, d_peak, ncells, ns, n, args.warmup, args.reps)
        occ.close()
        s, t = spread(sv), r["total_ms"]
        r.update(streams=ns, fft_size=n, cells=ncells, survey_ms=s, finder_over_survey=t["median"] / s["median"])
        result["beside_survey"].append(r)
        print(f"  {ns:7d}   {s['median']:9.4f} ({s['min']:.4f} .. {s['max']:.4f})   {t['median']:9.4f} ({t['min']:.4f} .. {t['max']:.4f})   "
              f"{t['median'] / s['median']:8.3f}x   {r['candidates']}")
        del iq, d_mean, d_peak
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
