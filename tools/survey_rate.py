#!/usr/bin/env python3
"""What the band survey costs beside stage 1 (figures in section 6).  Needs a GPU.

For each geometry (streams x fft size, --seconds of 2.56 MS/s u8 signal already in HBM, cells of one audio batch):
  survey   mi_survey_process_device, per launch from the stage's own HIP events (windows, fold): median, min and max over --reps
           calls after --warmup warm-up ones
  stage 1  the exchange kernel's full graph on a demod handle of the same geometry and the same IQ (8 AM channels, MI_OPT_LANE_FFT = 0,
           MI_OPT_PRUNE_FFT = 0, serial stage 2 so that the call has one stage-1 launch and nothing runs beside it): index 0 of
           mi_demod_kernel_time, over --demod-reps calls after one warm-up call.  It does the same butterflies and writes less.
           With --prune it is the pruned graph instead (k_channelize9p, fft 512).
Prints one table and one JSON line.
"""
import argparse
import json

import numpy as np

from rate_common import WAVE_BATCH, load_package


def spread(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), min=float(x.min()), max=float(x.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometries", nargs="+", default=["1x9", "64x9", "1x11", "1x13"], help="streams x log2(fft size)")
    ap.add_argument("--seconds", type=float, default=64.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--demod-reps", type=int, default=3)
    ap.add_argument("--no-stage1", action="store_true", help="the survey alone")
    ap.add_argument("--prune", action="store_true", help="stage 1 on the exchange kernel's pruned graph (MI_OPT_PRUNE_FFT = 1, fft 512 only)")
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("survey_rate.py needs a GPU")
    rate = 2560000
    ncells = int(round(args.seconds * pkg.WAVE_RATE / WAVE_BATCH))
    centre, chans = pkg.config2_channels()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    result = dict(tool="survey_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, sample_rate=rate, seconds=args.seconds,
                  cells=ncells, reps=args.reps, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.seconds:g} s of {rate / 1e6:g} MS/s u8 per stream = {ncells} cells of {WAVE_BATCH} windows, "
          f"{args.reps} repetitions")
    print("  streams   fft   survey ms: windows (min .. max)   fold (min .. max)    stage 1 ms (min .. max)   survey / stage 1")
    for geo in args.geometries:
        ns, log2n = (int(v) for v in geo.split("x"))
        dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=log2n)
        n = 1 << log2n
        survey = pkg.Survey(dev, nstreams=ns, max_cells=ncells)
        demod = None
        need = survey.bytes_needed(ncells)
        if not args.no_stage1:
            demod = pkg.Demod(dev, chans, nstreams=ns, max_batches=ncells)
            demod.set_option(pkg.OPT_LANE_FFT, 0)
            demod.set_option(pkg.OPT_PRUNE_FFT, 1 if args.prune else 0)
            demod.set_option(pkg.OPT_TIME_PARALLEL, 0)
            need = max(need, demod.bytes_needed(ncells))  # (a handle's first call: AGC_EXTRA more windows)
        stride = (need + 255) // 256 * 256
        iq = torch.empty(ns * stride, dtype=torch.uint8, device="cuda")
        cfg = pkg.iqgen_cfg(sample_rate=rate, carriers=pkg.carriers_for(centre, chans))
        pkg.iqgen_device(cfg, 0, ns, stride, 0, need // 2, iq.data_ptr(), hip_stream=s)
        mean = torch.empty((ns, ncells, n), dtype=torch.float32, device="cuda")
        peak = torch.empty_like(mean)
        stream.synchronize()
        survey.set_timing(True)
        parts = []
        for i in range(args.warmup + args.reps):
            survey.process_device(iq.data_ptr(), stride, ncells, mean.data_ptr(), peak.data_ptr(), hip_stream=s)
            ms = survey.last_launch_ms()
            if i >= args.warmup:
                parts.append(ms)
        parts = np.array(parts)
        win, fold = spread(parts[:, 0]), spread(parts[:, 1])
        total = spread(parts.sum(axis=1))
        case = dict(streams=ns, fft_size=n, iq_mb=ns * need / 1e6, survey_windows_ms=win, survey_fold_ms=fold, survey_ms=total,
                    windows_per_s=ns * ncells * WAVE_BATCH / (total["median"] * 1e-3))
        line = (f"  {ns:7d}  {n:4d}   {win['median']:9.4f} ({win['min']:.4f} .. {win['max']:.4f})   {fold['median']:.4f} ({fold['min']:.4f} .. "
                f"{fold['max']:.4f})")
        survey.close()
        if demod is not None:
            wave = torch.empty((ns, len(chans), ncells * WAVE_BATCH), dtype=torch.float32, device="cuda")
            axc = torch.empty((ns, len(chans), ncells), dtype=torch.uint8, device="cuda")
            st1 = []
            for i in range(1 + args.demod_reps):
                demod.process_device(iq.data_ptr(), stride, ncells, wave.data_ptr(), axc.data_ptr(), hip_stream=s)
                stream.synchronize()
                name, ms, launches = demod.kernel_times()[0]
                assert demod.last_stage1() == (1 if args.prune else 0), "not the exchange kernel that was asked for"
                if i >= 1:
                    st1.append(ms)
            demod.close()
            del wave, axc
            st = spread(st1)
            case.update(stage1_kernel=name, stage1_launches=launches, stage1_ms=st, survey_over_stage1=total["median"] / st["median"])
            line += f"    {st['median']:9.4f} ({st['min']:.4f} .. {st['max']:.4f})   {total['median'] / st['median']:6.2f}x"
        print(line)
        result["cases"].append(case)
        del iq, mean, peak
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
