#!/usr/bin/env python3
"""What the pager decoder stage costs beside the demodulator call it follows and beside the ACARS and packet stages (DESIGN.md
section 5s).  Needs a GPU.

At 64 x 32 = 2048 rows x 16 batches (the benchmark's config4: 64 streams of 32 mixed channels) the demodulator runs its steady-state
call over a generated capture, and mi_pocsag_process_device runs over an audio plane of the same shape -- white Gaussian noise of
deviation 0.03 on every row: no block is silent, the bank's full cost, the walk idle on random bits -- at its defaults, once per
baud; and over a plane whose every row carries the same transmission through the whole call (a short preamble, then groups of
message words behind one address: the walk inside a transmission from the first batch's end on, a word decoded every 32 slots, one
truncated message open).  Beside it on the noise plane, in the same job: mi_acars_process_device and mi_ax25_process_device at their defaults.  HIP
events over --reps repetitions after --warmup warm-up ones give the time of each call, taken twice to show the spread;
mi_pocsag_last_launch_ms says where the stage's time sits (bits, walk, scan, store, tails), and the walk's time per slot (B * 16
slots a call) stands beside the ACARS walk's per slot (300 * 16).  The stage's state carries from one repetition to the next as in a
replay.  Prints one table and one JSON line; --out writes the line to a file.  The walk decodes a word where it ends, serially; the
lane-per-word decode of a whole group was not built, so there is no figure for it.
"""
import argparse
import json

import os
import sys

import numpy as np

from rate_common import WAVE_BATCH, load_package, timed as timed_on

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

SAMPLE_RATE, AGC_EXTRA = 2560000, 100
NSTREAMS, FFT_LOG, NB = 64, 9, 16
SIGMA = 0.03


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    pkg = load_package()
    if pkg.device_count() < 1:
        raise SystemExit("pocsag_rate.py needs a GPU")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream

    def timed(fn):
        return timed_on(torch, stream, fn, args.warmup, args.reps)

    result = dict(tool="pocsag_rate", device=torch.cuda.get_device_name(0), hip=torch.version.hip, reps=args.reps, warmup=args.warmup, cases=[])
    print(f"{result['device']}, HIP {result['hip']}: {args.reps} repetitions after {args.warmup}")
    centre, chans = pkg.config3_channels()
    rows, nsteps, hop = NSTREAMS * len(chans), NB * WAVE_BATCH, 2 * (SAMPLE_RATE // 16000)
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=FFT_LOG)
    nbytes = ((nsteps + AGC_EXTRA) * hop + 2 * (1 << FFT_LOG) + 255) // 256 * 256
    gcfg = pkg.iqgen_cfg(sample_rate=SAMPLE_RATE, gate_samples=SAMPLE_RATE, carriers=pkg.carriers_for(centre, chans, amp_q8=1024))
    d_iq = torch.empty((NSTREAMS, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(gcfg, 0, NSTREAMS, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    wo = torch.empty((rows, nsteps), dtype=torch.float32, device="cuda")
    ax = torch.empty((rows, NB), dtype=torch.uint8, device="cuda")
    demod = pkg.Demod(dev, chans, nstreams=NSTREAMS, max_batches=NB)
    demod.process_device(d_iq.data_ptr(), nbytes, NB, wo.data_ptr(), ax.data_ptr(), hip_stream=s)  # (the first call takes AGC_EXTRA more windows)
    base = d_iq.data_ptr() + AGC_EXTRA * hop

    def run_demod():
        demod.process_device(base, nbytes, NB, wo.data_ptr(), ax.data_ptr(), hip_stream=s)

    demod_ms = [timed(run_demod), timed(run_demod)]  # (twice: the spread of the same measurement)
    stream.synchronize()
    demod.close()
    del d_iq, wo
    result["demod_ms"] = demod_ms
    noise = (torch.randn((rows, nsteps), dtype=torch.float32, device="cuda") * SIGMA).clamp_(-1.0, 1.0).contiguous()
    first = torch.empty((rows + 1,), dtype=torch.int32, device="cuda")
    count = torch.empty((2,), dtype=torch.int32, device="cuda")
    print(f"  demodulator, {rows} rows x {NB} batches: {demod_ms[0]:.4f} {demod_ms[1]:.4f} ms")
    print("  baud   pager ms          (bits / walk / scan / store / tails)              messages   pager / demod   us / block   walk ns / slot")
    import pocsag_model as m
    for baud, content in [(b, c) for b in (512, 1200, 2400) for c in ("noise", "a transmission on every row")]:
        if content == "noise":
            plane = noise
        else:  # more message words than the call has room for: the transmission never ends in it
            words = [m.message_word((0x12345 * i) & 0xFFFFF) for i in range(NB * m.GEOM[baud][3] // 32 + 16)]
            one = m.render(m.transmission([(0x8, 3, words)], preamble=48), 1234, nsteps, baud, noise=SIGMA, seed=baud).astype(np.float32)
            plane = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(one, (rows, nsteps)))).cuda()
        pg = pkg.Pocsag(np.ones(rows), max_batches=NB, cfg=pkg.pocsag_cfg(baud=baud))
        recs = torch.empty((pg.max_messages * 368,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def run_pager():
            pg.process_device(plane.data_ptr(), nsteps, NB, recs.data_ptr(), first.data_ptr(), count.data_ptr(), hip_stream=s)

        ms = [timed(run_pager), timed(run_pager)]
        pg.set_timing(True)
        parts, nmsgs = np.zeros(5), 0
        for _ in range(args.reps):
            run_pager()
            parts += pg.last_launch_ms()
            nmsgs += int(pg.download(s)[2][0])
        parts /= args.reps
        slots = pg.bits * NB
        pg.close()
        over_demod, us_block, ns_slot = min(ms) / min(demod_ms), 1000.0 * min(ms) / (rows * NB), 1e6 * parts[1] / slots
        result["cases"].append(dict(baud=baud, plane=content, rows=rows, batches=NB, sigma=SIGMA, pocsag_ms=ms, bits_ms=parts[0], walk_ms=parts[1], scan_ms=parts[2],
                                    store_ms=parts[3], tails_ms=parts[4], messages_per_call=nmsgs / args.reps, pocsag_over_demod=over_demod, us_per_block=us_block,
                                    walk_ns_per_slot=ns_slot))
        print(f"  {baud:4d} {content[:8]:8s}  {ms[0]:.4f} {ms[1]:.4f}   ({' / '.join(f'{p:.4f}' for p in parts)})   {nmsgs / args.reps:7.1f}   {over_demod:12.3f}   {us_block:10.3f}   {ns_slot:10.1f}")
    for name, cls, size, slots in (("acars", pkg.Acars, 272, 300 * NB), ("ax25", pkg.Ax25, 352, 150 * NB)):
        st = cls(np.ones(rows), max_batches=NB)
        recs = torch.empty((st.max_frames * size,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def run_other():
            st.process_device(noise.data_ptr(), nsteps, NB, recs.data_ptr(), first.data_ptr(), count.data_ptr(), hip_stream=s)

        ms = [timed(run_other), timed(run_other)]
        st.set_timing(True)
        parts = np.zeros(5)
        for _ in range(args.reps):
            run_other()
            parts += st.last_launch_ms()
        st.close()
        result[f"{name}_ms"], result[f"{name}_parts_ms"] = ms, list(parts / args.reps)
        result[f"{name}_walk_ns_per_slot"] = 1e6 * parts[1] / args.reps / slots
        print(f"  {name} stage on the noise plane: {ms[0]:.4f} {ms[1]:.4f} ms   ({' / '.join(f'{p:.4f}' for p in parts / args.reps)}), "
              f"walk {result[name + '_walk_ns_per_slot']:.1f} ns / slot")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
