#!/usr/bin/env python3
"""Where the channel probe's two classes lie: coherence and cv2 of AM and NFM carriers, measured with the
reference model of tests/probe_model.py on mi_iqgen_host captures.  No GPU.

For each fft size and carrier amplitude one capture of tests/probe_model.GATED_CARRIERS (kinds 0, 1 and 2 twice each) over the
sigma = 2 LSB floor, gated cell by cell so that every carrier is on in --cells / 2 cells.  The chain is the one a caller runs: survey
model -> finder model -> best_bin of each candidate -> probe model -> features masked by the finder's threshold.  Printed per
carrier: coherence, cv2, and the error of carrier_hz against the generator's offset -- of the model, and of the same features taken
from a float64 DFT of the same windowed samples.  Then the classes' extremes, the geometric middles between their nearest values
(the defaults of mi_probe_classify_host) and a JSON line."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import occupancy_model as om  # noqa: E402
import probe_model as pm  # noqa: E402
import survey_model as sv  # noqa: E402
from conftest import load_package  # noqa: E402


def float64_cells(dev, raw, wpc, ncells, b):
    """the model's sums with re, im and m from a float64 DFT of the float32 windowed samples"""
    n = 1 << dev.fft_size_log
    k = np.exp(-2j * np.pi * b * np.arange(n) / n)
    z = np.concatenate([(lambda x: (x[..., 0] + 1j * x[..., 1]) @ k)(sv.windowed(dev, raw, c * wpc, wpc).astype(np.float64)) for c in range(ncells)])
    m = np.abs(z)
    out = np.zeros(ncells, pm.CELL_DTYPE)
    for c in range(ncells):
        w = np.arange(c * wpc, (c + 1) * wpc)
        out[c]["s1"], out[c]["s2"] = m[w].sum(), (m[w] * m[w]).sum()
        w = w[w > 0]
        r = (z[w] * np.conj(z[w - 1])).sum()
        out[c]["r_re"], out[c]["r_im"], out[c]["windows"], out[c]["pairs"] = r.real, r.imag, wpc, w.size
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fft", nargs="+", type=int, default=[8, 9, 11], help="log2 of the fft sizes")
    ap.add_argument("--amps", nargs="+", type=int, default=[3072, 1536], help="amp_q8")
    ap.add_argument("--wpc", type=int, default=500)
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--gate-cells", type=int, default=1, help="the gate turns every this many cells")
    args = ap.parse_args()
    pkg = load_package()
    rows = []
    for log2n in args.fft:
        for amp in args.amps:
            n = 1 << log2n
            dev = pkg.device_cfg(sample_rate=pm.GATED_RATE, centerfreq=sv.CENTRE, fft_size_log=log2n)
            u8 = pm.gated_capture(log2n, amp, args.wpc, args.cells, args.gate_cells)
            mean, peak = sv.survey_model(dev, u8, args.wpc, args.cells)
            mean32 = mean.astype(np.float32)
            bins, cands, _, _ = om.finder(mean32[None], peak[None])
            want = sorted(pm.GATED_CARRIERS)
            if len(cands) != len(want):
                print(f"fft {n} amp_q8 {amp}: the finder gives {len(cands)} candidates for {len(want)} carriers: setting left out")
                continue
            targets = [int(c["best_bin"]) for c in cands]
            cells, _ = pm.probe_model(dev, u8, args.wpc, args.cells, targets)
            for k, (b, (off, kind, _)) in enumerate(zip(targets, want)):
                mask = mean32[:, b] > bins[0, b]["threshold"]
                f = pm.features(dev, b, cells[k], mask)
                f64 = pm.features(dev, b, float64_cells(dev, u8, args.wpc, args.cells, b), mask)
                true = sv.CENTRE + off
                row = dict(fft=n, amp_q8=amp, offset_hz=off, kind=kind, bin=b, active_cells=int(mask.sum()), coherence=f["coherence"], cv2=f["cv2"],
                           carrier_err_hz=f["carrier_hz"] - true, carrier_err_f64_hz=f64["carrier_hz"] - true)
                rows.append(row)
                print(f"fft {n:5d} amp_q8 {amp:5d} kind {kind} offset {off:8d} bin {b:5d} cells {row['active_cells']:3d}: coherence {f['coherence']:.5f} "
                      f"cv2 {f['cv2']:.5f} carrier error {row['carrier_err_hz']:+9.2f} Hz (float64 DFT {row['carrier_err_f64_hz']:+9.2f} Hz)")
    am = [r for r in rows if r["kind"] == 0]
    fm = [r for r in rows if r["kind"] != 0]
    summary = dict(am_coherence=(min(r["coherence"] for r in am), max(r["coherence"] for r in am)),
                   nfm_coherence=(min(r["coherence"] for r in fm), max(r["coherence"] for r in fm)),
                   am_cv2=(min(r["cv2"] for r in am), max(r["cv2"] for r in am)), nfm_cv2=(min(r["cv2"] for r in fm), max(r["cv2"] for r in fm)),
                   carrier_err_hz=max(abs(r["carrier_err_hz"]) for r in rows), carrier_err_f64_hz=max(abs(r["carrier_err_f64_hz"]) for r in rows))
    for name, v in summary.items():
        print(f"  {name}: {v}")
    print(f"  coherence: nearest AM {summary['am_coherence'][0]:.5f}, nearest NFM {summary['nfm_coherence'][1]:.5f}, geometric middle "
          f"{math.sqrt(summary['am_coherence'][0] * summary['nfm_coherence'][1]):.5f}")
    print(f"  cv2: nearest AM {summary['am_cv2'][0]:.5f}, nearest NFM {summary['nfm_cv2'][1]:.5f}, geometric middle "
          f"{math.sqrt(summary['am_cv2'][0] * summary['nfm_cv2'][1]):.5f}")
    print(json.dumps(dict(tool="probe_classes", wpc=args.wpc, cells=args.cells, gate_cells=args.gate_cells, rows=rows, summary=summary)))


if __name__ == "__main__":
    main()
