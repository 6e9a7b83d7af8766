#!/usr/bin/env python3
"""Generates tests/golden/components_ref.npz from the REFERENCE's own compiled classes (oracle/_ref,
built by `make -C oracle ref` from /root/reference/src/{squelch,ctcss,filters,logging,generate_signal}.cpp).

Run in the build container only (the reference does not travel to the GPU box):
    python tests/golden/gen_golden.py [components] [sweeps]     (default: both)
The committed .npz holds inputs-by-seed parameters and the reference's OUTPUTS (flags, levels, filter
outputs, counters) -- data, no reference source.  tests/test_oracle_components.py replays the same seeded
inputs through the oracle and requires identical bits; that pins the oracle on machines without _ref.
tests/golden/ref_sweeps.npz holds the reference's answers to the longer random sweeps (sha256 digests of the long
outputs, counters and levels in full), the standard tone list and whether default-constructed filters are disabled.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import libs  # noqa: E402
from golden_inputs import (CTCSS_CASES, FILTER_CASES, SQUELCH_CASES, SQUELCH_SWEEP_SEEDS, digest, make_audio, make_filtered,  # noqa: E402
                           make_raw, squelch_sweep, tone_bank_inputs)


FILES = {"components": "components_ref.npz", "sweeps": "ref_sweeps.npz"}


def components(r):
    out = {}
    for name, case in SQUELCH_CASES.items():
        raw = make_raw(case)
        filt = make_filtered(case, raw) if case.get("filt") else None
        audio = make_audio(case) if case.get("audio") else None
        res = r.squelch_run(raw, filt=filt, audio=audio, manual_level=case.get("manual_level", 0.0), snr_db=case.get("snr_db"),
                            ctcss_freq=case.get("ctcss_freq", 0.0), ctcss_rate=case.get("ctcss_rate", 16000))
        out[f"sq_{name}_flags"] = res["flags"]
        out[f"sq_{name}_level"] = res["level"]
        out[f"sq_{name}_noise"] = res["noise"]
        out[f"sq_{name}_signal"] = res["signal"]
        f = res["final"]
        out[f"sq_{name}_final_counts"] = np.array([f.open_count, f.flappy_count, f.ctcss_count, f.no_ctcss_count], np.uint64)
        out[f"sq_{name}_final_levels"] = np.array([f.noise_level, f.signal_level, f.squelch_level], np.float32)
    for name, case in CTCSS_CASES.items():
        x = make_audio(case)
        flags, found, nfound = r.ctcss_run(case["freq"], case["rate"], case["window"], x)
        out[f"ct_{name}_flags"] = flags
        out[f"ct_{name}_counts"] = np.array([found, nfound], np.uint64)
    for name, case in FILTER_CASES.items():
        rng = np.random.default_rng(case["seed"])
        x = rng.normal(size=case["n"]).astype(np.float32)
        y = rng.normal(size=case["n"]).astype(np.float32)
        if case["kind"] == "notch":
            out[f"fl_{name}_y"] = r.notch_run(case["freq"], 16000.0, case["q"], x)
        else:
            a, b = r.lowpass_run(case["freq"], 16000.0, x, y)
            out[f"fl_{name}_re"] = a
            out[f"fl_{name}_im"] = b
    out["tone_79_7"] = r.tone_run(8000, 79.7, 0.2, 4000)
    return out


def sweeps(r):
    """The reference's answers to the longer sweeps of tests/test_oracle_components.py: sha256 digests of the long outputs,
    counters and final levels in full."""
    import ctypes as C
    out = {}
    for seed in SQUELCH_SWEEP_SEEDS:
        raw, kws = squelch_sweep(seed)
        for i, kw in enumerate(kws):
            res = r.squelch_run(raw, **kw)
            for key in ("flags", "level", "noise", "signal"):
                out[f"sw{seed}_{i}_{key}"] = digest(res[key])
            f = res["final"]
            out[f"sw{seed}_{i}_final_counts"] = np.array([f.open_count, f.flappy_count, f.ctcss_count, f.no_ctcss_count], np.uint64)
            out[f"sw{seed}_{i}_final_levels"] = np.array([f.noise_level, f.signal_level, f.squelch_level], np.float32)
    tones = np.zeros(64, np.float32)
    r.lib.ref_standard_tones.argtypes = [np.ctypeslib.ndpointer(np.float32), C.c_int]
    r.lib.ref_standard_tones.restype = C.c_int
    tones = tones[:r.lib.ref_standard_tones(tones, 64)]
    out["standard_tones"] = tones
    flags, counts = [], []
    for t, rate, win, x in tone_bank_inputs(tones):
        f, found, nfound = r.ctcss_run(t, rate, win, x)
        flags.append(digest(f))
        counts.append((found, nfound))
    out["tone_bank_flags"] = np.stack(flags)
    out["tone_bank_counts"] = np.array(counts, np.uint64)
    r.lib.ref_filters_default_disabled.restype = C.c_int
    out["filters_default_disabled"] = np.array(r.lib.ref_filters_default_disabled(), np.int32)
    return out


def main():
    r = libs.ref()
    if r is None:
        raise SystemExit("oracle/_ref/libairband_ref.so unavailable: build it with `make -C oracle ref`")
    which = sys.argv[1:] or ["components", "sweeps"]
    for name, make in (("components", components), ("sweeps", sweeps)):
        if name not in which:
            continue
        out = make(r)
        path = os.path.join(HERE, FILES[name])
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
