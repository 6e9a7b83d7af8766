"""What gate_rate.py and tx_rate.py share: loading the package from the tree, drawing flags, timing by HIP events."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVE_BATCH = 2000


def load_package():
    path = os.path.join(ROOT, "boondock-airband_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location("boondock_airband_amd", path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["boondock_airband_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def draw(rng, rows, nb, frac, burst=None):
    """flags [rows][nb] whose open share is `frac`: independent batches, or with `burst` a two-state chain whose open runs have
    that mean length"""
    if burst is None:
        return np.where(rng.random((rows, nb)) < frac, ord("*"), ord(" ")).astype(np.uint8)
    if frac >= 1.0:
        return np.full((rows, nb), ord("*"), np.uint8)
    p_close = 1.0 / burst
    p_open = min(1.0, p_close * frac / (1.0 - frac))
    flags = np.full((rows, nb), ord(" "), np.uint8)
    for r in range(rows):
        on = rng.random() < frac
        for b in range(nb):
            if on:
                flags[r, b] = ord("*")
            on = (rng.random() >= p_close) if on else (rng.random() < p_open)
    return flags


def timed(torch, stream, fn, warmup, reps):
    """mean ms per repetition by HIP events on the stream"""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps
