"""The channel probe without a GPU: the host half of the stage (mi_probe_features_host, mi_probe_classify_host,
mi_probe_targets_from_candidates) against the model of tests/probe_model.py, the record layouts, symbols and refusals, and the model
itself against a float64 DFT."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import occupancy_model as om
import probe_model as pm
import survey_model as sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("s1", "s2", "r_re", "r_im")


def dev_for(pkg, rate=2560000, log2n=9):
    return pkg.device_cfg(sample_rate=rate, centerfreq=sv.CENTRE, fft_size_log=log2n)


def steps64(a, b):
    """distance in float64 steps between two finite doubles"""
    a, b = (np.array([v], np.float64).view(np.int64)[0] for v in (a, b))
    a, b = (int(v) if v >= 0 else -(int(v) & 0x7FFFFFFFFFFFFFFF) for v in (a, b))
    return abs(a - b)


def hand_made_cells(rng, ncells, wpc=2000):
    """cells as the device could emit them: s1 ~ wpc * a, s2 ~ wpc * a^2 * (1 + v), R of modulus <= s2 at any angle"""
    cells = np.zeros(ncells, pm.CELL_DTYPE)
    a = rng.uniform(0.5, 40.0, ncells)
    cells["s1"] = wpc * a
    cells["s2"] = wpc * a * a * (1.0 + rng.uniform(0.0, 0.3, ncells))
    mod = cells["s2"] * rng.uniform(0.3, 1.0, ncells)
    ang = rng.uniform(-math.pi, math.pi) + rng.normal(0, 0.05, ncells)
    cells["r_re"], cells["r_im"] = mod * np.cos(ang), mod * np.sin(ang)
    cells["windows"] = wpc
    cells["pairs"] = wpc
    cells["pairs"][0] = wpc - 1
    return cells


def compare(pkg, dev, b, cells, mask):
    got = pkg.probe_features_host(dev, b, cells, mask)
    want = pm.features(dev, b, cells, mask)
    for k in FIELDS:  # the totals: the same additions in the same order
        assert np.float64(getattr(got, k)).tobytes() == np.float64(want[k]).tobytes(), k
    assert got.n == want["n"] and got.pairs == want["pairs"]
    assert steps64(got.cv2, want["cv2"]) <= 4 and steps64(got.coherence, want["coherence"]) <= 4
    assert abs(got.dphi - want["dphi"]) <= 1e-12
    if want["n"]:
        # carrier_hz follows from dphi by the header's formula
        fw = dev.sample_rate / sv.hop_samples(dev.sample_rate)
        f0 = got.dphi / (2.0 * math.pi) * fw
        lo, hi = pkg.survey_bin_range(dev, b)
        assert (lo, hi) == pm.bin_range(dev, b)
        mid = (lo + hi) / 2.0
        assert abs(got.carrier_hz - (dev.centerfreq + f0 + fw * round((mid - dev.centerfreq - f0) / fw))) <= 1e-6
        assert abs(got.carrier_hz - mid) <= fw / 2 + 1e-6
    else:
        assert got.carrier_hz == 0.0 and got.cv2 == 0.0 and got.coherence == 0.0 and got.dphi == 0.0
    return got, want


@pytest.mark.parametrize("rate,log2n", [(2560000, 9), (2560000, 8), (2400000, 10), (2500000, 13), (2048000, 11)])
def test_features_host_against_the_model(pkg, rate, log2n):
    """hand-made cell arrays, every mask edge (all cells by NULL and by an all-ones mask, none, one cell, a random half), bins at the
    edges of the band and beside the centre; 2.5 MS/s has hop 156, so the window rate is not MI_WAVE_RATE"""
    dev = dev_for(pkg, rate, log2n)
    n = 1 << log2n
    rng = np.random.default_rng([rate, log2n])
    for ncells in (1, 2, 17):
        cells = hand_made_cells(rng, ncells)
        masks = [None, np.ones(ncells, bool), np.zeros(ncells, bool), np.arange(ncells) == ncells - 1, np.arange(ncells) == 0, rng.random(ncells) < 0.5]
        for b in (0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1, int(rng.integers(0, n))):
            for mask in masks:
                got, want = compare(pkg, dev, b, cells, mask)
                assert got.n == (ncells if mask is None else int(np.sum(mask))) * 2000
    zero = np.zeros(3, pm.CELL_DTYPE)
    zero["windows"] = 2000  # S1 == 0: digital silence
    got = pkg.probe_features_host(dev, 5, zero)
    assert got.n == 0 and got.s1 == 0.0 and got.carrier_hz == 0.0


def test_classify_host_against_the_model(pkg):
    """the rule at and around both thresholds, with the defaults and with a caller's rule; the defaults are the model's"""
    f = pkg.ProbeFeatures()
    f.n = 2000
    for rule in (None, (0.0, 0.0), (0.8, 0.0), (0.0, 0.2), (0.5, 0.01)):
        cmax = (rule and rule[0]) or pm.COHERENCE_MAX
        vmin = (rule and rule[1]) or pm.CV2_MIN
        for coh in (0.0, np.nextafter(cmax, 0), cmax, np.nextafter(cmax, 2), 1.0):
            for cv2 in (-1e-9, 0.0, np.nextafter(vmin, 0), vmin, np.nextafter(vmin, 2), 0.5):
                f.coherence, f.cv2 = coh, cv2
                want = pm.classify(dict(coherence=coh, cv2=cv2), cmax, vmin)
                assert pkg.probe_classify_host(f, rule) == want, (rule, coh, cv2)
                assert want == (pkg.MOD_NFM if (coh < cmax or cv2 < vmin) else pkg.MOD_AM)
    f.n = 0
    with pytest.raises(pkg.MiError) as e:
        pkg.probe_classify_host(f)
    assert e.value.code == pkg.MI_ERR_INVALID and "nothing to classify" in str(e.value)
    f.n = 1
    for bad in ((-1.0, 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(pkg.MiError) as e:
            pkg.probe_classify_host(f, bad)
        assert e.value.code == pkg.MI_ERR_INVALID


def test_targets_from_candidates(pkg):
    """best_bin of each candidate, sorted by (stream, bin): the finder's order is by position, so the upper half of the bins comes first"""
    rng = np.random.default_rng(7)
    cands = np.zeros(40, pkg.OCC_CAND_DTYPE)
    cands["stream"] = np.sort(rng.integers(0, 4, 40))
    for s in range(4):
        idx = np.flatnonzero(cands["stream"] == s)
        pos = np.sort(rng.choice(512, idx.size, replace=False))
        cands["best_bin"][idx] = (pos + 256) % 512
    cands["lo_bin"] = 99999  # nothing but stream and best_bin is read
    got = pkg.probe_targets_from_candidates(cands)
    want = sorted((int(c["stream"]), int(c["best_bin"])) for c in cands)
    assert got.dtype == pkg.PROBE_TARGET_DTYPE and [(int(t["stream"]), int(t["bin"])) for t in got] == want
    assert any(got["bin"][i] > got["bin"][i + 1] for i in range(39)) is True  # (streams change) and the list differs from the finder's order
    assert [tuple(t) for t in got] != [(int(c["stream"]), int(c["best_bin"])) for c in cands]
    assert pkg.probe_targets_from_candidates(cands[:0]).size == 0


def test_record_sizes_and_symbols(pkg):
    assert C.sizeof(pkg.ProbeCell) == 40 == pkg.PROBE_CELL_DTYPE.itemsize and C.sizeof(pkg.ProbeTarget) == 8 == pkg.PROBE_TARGET_DTYPE.itemsize
    assert C.sizeof(pkg.ProbeFeatures) == 80 and C.sizeof(pkg.ProbeRule) == 16
    assert pkg.PROBE_CELL_DTYPE == pm.CELL_DTYPE and pkg.PROBE_TARGET_DTYPE == pm.TARGET_DTYPE
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    declared = set(re.findall(r"\b(mi_probe_[a-z_]+)\(", header))
    assert declared == {"mi_probe_create", "mi_probe_destroy", "mi_probe_set_targets", "mi_probe_bytes_needed", "mi_probe_process_device",
                        "mi_probe_download", "mi_probe_set_timing", "mi_probe_last_launch_ms", "mi_probe_targets_from_candidates",
                        "mi_probe_features_host", "mi_probe_classify_host"}
    for name in declared:
        assert name in pkg.ABI_SYMBOLS and hasattr(pkg.lib(), name), name


def test_refusals(pkg):
    dev = dev_for(pkg)
    cells = hand_made_cells(np.random.default_rng(1), 4)
    L = pkg.lib()

    def refused(text, rc):
        assert rc == pkg.MI_ERR_INVALID and text in L.mi_last_error().decode(), L.mi_last_error()

    f = pkg.ProbeFeatures()
    p = cells.ctypes.data_as(C.c_void_p)
    refused("NULL argument", L.mi_probe_features_host(None, 0, p, 4, None, C.byref(f)))
    refused("NULL argument", L.mi_probe_features_host(C.byref(dev), 0, None, 4, None, C.byref(f)))
    refused("NULL argument", L.mi_probe_features_host(C.byref(dev), 0, p, 4, None, None))
    refused("ncells must be at least 1", L.mi_probe_features_host(C.byref(dev), 0, p, 0, None, C.byref(f)))
    refused("bin outside 0 .. fft_size - 1", L.mi_probe_features_host(C.byref(dev), 512, p, 4, None, C.byref(f)))
    refused("bin outside 0 .. fft_size - 1", L.mi_probe_features_host(C.byref(dev), -1, p, 4, None, C.byref(f)))
    refused("fft_size", L.mi_probe_features_host(C.byref(dev_for(pkg, log2n=14)), 0, p, 4, None, C.byref(f)))
    mod = C.c_int()
    refused("NULL argument", L.mi_probe_classify_host(None, None, C.byref(mod)))
    refused("NULL argument", L.mi_probe_classify_host(C.byref(f), None, None))
    refused("NULL argument", L.mi_probe_targets_from_candidates(None, 0, p))
    out = C.c_void_p()
    refused("NULL argument", L.mi_probe_create(None, 1, 1, 0, 1, 0, C.byref(out)))
    for args in ((0, 1, 0, 1), (1, 0, 0, 1), (1, 1, -1, 1), (1, 1, (1 << 20) + 1, 1)):
        refused("channel probe needs 1 <= nstreams", L.mi_probe_create(C.byref(dev), *args, 0, C.byref(out)))
    for max_targets in (0, -1, 2 * 512 + 1):
        refused("max_targets", L.mi_probe_create(C.byref(dev), 2, 1, 0, max_targets, 0, C.byref(out)))
    refused("max_targets * max_cells < 2^31", L.mi_probe_create(C.byref(dev), 64, 1 << 20, 1, 2048, 0, C.byref(out)))
    refused("fft_size", L.mi_probe_create(C.byref(dev_for(pkg, log2n=7)), 1, 1, 0, 1, 0, C.byref(out)))
    assert L.mi_probe_bytes_needed(None, 1) == 0
    if pkg.device_count() < 1:
        with pytest.raises(pkg.MiError) as e:
            pkg.Probe(dev)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE and "no HIP device: the channel probe runs on the GPU only" in str(e.value)


# ---- the model against a float64 DFT: one unmodulated carrier at a known place inside a bin

TONE_OFFSET = 301700  # Hz above the centre: 60.34 bins of 5 kHz
# |carrier_hz - the carrier| of the float64 DFT on this capture (12 LSB carrier, sigma = 2 LSB Gaussian noise, u8 rounding, 4 cells of
# 200 windows): measured 0.1112 Hz.  It is the noise in the bin that sets it, not the arithmetic: the phase of one window's bin is off by
# about noise / carrier = 0.01 rad, and 799 pairs average that down.
TONE_F64_ERR_HZ = 0.112
# the float32 model beside the float64 DFT: a bin of the float32 FFT is off by about 2^-23 of its magnitude, so a pair's phase by
# about 2.4e-7 rad = 6e-4 Hz at 16000 windows a second, before any averaging.  Measured: under 1e-9 Hz.
TONE_MODEL_MARGIN_HZ = 1e-3


def test_model_carrier_against_float64_dft(pkg):
    dev = dev_for(pkg)
    n, hop, wpc, ncells = 512, 160, 200, 4
    b = 60
    rng = np.random.default_rng(0x70E)
    t = np.arange(sv.samples_needed(dev, wpc * ncells))
    ph = 2.0 * np.pi * TONE_OFFSET * t / dev.sample_rate
    iq = np.stack([127.5 + 12.0 * np.cos(ph), 127.5 + 12.0 * np.sin(ph)], axis=1) + rng.normal(0.0, 2.0, (t.size, 2))
    u8 = np.clip(np.floor(iq + 0.5), 0, 255).astype(np.uint8).reshape(-1)
    cells, scale = pm.probe_model(dev, u8, wpc, ncells, [b])
    assert cells["pairs"].tolist() == [[wpc - 1, wpc, wpc, wpc]] and (cells["windows"] == wpc).all()
    f = pm.features(dev, b, cells[0])
    # the same sums from a float64 DFT of the same float32 windowed samples
    k = np.exp(-2j * np.pi * b * np.arange(n) / n)
    x = sv.windowed(dev, u8, 0, wpc * ncells).astype(np.float64)
    z = (x[..., 0] + 1j * x[..., 1]) @ k
    ref = np.zeros(ncells, pm.CELL_DTYPE)
    for c in range(ncells):
        w = np.arange(c * wpc, (c + 1) * wpc)
        ref[c]["s1"], ref[c]["s2"], ref[c]["windows"] = np.abs(z[w]).sum(), (np.abs(z[w]) ** 2).sum(), wpc
        w = w[w > 0]
        r = (z[w] * np.conj(z[w - 1])).sum()
        ref[c]["r_re"], ref[c]["r_im"], ref[c]["pairs"] = r.real, r.imag, w.size
    f64 = pm.features(dev, b, ref)
    true = sv.CENTRE + TONE_OFFSET
    print(f"one carrier at +{TONE_OFFSET} Hz: float64 DFT {f64['carrier_hz'] - true:+.4f} Hz, model {f['carrier_hz'] - true:+.4f} Hz, "
          f"model - float64 {f['carrier_hz'] - f64['carrier_hz']:+.3e} Hz; coherence {f['coherence']:.6f}, cv2 {f['cv2']:.6f}")
    assert abs(f64["carrier_hz"] - true) <= TONE_F64_ERR_HZ
    assert abs(f["carrier_hz"] - true) <= TONE_F64_ERR_HZ + TONE_MODEL_MARGIN_HZ
    assert abs(f["carrier_hz"] - f64["carrier_hz"]) <= TONE_MODEL_MARGIN_HZ
    for name in FIELDS:  # and the sums themselves: within the float32 FFT's 2^-23 or so of the scale of their terms
        tol = 4e-6 * (float(scale[0].sum()) if name.startswith("r_") else float(ref[name].sum()))
        assert abs(float(cells[0][name].sum()) - float(ref[name].sum())) <= tol, name
    lo, hi = pkg.survey_bin_range(dev, b)
    assert lo <= f["carrier_hz"] <= hi
    # the host function on the model's cells gives the model's features
    got, _ = compare(pkg, dev, b, cells[0], None)
    assert pkg.probe_classify_host(got) == pm.classify(f) == pm.MOD_NFM  # an unmodulated carrier has a constant envelope
