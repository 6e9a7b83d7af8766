"""The band survey without a GPU: the reference model of tests/survey_model.py against a float64 FFT, and the host half of the
stage -- mi_survey_bin_range against the plan's own bin rule, the byte count, the exported symbols and the refusals."""
import os
import re

import numpy as np
import pytest

import survey_model as sv
from stage1_plans import STAGE1_BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [2560000, 2400000, 2048000, 2500000]  # the last: sample_rate / fft_size truncates


def dev_for(pkg, rate=2560000, log2n=9, sfmt=sv.SFMT_U8, fullscale=127.5):
    return pkg.device_cfg(sample_rate=rate, centerfreq=sv.CENTRE, fft_size_log=log2n, sfmt=sfmt, fullscale=fullscale)


@pytest.mark.parametrize("log2n,sfmt,rate,fullscale", [(8, sv.SFMT_U8, 2560000, 127.5), (9, sv.SFMT_S8, 2400000, 127.5),
                                                       (11, sv.SFMT_S16, 2048000, 32767.0), (13, sv.SFMT_F32, 2560000, 2.0)])
def test_model_magnitudes_against_float64_fft(pkg, log2n, sfmt, rate, fullscale):
    """max |model - |numpy.fft.fft(float64 of the same float32 windowed input)|| over the RMS of that spectrum (all bins of all windows
    compared), within the bound stage 1 is held to (tests/stage1_plans.py: 2.96e-6).
    What that bound means for a whole spectrum: a float32 FFT leaves a bin with an error of about 2^-24 of the bin's own magnitude
    or of the RMS, whichever is larger, so in units of the RMS the figure is about (largest bin / RMS) x 2^-23 -- a statement about
    the input as much as about the FFT.  Stage 1's figure was taken over planes of picked channels, where the two are of one size; a
    full spectrum of 12 LSB carriers over a 2 LSB floor has a largest bin of 52 RMS at fft 8192 (3.98e-6 there).  The capture here
    keeps the largest bin under 25 RMS at every size (carriers of 1 LSB), which the test checks first: 25 x 2^-23 = 2.98e-6."""
    dev = dev_for(pkg, rate, log2n, sfmt, fullscale)
    nwin = 12
    u8 = sv.noise_and_carriers(pkg, rate, sv.samples_needed(dev, nwin), [(-700000, 0), (25000, 0), (901000, 0)], amp_q8=256)
    raw = sv.as_format(u8, sfmt)
    mag = sv.magnitudes(dev, raw, 0, nwin)
    xin = sv.windowed(dev, raw, 0, nwin).astype(np.float64)
    ref = np.abs(np.fft.fft(xin[..., 0] + 1j * xin[..., 1], axis=1))
    scale = float(np.sqrt(np.mean(ref * ref)))
    err = float(np.max(np.abs(mag.astype(np.float64) - ref))) / scale
    print(f"survey model vs float64 FFT: fft {1 << log2n}, format {sfmt}: {err:.3e} of the RMS {scale:.4g}")
    assert scale > 0 and ref.max() < 25 * scale, f"largest bin {ref.max() / scale:.1f} RMS"
    assert err <= STAGE1_BOUND


def plan_bins(pkg, dev, freqs):
    """the bins mi_plan_create / mi_plan_channel give a list of frequencies"""
    p = pkg.Plan(dev, [pkg.channel_cfg(int(f)) for f in freqs])
    bins = np.array([p.channel(i).bin for i in range(len(freqs))], np.int64)
    p.close()
    return bins


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("log2n", [8, 13])
def test_bin_range_round_trip(pkg, rate, log2n):
    """Every bin: lo and hi map to the bin, lo - 1 and hi + 1 do not where they lie inside the band.  The ranges are disjoint and lie
    in the band.  They cannot tile it to the last Hz: the rule's cells are open below and closed above (a frequency on a bin's centre
    lands in the bin below), the band [centre - rate / 2, centre + rate / 2) is the other way round, and it is wider than
    fft_size * (rate // fft_size) where the quotient truncates -- so it holds more than fft_size cells, and a bin beside fft_size / 2
    owns a second, shorter piece at the opposite edge (include/mi_airband.h).  What the ranges leave uncovered is exactly those
    pieces: fewer than 2 q + fft_size frequencies, all at the two edges of the band, every one of them mapped by the plan to a bin
    whose own range lies elsewhere and is at least as long as the piece."""
    n, q = 1 << log2n, rate // (1 << log2n)
    dev = dev_for(pkg, rate, log2n)
    band_lo, band_hi = sv.CENTRE - rate // 2, sv.CENTRE + (rate + 1) // 2 - 1
    rng = np.array([pkg.survey_bin_range(dev, b) for b in range(n)], np.int64)
    lo, hi = rng[:, 0], rng[:, 1]
    assert (lo <= hi).all() and (lo >= band_lo).all() and (hi <= band_hi).all()
    bins = np.arange(n)
    assert np.array_equal(plan_bins(pkg, dev, lo), bins) and np.array_equal(plan_bins(pkg, dev, hi), bins)
    below, above = lo - 1 >= band_lo, hi + 1 <= band_hi
    assert below.sum() >= n - 1 and above.sum() >= n - 1
    assert (plan_bins(pkg, dev, (lo - 1)[below]) != bins[below]).all()
    assert (plan_bins(pkg, dev, (hi + 1)[above]) != bins[above]).all()
    # no overlap, and the gaps
    order = np.argsort(lo)
    slo, shi = lo[order], hi[order]
    assert (slo[1:] > shi[:-1]).all(), "two ranges overlap"
    gaps = [(band_lo, slo[0] - 1)] + [(shi[i] + 1, slo[i + 1] - 1) for i in range(n - 1)] + [(shi[-1] + 1, band_hi)]
    gaps = [(a, b) for a, b in gaps if a <= b]
    uncovered = sum(b - a + 1 for a, b in gaps)
    covered = int((hi - lo + 1).sum())
    print(f"{rate} S/s, fft {n}: q = {q}, {covered} Hz in the ranges, {uncovered} Hz in {len(gaps)} edge pieces: {gaps}")
    assert covered + uncovered == rate
    assert 1 <= uncovered < 2 * q + n
    for a, b in gaps:
        assert b - band_lo < 2 * q + n or band_hi - a < 2 * q + n, "a gap away from the band's edges"
        ends = plan_bins(pkg, dev, [a, b])
        for f, owner in zip((a, b), ends):
            assert not (lo[owner] <= f <= hi[owner])
        if ends[0] == ends[1]:  # one piece of one bin: not longer than the range that bin was given
            assert b - a + 1 <= hi[ends[0]] - lo[ends[0]] + 1


def test_bin_range_refusals(pkg):
    dev = dev_for(pkg, log2n=9)
    for bad in (-1, 512, 1 << 20):
        with pytest.raises(pkg.MiError) as e:
            pkg.survey_bin_range(dev, bad)
        assert e.value.code == pkg.MI_ERR_INVALID and "bin" in str(e.value)
    for log2n in (7, 14):
        with pytest.raises(pkg.MiError) as e:
            pkg.survey_bin_range(dev_for(pkg, log2n=log2n), 0)
        assert e.value.code == pkg.MI_ERR_INVALID
    assert pkg.survey_bin_range(dev, 0)[0] <= pkg.survey_bin_range(dev, 0)[1]


def test_every_survey_symbol_is_declared_and_exported(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_survey_")}
    assert declared == {"mi_survey_create", "mi_survey_destroy", "mi_survey_set_streams", "mi_survey_bytes_needed", "mi_survey_process_device",
                        "mi_survey_set_timing", "mi_survey_last_launch_ms", "mi_survey_bin_range"}
    assert declared <= set(pkg.ABI_SYMBOLS)
    for s in declared:
        assert hasattr(pkg.lib(), s), s


def test_create_refusals_without_a_device(pkg):
    """MI_ERR_NO_DEVICE with a message where no GPU is visible (as test_poststage_refusals.py does for the other stages: on a machine
    with one the same call succeeds); bad arguments are refused before the device is looked for, and a NULL handle everywhere."""
    if pkg.device_count() < 1:
        with pytest.raises(pkg.MiError) as e:
            pkg.Survey(dev_for(pkg), nstreams=1, max_cells=1)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE
        assert "no HIP device: the band survey runs on the GPU only" in str(e.value)
    else:
        pkg.Survey(dev_for(pkg), nstreams=1, max_cells=1).close()
    L = pkg.lib()
    some = np.zeros(64, np.uint8).ctypes.data
    for rc in (L.mi_survey_set_streams(None, None), L.mi_survey_process_device(None, some, 0, 1, some, some, None), L.mi_survey_set_timing(None, 1),
               L.mi_survey_last_launch_ms(None, some)):
        assert rc == pkg.MI_ERR_INVALID and L.mi_last_error() == b"NULL argument"
    assert L.mi_survey_bytes_needed(None, 1) == 0
    L.mi_survey_destroy(None)
    for kw in (dict(nstreams=0), dict(max_cells=0), dict(windows_per_cell=-1)):
        with pytest.raises(pkg.MiError) as e:
            pkg.Survey(dev_for(pkg), **kw)
        assert e.value.code == pkg.MI_ERR_INVALID
    for log2n in (7, 14):
        with pytest.raises(pkg.MiError) as e:
            pkg.Survey(dev_for(pkg, log2n=log2n))
        assert e.value.code == pkg.MI_ERR_INVALID


def test_bytes_needed_formula_in_the_model():
    """mi_survey_bytes_needed takes a handle, and a handle takes a GPU: the call itself is checked against the formula on the device
    (tests/test_gpu_survey.py, every case).  Here: the model's own count of samples is that formula in samples, at every hop."""
    for rate, hop in ((2560000, 160), (2048000, 128), (2400000, 150), (2500000, 156)):
        assert sv.hop_samples(rate) == hop
    import libs
    dev = libs.device_cfg(sample_rate=2400000, fft_size_log=10)
    assert sv.samples_needed(dev, 99) == 98 * 150 + 1024
