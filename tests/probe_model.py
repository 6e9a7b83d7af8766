"""Reference model of the channel probe (mi_probe_*, csrc/probe.hip; definition in include/mi_airband.h "channel probe") and the
captures its tests share.

The model is the definition in numpy, not a twin of the code under test: survey_model.spectra() gives re and im of every window --
the oracle's bits --, m = sqrtf(re * re + im * im) in float32 as survey_model.magnitudes() forms it, and per (target, cell) the four
float64 sums are taken in window order, one addition after the other, the pair (w, w - 1) belonging to the
cell of w and window 0 of the call having none.  pair_scale = the sum of (double)m_w * (double)m_p over a cell's pairs is what the
tolerance of r_re and r_im is stated in.  features() and classify() are float64 Python."""
import functools
import math

import numpy as np

import survey_model as sv

CELL_DTYPE = np.dtype([("s1", "<f8"), ("s2", "<f8"), ("r_re", "<f8"), ("r_im", "<f8"), ("windows", "<u4"), ("pairs", "<u4")])
TARGET_DTYPE = np.dtype([("stream", "<u4"), ("bin", "<u4")])
assert CELL_DTYPE.itemsize == 40 and TARGET_DTYPE.itemsize == 8
MOD_AM, MOD_NFM = 0, 1


def _ordered_sum(x):
    """float64 sum in index order (np.sum adds pairwise)"""
    acc = 0.0
    for v in x.tolist():
        acc += v
    return acc


def bin_values(dev, raw, nwin, bins):
    """float32 re, im [len(bins)][nwin] of the bins over windows 0 .. nwin - 1 of one stream's capture, in pieces that bound the memory"""
    n = 1 << dev.fft_size_log
    piece = max(1, (1 << 22) // n)
    bins = np.asarray(bins, np.int64)
    re = np.empty((bins.size, nwin), np.float32)
    im = np.empty((bins.size, nwin), np.float32)
    for w0 in range(0, nwin, piece):
        z = sv.spectra(dev, raw, w0, min(piece, nwin - w0))
        re[:, w0:w0 + z.shape[0]] = z[:, bins, 0].T
        im[:, w0:w0 + z.shape[0]] = z[:, bins, 1].T
    return re, im


def cells_of(re, im, wpc, ncells):
    """(CELL_DTYPE [ncells], pair_scale float64 [ncells]) of one target: re, im float32 [>= ncells * wpc]"""
    assert re.dtype == np.float32 and im.dtype == np.float32
    m = np.sqrt(re * re + im * im)
    assert m.dtype == np.float32
    md, red, imd = m.astype(np.float64), re.astype(np.float64), im.astype(np.float64)
    out = np.zeros(ncells, CELL_DTYPE)
    scale = np.zeros(ncells, np.float64)
    for c in range(ncells):
        w = np.arange(c * wpc, (c + 1) * wpc)
        out[c]["s1"] = _ordered_sum(md[w])
        out[c]["s2"] = _ordered_sum(md[w] * md[w])
        w = w[w > 0]
        p = w - 1
        out[c]["r_re"] = _ordered_sum(red[w] * red[p] + imd[w] * imd[p])  # exact products, one rounding per term
        out[c]["r_im"] = _ordered_sum(imd[w] * red[p] - red[w] * imd[p])
        out[c]["windows"] = wpc
        out[c]["pairs"] = w.size
        scale[c] = _ordered_sum(md[w] * md[p])
    return out, scale


def probe_model(dev, raw, wpc, ncells, bins):
    """(CELL_DTYPE [len(bins)][ncells], pair_scale [len(bins)][ncells]) of one stream's capture"""
    re, im = bin_values(dev, raw, wpc * ncells, bins)
    got = [cells_of(re[k], im[k], wpc, ncells) for k in range(len(bins))]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def bin_range(dev, b):
    """mi_survey_bin_range's rule, restated: the longest piece of the band that the plan's bin rule sends to bin b"""
    n, sr = 1 << dev.fft_size_log, dev.sample_rate
    q = sr // n
    d_first, d_last = sr - sr // 2, sr + (sr + 1) // 2 - 1
    best = None
    k = b
    while k * q + 1 <= d_last:
        lo, hi = max(k * q + 1, d_first), min((k + 1) * q, d_last)
        if hi >= lo and (best is None or hi - lo > best[1] - best[0]):
            best = (lo, hi)
        k += n
    return best[0] - sr + dev.centerfreq, best[1] - sr + dev.centerfreq


def features(dev, b, cells, mask=None):
    """dict of the totals over the selected cells (added in cell order), n, pairs, cv2, coherence, dphi, carrier_hz"""
    s1 = s2 = rr = ri = 0.0
    n = pairs = 0
    for c in range(len(cells)):
        if mask is not None and not mask[c]:
            continue
        s1 += float(cells[c]["s1"])
        s2 += float(cells[c]["s2"])
        rr += float(cells[c]["r_re"])
        ri += float(cells[c]["r_im"])
        n += int(cells[c]["windows"])
        pairs += int(cells[c]["pairs"])
    if n == 0 or s1 == 0.0:
        return dict(s1=0.0, s2=0.0, r_re=0.0, r_im=0.0, n=0, pairs=0, cv2=0.0, coherence=0.0, dphi=0.0, carrier_hz=0.0)
    dphi = math.atan2(ri, rr)
    fw = dev.sample_rate / sv.hop_samples(dev.sample_rate)
    f0 = dphi / (2.0 * math.pi) * fw
    lo, hi = bin_range(dev, b)
    mid = (lo + hi) / 2.0
    carrier = dev.centerfreq + f0 + fw * round((mid - dev.centerfreq - f0) / fw)
    return dict(s1=s1, s2=s2, r_re=rr, r_im=ri, n=n, pairs=pairs, cv2=n * s2 / (s1 * s1) - 1.0, coherence=math.hypot(rr, ri) / s2, dphi=dphi,
                carrier_hz=carrier)


# the defaults of mi_probe_classify_host, measured by tools/probe_classes.py: the geometric middles between the
# classes' nearest values
COHERENCE_MAX, CV2_MIN = 0.9314, 0.1005


def classify(f, coherence_max=COHERENCE_MAX, cv2_min=CV2_MIN):
    return MOD_NFM if (f["coherence"] < coherence_max or f["cv2"] < cv2_min) else MOD_AM


# ------------------------------------------------------------------ the gated-carrier capture of the classification and end-to-end tests

# (offset from the centre in Hz, iqgen kind: 0 AM, 1 NFM, 2 NFM + CTCSS, gate phase).  At 2.56 MS/s every carrier is at least 25 bins of
# fft 256 from the next, so the Blackman-7 lobes (about 13 bins) do not overlap at any size.  Each sits 250 .. 450 Hz above a multiple
# of 10 kHz: at fft 256, 512 and 2048 that is 0.02 .. 0.36 of a bin above an FFT bin's centre, so the strongest FFT bin is also the
# bin the plan's rule -- which sends the frequencies from one bin centre up to the next to the lower bin -- gives the carrier.
GATED_CARRIERS = [(-699700, 0, 0), (-449600, 1, 1), (200300, 2, 1), (450400, 0, 1), (700250, 1, 0), (950450, 2, 0)]
GATED_RATE = 2560000


@functools.lru_cache(maxsize=4)
def gated_capture(log2n, amp_q8, wpc, ncells, gate_cells):
    """(dev fields are the caller's; u8 capture exactly as long as the survey reads): sigma = 2 LSB noise and GATED_CARRIERS, the gate
    turning every gate_cells cells: phase 0 is on in the odd groups of gate_cells cells, phase 1 in the even ones"""
    from conftest import load_package
    pkg = load_package()
    dev = pkg.device_cfg(sample_rate=GATED_RATE, centerfreq=sv.CENTRE, fft_size_log=log2n)
    hop = sv.hop_samples(GATED_RATE)
    cfg = pkg.iqgen_cfg(sample_rate=GATED_RATE, seed=0x5EED, noise_q8_mul=111, gate_samples=gate_cells * wpc * hop,
                        carriers=[(off, kind, amp_q8, ph) for off, kind, ph in GATED_CARRIERS])
    u8 = pkg.iqgen_host(cfg, 0, 0, sv.samples_needed(dev, wpc * ncells))
    u8.setflags(write=False)
    return u8
