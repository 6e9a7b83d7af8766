"""Channel plans, captures and comparisons for stage 1 (convert x window -> FFT -> bin pick) away from the benchmark's plans:
hop 128 and 160, N = 512 / 1024 / 2048, the edge bins of the spectrum, 1 .. 64 live classes (bin mod 64) and 65 channels.
Shared by tests/test_oracle_stage1_plans.py (oracle against the float64 model, plan derivation; no GPU) and
tests/test_gpu_stage1_plans.py (HIP against the oracle bit for bit, and against the model).  Plain helpers, no pytest hooks.

Every channel gets squelch_threshold_dbfs = -1: no squelch opens, so stage 2 leaves the planes as stage 1 wrote them.
"""
import numpy as np

import libs
import signal_model as sm
from common import AGC_EXTRA, WAVE_BATCH, to_oracle_cfg

CENTRE = 120000000
RATES = (2048000, 2560000)  # hop 128 and hop 160
SIZES = (9, 10, 11)
CLASS_COUNTS = (8, 9, 16, 17, 32, 33)  # both sides of every threshold of Geo::round_windows (l64_kernel.h)
PLAN_NAMES = ["edges", "one"] + [f"classes{m}" for m in CLASS_COUNTS] + ["all64", "all64_iq", "over"]

# two calls of one batch each: windows 0 .. 2099, then 2100 .. 4099 -- whole tiles and a tail tile at all three sizes in the
# first call (2100 = 65 x 32 + 20 = 131 x 16 + 4 = 262 x 8 + 4), and the 100 carried entries between them
CALLS = (WAVE_BATCH + AGC_EXTRA, WAVE_BATCH)
NWIN = sum(CALLS)

# Oracle (float32, radix-2) against the float64 model, max-norm over the RMS of the model's planes of the case (every channel
# and compared window of it: the rounding error of an N-point float32 sum is absolute, set by the energy in the window and
# not by the bin it lands in).  Largest figure over RATES x SIZES x PLAN_NAMES and the s8 / s16 / f32 cases, as printed by
# tests/test_oracle_stage1_plans.py: 7.40e-7 (magnitudes, 2.56 MS/s, fft 1024, `over`: 7.392e-7; complex planes 6.38e-7, same
# case).  The figure grows with the share of noise-only channels in the RMS: 1.2e-7 .. 2.0e-7 for `one`, 2.1e-7 .. 3.8e-7
# for `edges` and its s8 / s16 / f32 variants.  The bound is 4 x the largest, the rule of signal_cases.IQ_BOUND: the factor
# covers the spread of float32 rounding from capture to capture.
STAGE1_MEASURED = 7.40e-7
STAGE1_BOUND = 4 * STAGE1_MEASURED

SFMT = {"u8": (sm.SFMT_U8, 127.5), "s8": (sm.SFMT_S8, 127.5), "s16": (sm.SFMT_S16, 32767.0), "f32": (sm.SFMT_F32, 1.0)}


# ------------------------------------------------------------------ bins and frequencies

def freqs_for_bins(rate, log2n, bins):
    """A frequency for every wanted bin: one Hz above the grid point, where ceil(x - 1) of the bin formula (config.cpp:669-670)
    lands on the bin itself; the upper half of the spectrum lies below the centre."""
    n = 1 << log2n
    sp = rate // n
    return [CENTRE + (b if b < n // 2 else b - n) * sp + 1 for b in bins]


def named_edges(rate, log2n):
    """The edge frequencies used verbatim and the bins they map to: (name, frequency, bin)."""
    n = 1 << log2n
    sp = rate // n
    return [("centre+1", CENTRE + 1, 0), ("centre+sp", CENTRE + sp, 0), ("centre", CENTRE, n - 1), ("centre-sp", CENTRE - sp, n - 2),
            ("centre+rate/2", CENTRE + rate // 2, n // 2 - 1), ("centre-rate/2", CENTRE - rate // 2, n // 2 - 1),
            ("centre-rate/2+1", CENTRE - rate // 2 + 1, n // 2)]


def class_bins(log2n, m):
    """m bins with m distinct classes (bin mod 64), the upper bits varied."""
    n = 1 << log2n
    return [k + 64 * ((7 * k) % (n // 64)) for k in range(m)]


def plan(name, rate, log2n):
    """(frequencies, modulations, the bins they are meant for) of a named list."""
    n = 1 << log2n
    if name == "edges":
        # 0 twice (two frequencies), N-1, N-2, N/2-1 twice (both ends of the band), N/2, N/2+1, a mid-band bin twice at one
        # frequency, the same class 64 bins up, and a third of that class in the other half of the spectrum
        mid = n // 8 + 5
        named = named_edges(rate, log2n)
        bins = [b for _, _, b in named] + [n // 2 + 1, mid, mid, mid + 64, mid + 64 + n // 2]
        freqs = [f for _, f, _ in named] + freqs_for_bins(rate, log2n, bins[len(named):])
    elif name == "one":
        bins = [3 * n // 8 + 11]
        freqs = freqs_for_bins(rate, log2n, bins)
        return freqs, [sm.MOD_NFM], bins
    elif name.startswith("classes"):
        bins = class_bins(log2n, int(name[len("classes"):]))
        freqs = freqs_for_bins(rate, log2n, bins)
    elif name in ("all64", "all64_iq"):
        bins = class_bins(log2n, 64)
        freqs = freqs_for_bins(rate, log2n, bins)
        if name == "all64_iq":
            return freqs, [sm.MOD_NFM] * 64, bins
    elif name == "over":
        bins = class_bins(log2n, 64) + [n // 2 + 100]
        freqs = freqs_for_bins(rate, log2n, bins)
    else:
        raise ValueError(name)
    return freqs, [sm.MOD_NFM if i % 2 else sm.MOD_AM for i in range(len(freqs))], bins


def live_classes(bins):
    return len({b % 64 for b in bins})


# the handle's options -> the MI_STAGE1_* kind its calls must report (0 / 1 exchange kernel full / pruned, 2 / 3 lane-resident
# full graph / compiled for the plan)
VARIANTS = {"default": {}, "prebuilt full graph": {"OPT_LANE_FFT_JIT": 0}, "exchange kernel": {"OPT_LANE_FFT": 0}}


def expected_kind(variant, name, log2n):
    """65 channels take the exchange kernel whatever is asked for.  The exchange kernel prunes at N = 512 where the packed
    passes are well under the full ones (plan.cpp: 8 x residues mod 8 + residues mod 64 <= 64): `edges` (5 and 5) and `one`
    (1 and 1) do, every list with eight or more classes has all eight residues mod 8 and does not."""
    if variant == "exchange kernel" or name == "over":
        return 1 if log2n == 9 and name in ("edges", "one") else 0
    return 3 if variant == "default" else 2


def device(mk, rate, log2n, sfmt="u8"):
    code, fullscale = SFMT[sfmt]
    return mk(sample_rate=rate, centerfreq=CENTRE, fft_size_log=log2n, sfmt=code, fullscale=fullscale)


def channels(mk, freqs, mods):
    """mk: the channel_cfg constructor of either binding (libs.channel_cfg / pkg.channel_cfg)."""
    return [mk(f, modulation=m, squelch_threshold_dbfs=-1) for f, m in zip(freqs, mods)]


def assert_bins(pkg, dev, chans, bins):
    """Every channel lands on the bin it was meant for, by the plan under test and by the model's restatement of the formula."""
    p = pkg.Plan(dev, chans)
    got = [int(p.channel(i).bin) for i in range(len(chans))]
    p.close()
    assert got == list(bins), f"plan bins {got}, meant {list(bins)}"
    n = 1 << dev.fft_size_log
    assert [sm.bin_index(c.freq, dev.centerfreq, dev.sample_rate, n) for c in chans] == list(bins)


# ------------------------------------------------------------------ captures

TONE_GAP = 16


def tone_freqs(rate, log2n, freqs):
    """Of the first eight channel frequencies, those that get a tone: each at least TONE_GAP bins (cyclically, by its true
    position on the grid) from every tone before it."""
    n = 1 << log2n
    out, at = [], []
    for f in freqs[:8]:
        b = ((f - CENTRE) * n / rate) % n
        if all(min(abs(b - a), n - abs(b - a)) >= TONE_GAP for a in at):
            out.append(f), at.append(b)
    return out


def capture(rate, log2n, freqs, seed=1, sfmt="u8"):
    """Seeded bytes for NWIN windows: Gaussian noise of 2 LSB and a tone on the first (up to eight) channel frequencies.
    Stage 1 is linear: nothing depends on the generator.  No squelch may open (stage 2 then rewrites raw-I/Q planes).  A tone
    of a LSB leaves a / 127.5 x sum(w) = 0.00213 a N in its bin, the -1 dBFS squelch level is 0.696 sqrt(N): 12 LSB reach
    it from N = 1024 on.  So the tone is 12 LSB or what puts it at half that level, whichever is less (7.2 / 5.1 / 3.6 LSB
    at N = 512 / 1024 / 2048, 40 x the noise in its bin and more), and since the window's main lobe is seven bins wide either
    way, a frequency whose bin lies within TONE_GAP bins of an earlier tone's gets none.  The wider formats are the same
    values widened (u8 0 is never produced, so s8 stays clear of -128, whose table entry the reference never writes)."""
    level = float(libs.oracle_lib().ao_dbfs_to_level(-1.0, 1 << log2n))
    amp = min(12.0, 0.5 * level * 127.5 / float(np.sum(sm.window(1 << log2n))))
    hop = sm.hop_of(rate)
    ns = NWIN * hop + (1 << log2n) + hop
    rng = np.random.default_rng([seed, rate, log2n])
    t = np.arange(ns, dtype=np.float64)
    x = rng.normal(0.0, 2.0, ns) + 1j * rng.normal(0.0, 2.0, ns)
    for f in tone_freqs(rate, log2n, freqs):
        x += amp * np.exp(2j * np.pi * (((f - CENTRE) / rate) * t + rng.uniform()))
    u8 = np.empty(2 * ns, np.uint8)
    u8[0::2] = np.clip(np.round(x.real + 127.5), 1, 255)
    u8[1::2] = np.clip(np.round(x.imag + 127.5), 1, 255)
    if sfmt == "u8":
        return u8
    v = u8.astype(np.float32) - 127.5
    raw = {"s8": lambda: np.round(v - 0.5).astype(np.int8), "s16": lambda: np.round(v * 200.0).astype(np.int16),
           "f32": lambda: (v / 128.0).astype(np.float32)}[sfmt]()
    return raw.view(np.uint8)


def subset_windows(seed=7):
    """Windows compared with the float64 model: the first and last 64 of each call, the first 64 that are still in the planes
    after the first call (its first AGC_EXTRA entries are overwritten by the carried ones), and 128 seeded random ones."""
    c0, c1 = CALLS
    w = list(range(64)) + list(range(AGC_EXTRA, AGC_EXTRA + 64)) + list(range(c0 - 64, c0)) + list(range(c0, c0 + 64)) + \
        list(range(NWIN - 64, NWIN))
    w += [int(v) for v in np.random.default_rng(seed).integers(0, NWIN, 128)]
    return np.array(sorted(set(w)))


def model_planes(dev, chans, raw, windows):
    """The float64 model's X[channel][k] for the windows `windows` (sorted), one DFT bin per channel as a dot product."""
    n = 1 << dev.fft_size_log
    x = sm.samples_from_bytes(raw, dev.sfmt, dev.fullscale)
    bins = [sm.bin_index(c.freq, dev.centerfreq, dev.sample_rate, n) for c in chans]
    uniq = sorted(set(bins))
    out = sm.channelize_windows(x, dev.sample_rate, n, uniq, windows)
    return np.stack([out[uniq.index(b)] for b in bins])


def oracle_planes(dev, chans, raw):
    """OracleDemod.stage1 over all NWIN windows: (mag [nch][NWIN], complex [nch][NWIN][2])."""
    odev, ochans = to_oracle_cfg(dev, chans)
    od = libs.OracleDemod(odev, ochans)
    mag, z = od.stage1(raw, NWIN)
    od.close()
    return mag, z


def residuals(model, mag, z, nfm):
    """(complex, magnitude) max-norm residual over the model's RMS.  model: [nch][k] complex; mag [nch][k]; z [nch][k][2], of
    which only the rows `nfm` (raw-I/Q channels: the others have no complex plane) are compared."""
    scale = sm.rms(model)
    assert scale > 0
    zc = z[..., 0].astype(np.float64) + 1j * z[..., 1].astype(np.float64)
    rows = [i for i, on in enumerate(nfm) if on]
    e_iq = float(np.max(np.abs(zc[rows] - model[rows]))) / scale if rows else 0.0
    e_mag = float(np.max(np.abs(mag.astype(np.float64) - np.abs(model)))) / scale
    return e_iq, e_mag, scale
