"""The random plans and captures of the fuzzers as functions of the seed, shared by tools/fuzz_oracle.py, tools/fuzz_tp.py and
tests/test_bench_geometry.py, so that the tools and the suite cannot diverge.  Nothing here touches the GPU: a plan is a device
configuration, a channel list and a host capture (mi_iqgen_host)."""
import numpy as np

from common import bytes_for_batches

CENTRE = 120000000
MIXED_FFT_LOGS = [8, 9, 10, 11]
MIXED_NBAT = 8
TP_NBAT = 16


def is_plain_am(pkg, ch):
    """The rows the time-parallel path can take (mi_demod_create): AM without low-pass, notch, CTCSS or raw I/Q."""
    return (ch.modulation == pkg.MOD_AM and ch.bandwidth == 0 and ch.notch_freq == 0 and ch.ctcss_freq == 0 and not ch.has_iq_outputs
            and ch.afc == 0)


def mixed_plan(pkg, seed):
    """Every channel type (AM / NFM, low-pass, notch, CTCSS, manual / SNR thresholds, amplification, raw I/Q), odd thresholds,
    carriers from under the squelch level to clipping, 3 .. 19 channels, fft 256 .. 2048.
    Returns (dev, chans, iq, nbat, per_call): the capture holds `nbat` batches, the tool feeds it `per_call` batches a call."""
    rng = np.random.default_rng(10000 + seed)
    centre = CENTRE
    nchan = int(rng.integers(3, 20))
    chans, carriers = [], []
    for k in range(nchan):
        f = centre - 1200000 + 40000 + k * 120000 + int(rng.integers(0, 20)) * 5000
        kw = {}
        nfm = rng.random() < 0.5
        if nfm:
            kw["modulation"] = pkg.MOD_NFM
        if rng.random() < 0.5:
            kw["bandwidth"] = int(rng.choice([5000, 8000, 12500]))
        if rng.random() < 0.25:
            kw["notch"] = float(rng.choice([100.0, 400.0, 1000.0]))
        if nfm and rng.random() < 0.4:
            kw["ctcss"] = float(rng.choice([100.0, 123.0, 151.4]))
        r = rng.random()
        if r < 0.2:
            kw["squelch_threshold_dbfs"] = int(rng.integers(-55, -30))
        elif r < 0.5:
            kw["squelch_snr_db"] = float(rng.choice([0.0, 3.0, 6.0, 12.0]))
        if rng.random() < 0.3:
            kw["ampfactor"] = float(rng.choice([0.5, 2.0, 4.0]))
        if rng.random() < 0.3:
            kw["has_iq_outputs"] = 1
        chans.append(pkg.channel_cfg(f, **kw))
        if rng.random() < 0.8:
            carriers.append((f - centre, int(rng.integers(0, 3)), int(rng.choice([150, 300, 600, 1200, 2500, 5000])), int(rng.integers(0, 1000))))
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=int(rng.choice(MIXED_FFT_LOGS)), fm_quadri=int(seed % 2))
    nbat, per_call = MIXED_NBAT, int(rng.choice([1, 2, 4, 8]))
    n = bytes_for_batches(dev, nbat) // 2
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, seed=20000 + seed, gate_samples=dev.sample_rate // int(rng.integers(3, 9)), carriers=carriers)
    iq = pkg.iqgen_host(cfg, 0, 0, n)
    return dev, chans, iq, nbat, per_call


def tp_plan(pkg, seed):
    """Plain-AM plans of 2 .. 11 channels (SNR / manual thresholds, amplification), carriers from under the squelch level to
    clipping, random gate periods and phases, fft 256 .. 1024.  Returns (dev, chans, iq, nbat)."""
    rng = np.random.default_rng(seed)
    centre = CENTRE
    nchan = int(rng.integers(2, 12))
    chans, carriers = [], []
    for k in range(nchan):
        f = centre - 1200000 + 60000 + k * 200000 + int(rng.integers(0, 20)) * 5000
        kw = {}
        r = rng.random()
        if r < 0.25:
            kw["squelch_threshold_dbfs"] = int(rng.integers(-55, -30))
        elif r < 0.6:
            kw["squelch_snr_db"] = float(rng.choice([0.0, 1.0, 3.0, 6.0, 12.0]))
        if rng.random() < 0.3:
            kw["ampfactor"] = float(rng.choice([0.5, 2.0, 4.0]))
        chans.append(pkg.channel_cfg(f, **kw))
        if rng.random() < 0.8:
            carriers.append((f - centre, 0, int(rng.choice([120, 250, 500, 1000, 2500, 6000])), int(rng.integers(0, 1000))))
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=int(rng.choice([8, 9, 10])))
    nbat = TP_NBAT
    n = bytes_for_batches(dev, nbat) // 2
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, seed=5000 + seed, gate_samples=dev.sample_rate // int(rng.integers(2, 12)), carriers=carriers)
    iq = pkg.iqgen_host(cfg, 0, 0, n)
    return dev, chans, iq, nbat


def tp_call_sizes(seed):
    """Device-call sizes of the overlapped reading of a tp_plan capture: every call has at least 8 batches."""
    return [[8, 8], [16], [8, 8], [8, 8]][seed % 4]
