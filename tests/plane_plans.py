"""Channel plans over the planes of plane_cases.py, and their oracle results: shared by tests/test_oracle_planes.py (CPU: the
generators do their job, the plane entry of the oracle is the IQ entry) and tests/test_gpu_planes.py (the HIP stage 2 equals it).

A plan is (dev, chans, rows, mag[rows][count], cplx or None); a row is (family or raw-I/Q kind, seed, settings).  Everything is
computed once per process and must be left unchanged by its users."""
import functools

import numpy as np

import libs
import plane_cases as pc
from plane_cases import AGC_EXTRA, WAVE_BATCH

CENTRE = 120000000
MANUAL_DBFS = -30

# squelch settings a row can have: keyword arguments of channel_cfg
SETTINGS = {"default": {}, "snr0": {"squelch_snr_db": 0.0}, "snr1": {"squelch_snr_db": 1.0}, "snr14": {"squelch_snr_db": 14.0},
            "manual": {"squelch_threshold_dbfs": MANUAL_DBFS}, "amp3": {"ampfactor": 3.0},
            # a manual level of 3e-20, three times the floor of the scaled dynamic_range rows
            "manual415": {"squelch_threshold_dbfs": -415}}
BASIC_SETTINGS = ("default", "snr0", "snr1", "snr14", "manual", "amp3")  # what the 16- and the 96-row plan vary per row

# the plain AM plan of 16 rows: one family x seed per channel, squelch settings varied per row
AM16 = [("edges_on_boundaries", 0, "default"), ("edges_on_boundaries", 1, "snr1"), ("threshold_grazers", 0, "default"),
        ("threshold_grazers", 1, "snr0"), ("threshold_grazers", 2, "snr1"), ("threshold_grazers", 3, "snr14"),
        ("threshold_grazers", 4, "manual"), ("flap_and_recover", 0, "default"), ("flap_and_recover", 1, "amp3"),
        ("regime_breakers", 0, "default"), ("regime_breakers", 1, "manual"), ("noise_staircase", 0, "default"),
        ("noise_staircase", 1, "snr0"), ("random_walk", 0, "default"), ("random_walk", 1, "snr14"), ("edges_on_boundaries", 2, "manual")]
DYNAMIC_RANGE = [("dynamic_range", s, "manual415" if s % 3 == 1 else ("default", "snr0")[s // 3 % 2]) for s in range(6)]
SILENCE = [("silence", s, ("default", "snr0", "manual", "default")[(s // 4 + s) % 4]) for s in range(8)]


def am96():
    """3 streams x 32 plain AM channels, every row a different plane: all families, random_walk with seeds 0 .. 7.  The streams of a
    handle share the channel plan, so a row's squelch settings are those of its channel (row % 32)."""
    fams = ["edges_on_boundaries", "threshold_grazers", "flap_and_recover", "regime_breakers", "noise_staircase", "dynamic_range", "silence"]
    names = list(BASIC_SETTINGS)
    rows, k = [], 0
    for r in range(96):
        setting = names[(r % 32) % len(names)]
        if r < 8:
            rows.append(("random_walk", r, setting))
            continue
        # (a threshold at the floor opens on the jitter alone: such a row never rests for recent_sample_size steps, and behind a
        #  saturated stretch it stays open for good -- those two families go with the other settings)
        while (fams[k % len(fams)] == "flap_and_recover" and setting in ("snr0", "snr1")) or (fams[k % len(fams)] == "regime_breakers" and setting == "snr0"):
            k += 1
        seed = 10 + r
        if fams[k % len(fams)] == "dynamic_range" and seed % 3 == 1:
            seed += 1  # (the rows scaled to a floor of 1e-20 need a manual threshold down there: they are in the plan of their own)
        rows.append((fams[k % len(fams)], seed, setting))
        k += 1
    return rows


def manual_level(dbfs=MANUAL_DBFS, fft_size=512):
    return float(libs.oracle_lib().ao_dbfs_to_level(float(dbfs), fft_size))


def squelch_kw(setting):
    """The keyword arguments of ComponentAPI.squelch_run / oracle_core_trace for a row's settings."""
    kw = SETTINGS[setting]
    out = {}
    if "squelch_threshold_dbfs" in kw:
        out["manual_level"] = manual_level(kw["squelch_threshold_dbfs"])
    if "squelch_snr_db" in kw:
        out["snr_db"] = kw["squelch_snr_db"]
    return out


def floor_of(setting):
    return 0.1 if setting == "manual" else 1.0  # a manual threshold of -30 dBFS is a level of 0.56: the quiet floor sits under it


@functools.lru_cache(maxsize=None)
def am_row(family, seed, setting, nsteps, L):
    kw = {}
    if family in ("edges_on_boundaries", "threshold_grazers", "flap_and_recover", "regime_breakers"):
        kw["floor"] = floor_of(setting)
    if family == "threshold_grazers":
        # the level the squelch compares against after a quiet part, from the oracle's own trace of the row so far
        kw["threshold_of"] = lambda quiet: libs.oracle().squelch_run(quiet, **squelch_kw(setting))["level"][-1]
    plane = pc.FAMILIES[family](seed, nsteps, L, **kw)
    plane.setflags(write=False)
    return plane


def am_chans(cfg, rows):
    """channel_cfg of one stream's rows (cfg: libs.channel_cfg or the package's)."""
    n = len(rows)
    return [cfg(CENTRE + 12500 + 25000 * (i - n // 2), **SETTINGS[setting]) for i, (_, _, setting) in enumerate(rows)]


@functools.lru_cache(maxsize=None)
def am_planes(name, nbatches, L):
    rows = {"am16": AM16, "dynamic_range": DYNAMIC_RANGE, "silence": SILENCE}[name] if name != "am96" else am96()
    mag = np.stack([am_row(f, s, st, nbatches * WAVE_BATCH, L) for f, s, st in rows])
    mag.setflags(write=False)
    return tuple(rows), mag


# ---- the mixed plan: rows with raw I/Q beside plain AM rows
def mixed_chans(cfg, MOD_NFM=1):
    """The channel kinds of test_manual_squelch_and_options, a CTCSS + notch row, two low-pass rows without derotation (their frequency
    offset is a multiple of WAVE_RATE * 10: dm_dphi = 0, so +-7 kHz in the plane is +-7 kHz at the filter) and two plain AM rows."""
    c = CENTRE
    return [cfg(c + 250000, squelch_threshold_dbfs=-40),
            cfg(c - 250000, squelch_snr_db=0.0, ampfactor=2.5),
            cfg(c + 500000, modulation=MOD_NFM, tau=0, notch=1000.0, notch_q=5.0),
            cfg(c - 500000, bandwidth=8000, has_iq_outputs=1),
            cfg(c + 750000, modulation=MOD_NFM, ctcss=100.0, bandwidth=12500),
            cfg(c - 750000, modulation=MOD_NFM, ctcss=100.0, notch=100.0, has_iq_outputs=1),
            cfg(c + 160000, bandwidth=5000, has_iq_outputs=1),
            cfg(c - 320000, bandwidth=5000, squelch_snr_db=6.0),
            cfg(c + 100000),
            cfg(c - 100000, squelch_snr_db=1.0)]


# per channel of mixed_chans: the plain AM family, or the raw-I/Q kind, and a seed
MIXED_ROWS = [("am", "flap_and_recover", 20), ("am", "threshold_grazers", 21), ("iq", "nfm", 0), ("iq", "notch", 1), ("iq", "ctcss", 2),
              ("iq", "ctcss", 3), ("iq", "lowpass_outside", 4), ("iq", "lowpass_inside", 5), ("am", "edges_on_boundaries", 22),
              ("am", "random_walk", 23)]
MIXED_LOWPASS = (6, 7)
MIXED_CTCSS = (4, 5)


@functools.lru_cache(maxsize=None)
def mixed_planes(nbatches):
    """(mag[10][count], cplx[6][count][2]): cplx holds the rows of the channels with needs_raw_iq, in channel order."""
    nsteps = nbatches * WAVE_BATCH
    mags, cplx = [], []
    for ch, (what, kind, seed) in enumerate(MIXED_ROWS):
        if what == "iq":
            m, z = pc.raw_iq_row(kind, seed, nsteps, 512, scale=(1.0, 1e15, 1e-3)[seed % 3] if kind in ("nfm", "notch") else 1.0)
            mags.append(m), cplx.append(z)
        elif kind == "threshold_grazers":
            lvl = lambda quiet: libs.oracle().squelch_run(quiet, snr_db=0.0)["level"][-1]
            mags.append(pc.threshold_grazers(seed, nsteps, 512, threshold_of=lvl))
        else:
            mags.append(pc.FAMILIES[kind](seed, nsteps, 512, **({"floor": 0.02} if ch == 0 else {})))  # (-40 dBFS is a level of 0.18)
    mag, cplx = np.stack(mags), np.stack(cplx)
    mag.setflags(write=False), cplx.setflags(write=False)
    return mag, cplx


# ---- the oracle over a plan, call by call
class CallResult:
    """What one call leaves: audio [rows][n], lookahead [rows][AGC_EXTRA], flags [rows][nb], raw I/Q [rows][2n] or None, stats."""

    def __init__(self, wo, look, axc, iqo, stats):
        self.wo, self.look, self.axc, self.iqo, self.stats = wo, look, axc, iqo, stats


def oracle_calls(dev, chans, mag, cplx, calls, want_iq=False, trace=False):
    """ao_demod_run_planes over `calls` = (nbatches, ...) consecutive calls: a CallResult per call, and the per-step trace
    [rows][steps] of the whole run if asked for.  chans: one libs.ChannelCfg per row of mag."""
    od = libs.OracleDemod(dev, list(chans))
    if trace:
        od.trace_start(sum(calls) * WAVE_BATCH)
    out, at = [], 0
    for k in calls:
        count = k * WAVE_BATCH + (AGC_EXTRA if at == 0 else 0)
        nb, wo, axc, iqo = od.run_planes(mag[:, at:at + count], k, cplx=None if cplx is None else cplx[:, at:at + count], want_iq=want_iq)
        assert nb == k
        out.append(CallResult(wo, od.lookahead(), axc, iqo, od.channel_stats()))
        at += count
    tr = od.trace() if trace else None
    od.close()
    return out, tr


def state_of(trace):
    return (trace >> libs.TRACE_STATE_SHIFT) & 7


def decisions(trace_row):
    """open and close decisions along one row of a trace: the rising and the falling edges of its open mask"""
    o = (trace_row & libs.TRACE_OPEN) != 0
    return int(np.count_nonzero(o[1:] != o[:-1]))
