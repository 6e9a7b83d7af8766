"""The inputs and comparisons that tests/test_signal_model.py (oracle) and tests/test_gpu_signal_model.py (HIP library)
share: two channel sets (the nine plain rows, and eight rows for AM on the raw-I/Q path and the low-pass), gated synthetic
carriers, the residual of a backend's output against tests/signal_model.py, and the dBFS bracket around a steady carrier.

A backend is anything that turned the capture into (waveout [nch][n], axc [nch][nb], iq_out [nch][n][2], squelch levels
[nch]); both comparisons run the same code on it with the same bounds.

Timing of every case: the carriers are off for the first 16 000 windows (the squelch learns the noise) and on for the
next 16 000; 16 batches are run and the compared span is audio samples 27 900 .. 31 900, i.e. it ends before the carriers
do and begins 11 900 samples after they came on -- the slowest recursion of the chain (the Q = 10 notch at 100 Hz, pole
radius 0.99804: 0.99804^8000 = 1.6e-7) has forgotten how it started long before.
"""
import numpy as np

import signal_model as sm

WAVE_BATCH = 2000
CENTRE = 120000000
GATE_WINDOWS = 16000
NBATCHES = 16
SPAN = (27900, 31900)
OPEN_BEFORE = 8000  # the backend must have been open this long before the span (see above)
AUDIO_BOUND = 1e-4  # RMS, the project's stated audio bound (README)

# Raw I/Q bound, relative to the RMS of the model's I/Q over the span: 4 x the largest oracle-vs-model residual measured
# over every case below (DESIGN 3 lists them per case).
IQ_BOUND = 4 * 1.107e-7

# The same for a row behind the low-pass (bandwidth > 0), whose float32 recursion adds its own rounding: 4 x the largest
# oracle-vs-model residual over FILTERED_ROWS in every case tests/test_signal_model.py runs them at (2.288e-7, the NFM
# bandwidth = 12500 row at fft 1024 and 2.5 MS/s; DESIGN 3 lists them per case).
IQ_BOUND_FILTERED = 4 * 2.288e-7

AM_ON_GRID, AM_OFF_GRID, NFM_IQ, NFM_TONE, NFM_TONE_NOTCH, NFM_TONE_CTCSS_NOTCH, NFM_TAU75, NFM_TAU0, AM_LOUD = range(9)
ROW_NAMES = ["am_on_grid", "am_off_grid", "nfm_iq", "nfm_tone", "nfm_tone_notch", "nfm_tone_ctcss_notch", "nfm_tau75", "nfm_tau0",
             "am_ampfactor3"]

OFF_AM_ON, OFF_AM_OFF, OFF_NFM, OFF_NFM_TONE = 250000, -377300, 613700, -801900


def channels(mk):
    """mk: the channel_cfg constructor of either binding (libs.channel_cfg / pkg.channel_cfg)."""
    return [
        mk(CENTRE + OFF_AM_ON),                                               # on the bin grid at 2.56 MS/s: one bin down
        mk(CENTRE + OFF_AM_OFF),
        mk(CENTRE + OFF_NFM, modulation=1, has_iq_outputs=1),
        mk(CENTRE + OFF_NFM_TONE, modulation=1, has_iq_outputs=1),               # carrier with the 100 Hz tone, no notch
        mk(CENTRE + OFF_NFM_TONE, modulation=1, has_iq_outputs=1, notch=100.0),  # the same carrier through the notch
        mk(CENTRE + OFF_NFM_TONE, modulation=1, has_iq_outputs=1, notch=100.0, ctcss=100.0),  # is_open gated by the tone
        mk(CENTRE + OFF_NFM, modulation=1, has_iq_outputs=1, tau=75),
        mk(CENTRE + OFF_NFM, modulation=1, has_iq_outputs=1, tau=0),
        mk(CENTRE + OFF_AM_OFF, ampfactor=3.0),                               # 3 x m / 1.5 = 1.0: the clamp engages
    ]


# The second channel set: AM on the raw-I/Q path and the low-pass, on the same carriers.  An AM channel with a raw-I/Q output
# or with the bandwidth key present overwrites its magnitudes 100 steps late (tests/signal_model.py, time axes); a positive
# bandwidth puts the second-order Bessel low-pass at bandwidth / 2 behind the derotation.
F_AM_PLAIN, F_AM_IQ, F_AM_BW_KEY, F_AM_BW7000, F_AM_BW3000_IQ, F_AM_BW15000_LOUD, F_NFM_BW12500_IQ, F_NFM_BW5000_NOTCH = range(8)
FILTERED_ROW_NAMES = ["f_am_plain", "f_am_iq", "f_am_bw_key_only", "f_am_bw7000", "f_am_bw3000_iq", "f_am_bw15000_ampfactor3",
                      "f_nfm_bw12500_iq", "f_nfm_bw5000_notch_tau75_iq"]


def filtered_channels(mk):
    return [
        mk(CENTRE + OFF_AM_OFF),                                               # the companion the others are compared with
        mk(CENTRE + OFF_AM_OFF, has_iq_outputs=1),                             # the same audio 100 samples later
        mk(CENTRE + OFF_AM_OFF, bandwidth=-1),                                 # key present: raw-I/Q path, no filter, no output
        mk(CENTRE + OFF_AM_OFF, bandwidth=7000),                               # (8000: see below)
        mk(CENTRE + OFF_AM_OFF, bandwidth=3000, has_iq_outputs=1),             # cut-off 1.5 kHz: the 1 kHz tone is attenuated
        mk(CENTRE + OFF_AM_OFF, bandwidth=15000, ampfactor=3.0),               # the clamp, reached from filtered magnitudes
        mk(CENTRE + OFF_NFM, modulation=1, bandwidth=12500, has_iq_outputs=1),
        mk(CENTRE + OFF_NFM_TONE, modulation=1, bandwidth=5000, notch=100.0, tau=75, has_iq_outputs=1),
    ]


# Why 7000 and not 8000: at fft 512 (u8) the 8000 Hz rows' audio sample 28 279 is an exact 0.0 -- a zero crossing where the
# float32 magnitude equals the float32 average (neighbours -0.133 and +0.111, every batch flagged open) -- and assert_open()
# counts every exact zero as a closed squelch.  At 7000 Hz no sample of any case is zero; the span and the rule stay.
# Why 15000 on the ampfactor-3 row: 3 x m g / 1.5 only just reaches 1.0 (the plain row sits on the clamp for 64 of the span's
# 4 000 samples at fft 512), and a cut-off near the 1 kHz tone takes that away -- 20 samples at 8000 Hz, 3 at 7000, 58 at 15000,
# where check_row's "more than 50" holds as it does for the plain row.
ROW_SETS = {"plain": (channels, ROW_NAMES), "filtered": (filtered_channels, FILTERED_ROW_NAMES)}

CARRIERS = [(OFF_AM_ON, 0, 3072, 0), (OFF_AM_OFF, 0, 3072, 0), (OFF_NFM, 1, 3072, 0), (OFF_NFM_TONE, 2, 3072, 0)]

# name -> device keywords; every case runs the whole channel set
CASES = {
    "fft512": dict(fft_size_log=9),
    "fft512_quadri": dict(fft_size_log=9, fm_quadri=1),
    "fft512_s16": dict(fft_size_log=9, sfmt=sm.SFMT_S16, fullscale=32768.0),
    "fft2048": dict(fft_size_log=11),
    "fft2048_quadri": dict(fft_size_log=11, fm_quadri=1),
    "fft1024_2500k": dict(fft_size_log=10, sample_rate=2500000),
    "fft4096": dict(fft_size_log=12),
}


def capture(pkg, dev, nbatches=NBATCHES, seed=0x51C0DE):
    """u8 bytes from iqgen at its default noise level (s16: the same values widened), long enough for `nbatches`."""
    hop = sm.hop_of(dev.sample_rate)
    count = (nbatches * WAVE_BATCH + sm.AGC_EXTRA) * hop + (1 << dev.fft_size_log) + hop
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, seed=seed, gate_samples=GATE_WINDOWS * hop, carriers=CARRIERS)
    raw = pkg.iqgen_host(cfg, 0, 0, count)
    if dev.sfmt == sm.SFMT_S16:
        raw = (raw.astype(np.int16) * 256 - 32640).astype("<i2").view(np.uint8)
    return raw


class Backend:
    """What a backend made of a capture."""

    def __init__(self, name, waveout, axc, iq_out, squelch_levels, names=None):
        self.name = name
        self.names = ROW_NAMES if names is None else names
        self.waveout = np.asarray(waveout, dtype=np.float64)
        self.axc = np.asarray(axc)
        if iq_out is None:  # a plan with no raw-I/Q row
            iq_out = np.zeros(self.waveout.shape + (2,))
        self.iq = np.asarray(iq_out, dtype=np.float64).reshape(self.waveout.shape[0], -1, 2)
        self.iq = self.iq[..., 0] + 1j * self.iq[..., 1]
        self.levels = np.asarray(squelch_levels, dtype=np.float64)


def assert_open(be, row, chan, g0=SPAN[0] - OPEN_BEFORE, g1=SPAN[1]):
    """The backend's own output says the row was open for every sample g0 .. g1: every batch flagged, no sample the exact
    zero a closed squelch writes (audio; raw I/Q at the steps the audio belongs to)."""
    flags = be.axc[row, g0 // WAVE_BATCH:(g1 - 1) // WAVE_BATCH + 1]
    assert (flags == ord("*")).all(), f"{be.name} row {be.names[row]}: batch flags {bytes(flags)!r}: not open throughout"
    closed = be.waveout[row, g0:g1] == 0.0
    if chan.has_iq_outputs:
        closed = closed | (be.iq[row, g0 - sm.AGC_EXTRA:g1 - sm.AGC_EXTRA] == 0)
    assert not closed.any(), f"{be.name} row {be.names[row]}: {int(closed.sum())} closed samples in {g0}..{g1}, first at {g0 + int(np.argmax(closed))}"


class Model:
    """The channelizer's output of one case, computed once per (device, capture)."""

    def __init__(self, dev, chans, raw, span=SPAN, warmup=10000):
        self.dev, self.chans, self.span, self.warmup = dev, chans, span, warmup
        self.x = sm.samples_from_bytes(raw, dev.sfmt, dev.fullscale)
        n = 1 << dev.fft_size_log
        self.bins = [sm.bin_index(c.freq, dev.centerfreq, dev.sample_rate, n) for c in chans]
        self.w0 = span[0] - sm.AGC_EXTRA - warmup
        uniq = sorted(set(self.bins))
        X = sm.channelize(self.x, dev.sample_rate, n, uniq, self.w0, span[1] - self.w0)
        self.X = [X[uniq.index(b)] for b in self.bins]
        self._rows = {}

    def row(self, r, mode="as_specified", backend=None):
        """The model's output for row r; as_specified takes the accumulator's value at the head of the span from `backend`'s
        raw I/Q: from its first sample of the span on a row without a low-pass, from its first FIT_SAMPLES on one with."""
        c = self.chans[r]
        phase0 = None
        if mode == "as_specified" and sm.needs_raw_iq(c):
            s0 = self.span[0] - sm.AGC_EXTRA
            assert c.has_iq_outputs, "a row that emits no raw I/Q has nothing to take the accumulator from: compare it in exact mode"
            if sm.bandwidth_of(c) > 0:
                settle = 200
                phase0 = sm.accumulator_fit(self.X[r][self.warmup - settle:self.warmup + FIT_SAMPLES], backend.iq[r, s0:s0 + FIT_SAMPLES], c.freq,
                                            self.dev.centerfreq, self.dev.sample_rate, s0, sm.bandwidth_of(c) / 2.0, settle=settle)
            else:
                phase0 = sm.accumulator_at(self.X[r][self.warmup], backend.iq[r, s0], c.freq, self.dev.centerfreq, self.dev.sample_rate, s0)
        key = (r, mode, phase0)
        if key not in self._rows:  # (a model shared between tests computes a row once; nobody writes into the result)
            self._rows[key] = sm.model_channel(self.x, self.dev, c, self.span[0], self.span[1], mode=mode, warmup=self.warmup, phase0=phase0, X=self.X[r])
        return self._rows[key]


FIT_SAMPLES = 400  # raw-I/Q samples at the head of the span from which a low-passed row's accumulator is chosen


def mode_for(chan):
    """as_specified wherever the row emits the raw I/Q that names the accumulator.  An AM row on the raw-I/Q path with no such
    output (the bandwidth key alone) is compared with true sin / cos derotation: only the magnitude of its derotated sample is
    ever used, and that depends on the accumulator through the table's amplitude error alone -- a chord of the unit circle
    between two of 256 points is short of 1 by e = (2 pi / 256)^2 / 2 x t (1 - t), t the table fraction: at most 1 - cos(pi / 256)
    = 7.5e-5, mean 5.0e-5 (which the AGC's average takes out), standard deviation (2 pi / 256)^2 / 2 sqrt(1 / 180) = 2.2e-5.  The
    audio's 1 / 1.5 agc makes that 1.5e-5 RMS times the ampfactor -- 4.5e-5 at ampfactor 3, inside the 1e-4 RMS audio bound that
    applies to these rows like to any other (measured: 1.6e-5, 1.2e-5 behind a 3.5 kHz low-pass, 4.9e-5 at ampfactor 3)."""
    return "exact" if sm.needs_raw_iq(chan) and not chan.has_iq_outputs else "as_specified"


def iq_bound(chan):
    return IQ_BOUND_FILTERED if sm.bandwidth_of(chan) > 0 else IQ_BOUND


def residuals(model, be, row, mode=None):
    """(audio RMS residual, raw-I/Q residual relative to the model's I/Q RMS or None, the model's row)."""
    g0, g1 = model.span
    m = model.row(row, mode_for(model.chans[row]) if mode is None else mode, be)
    audio = sm.rms(be.waveout[row, g0:g1] - m["audio"])
    iq = None
    if m["iq"] is not None and model.chans[row].has_iq_outputs:
        iq = sm.rms(be.iq[row, g0 - sm.AGC_EXTRA:g1 - sm.AGC_EXTRA] - m["iq"]) / sm.rms(m["iq"])
    return audio, iq, m


def assert_am_above_level(model, be, row, m):
    """The model's AM average takes every sample; the backend's only those above the squelch level.  Twice the level must
    still lie below the smallest magnitude the model saw (warm-up included)."""
    lo = float(np.min(m["agc_mag"]))  # |X| of a plain row; the derotated, low-passed magnitudes of a row on the raw-I/Q path
    assert be.levels[row] > 0 and lo >= 2.0 * be.levels[row], \
        f"{be.name} row {be.names[row]}: smallest |X| {lo:.4g} against squelch level {be.levels[row]:.4g}: less than 2 x headroom"


# ------------------------------------------------------------------ dBFS: a manual threshold either side of a steady carrier

DBFS_BATCHES = 8
DBFS_OFFSET_HZ = 402700
DBFS_BRACKET_DB = 3.0


def dbfs_offset(n):
    """7.54 + 10 log10(N / 2) - 2.38: what the reference adds to 20 log10(level / N)."""
    return 7.54 + 10.0 * np.log10(n / 2.0) - 2.38


def dbfs_to_level(db, n):
    return 10.0 ** ((db - dbfs_offset(n)) / 20.0) * n


def dbfs_capture(dev, seed=0xDBF5):
    """u8 bytes made here (iqgen has no unmodulated carrier): Gaussian noise of 2 LSB and a 6-LSB carrier (about -8.7 dBFS at fft 512) at DBFS_OFFSET_HZ
    that is off for the first half of DBFS_BATCHES batches and on for the second."""
    hop = sm.hop_of(dev.sample_rate)
    count = (DBFS_BATCHES * WAVE_BATCH + sm.AGC_EXTRA) * hop + (1 << dev.fft_size_log) + hop
    rng = np.random.default_rng(seed)
    t = np.arange(count, dtype=np.float64)
    on = t >= (DBFS_BATCHES // 2) * WAVE_BATCH * hop
    z = 6.0 * on * np.exp(2j * np.pi * DBFS_OFFSET_HZ * t / dev.sample_rate)
    v = np.stack([z.real + rng.normal(0.0, 2.0, count), z.imag + rng.normal(0.0, 2.0, count)], axis=1)
    return np.clip(np.rint(127.5 + v), 0, 255).astype(np.uint8).reshape(-1)


def dbfs_bracket(mk, dev, raw):
    """Two plain AM channels on the carrier, thresholds (whole dBFS) at least DBFS_BRACKET_DB under and over the carrier's
    level as the float64 channelizer measures it over the last two batches; returns (channels, carrier dBFS, (under, over))."""
    n = 1 << dev.fft_size_log
    f = CENTRE + DBFS_OFFSET_HZ
    x = sm.samples_from_bytes(raw, dev.sfmt, dev.fullscale)
    first = (DBFS_BATCHES - 2) * WAVE_BATCH
    mag = np.abs(sm.channelize(x, dev.sample_rate, n, [sm.bin_index(f, dev.centerfreq, dev.sample_rate, n)], first, 2 * WAVE_BATCH)[0])
    noise = np.abs(sm.channelize(x, dev.sample_rate, n, [sm.bin_index(f, dev.centerfreq, dev.sample_rate, n)], 0, 2 * WAVE_BATCH)[0])
    db = 20.0 * np.log10(float(np.mean(mag)) / n) + dbfs_offset(n)
    under, over = int(np.floor(db - DBFS_BRACKET_DB)), int(np.ceil(db + DBFS_BRACKET_DB))
    # the bracket clears the carrier's own scatter and the noise: every magnitude of the carrier lies above the lower
    # level and below the upper one, every magnitude of the noise below the lower one
    assert mag.min() > dbfs_to_level(under, n) and mag.max() < dbfs_to_level(over, n) and noise.max() < dbfs_to_level(under, n)
    assert -100 <= under < over < 0
    return [mk(f, squelch_threshold_dbfs=under), mk(f, squelch_threshold_dbfs=over)], db, (under, over)


def assert_dbfs_bracket(be):
    """Row 0 (threshold under the carrier) is open for the whole second half of the carrier's time; row 1 never opens."""
    n = DBFS_BATCHES * WAVE_BATCH
    half = n * 3 // 4
    print(f"{be.name}: flags {bytes(be.axc[0])!r} / {bytes(be.axc[1])!r}")
    assert (be.axc[0, half // WAVE_BATCH:] == ord("*")).all() and not (be.waveout[0, half:n] == 0.0).any(), f"{be.name}: threshold under the carrier, not open throughout its second half"
    # (audio sample g judges window g + 100: the batch before the carrier's first window sees its first 100 windows)
    assert (be.axc[0, :DBFS_BATCHES // 2 - 1] == ord(" ")).all(), f"{be.name}: open on noise alone"
    assert (be.axc[1] == ord(" ")).all() and not be.waveout[1, sm.AGC_EXTRA:n].any(), f"{be.name}: threshold over the carrier, yet it opened"
