"""The inputs and comparisons that tests/test_signal_model.py (oracle) and tests/test_gpu_signal_model.py (HIP library)
share: one channel set, gated synthetic carriers, and the residual of a backend's output against tests/signal_model.py.

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

    def row(self, r, mode="as_specified", backend=None):
        """The model's output for row r; as_specified takes the accumulator's value at the head of the span from `backend`."""
        c = self.chans[r]
        phase0 = None
        if mode == "as_specified" and (c.modulation == sm.MOD_NFM or c.has_iq_outputs):
            s0 = self.span[0] - sm.AGC_EXTRA
            phase0 = sm.accumulator_at(self.X[r][self.warmup], backend.iq[r, s0], c.freq, self.dev.centerfreq, self.dev.sample_rate, s0)
        return sm.model_channel(self.x, self.dev, c, self.span[0], self.span[1], mode=mode, warmup=self.warmup, phase0=phase0, X=self.X[r])


def residuals(model, be, row, mode="as_specified"):
    """(audio RMS residual, raw-I/Q residual relative to the model's I/Q RMS or None, the model's row)."""
    g0, g1 = model.span
    m = model.row(row, mode, be)
    audio = sm.rms(be.waveout[row, g0:g1] - m["audio"])
    iq = None
    if m["iq"] is not None and model.chans[row].has_iq_outputs:
        iq = sm.rms(be.iq[row, g0 - sm.AGC_EXTRA:g1 - sm.AGC_EXTRA] - m["iq"]) / sm.rms(m["iq"])
    return audio, iq, m


def assert_am_above_level(model, be, row, m):
    """The model's AM average takes every sample; the backend's only those above the squelch level.  Twice the level must
    still lie below the smallest magnitude the model saw (warm-up included)."""
    lo = float(np.min(np.abs(model.X[row])))
    assert be.levels[row] > 0 and lo >= 2.0 * be.levels[row], \
        f"{be.name} row {be.names[row]}: smallest |X| {lo:.4g} against squelch level {be.levels[row]:.4g}: less than 2 x headroom"
