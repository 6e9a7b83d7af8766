"""A float64 signal model of the demodulate() chain, written from signal theory and the reference's formulas.

It is the anchor the oracle (`oracle/airband_oracle.c`) and the HIP library are both compared with
(`tests/test_signal_model.py`, `tests/test_gpu_signal_model.py`).  numpy only; it calls neither of them nor
the host plan for any arithmetic, and it has no squelch: the caller names a span of output samples over which
the squelch under test is open throughout (and has been for `warmup` samples before), and asserts that on the
backend's own output.

Time axes (all at WAVE_RATE = 16 kHz):
  window w     the channelizer's w-th FFT: input samples [w*hop, w*hop + N), hop = round(rate / 16000)
  audio g      AM:  (|X_{g-100}| - agc_g) / (1.5 agc_g), agc running over |X_g|   (the AGC looks 100 windows ahead)
               AM on the raw-I/Q path (has_iq_outputs, or the bandwidth key present): step g derotates (and low-passes)
                    window g-100 into z_{g-100} and stores its magnitude where |X_g| stood, so the sequence the AGC and
                    the numerator read is m[g] = |z_{g-100}|: (m[g-100] - agc_g) / (1.5 agc_g) with agc running over m[g],
                    i.e. the numerator is window g-200 and the average looks at window g-100 -- the plain channel's audio
                    100 samples later, from filtered magnitudes when a low-pass is configured
               NFM: the discriminator of windows g-100 and g-101 (of the low-passed samples when bandwidth > 0)
  raw I/Q s    the derotated (bandwidth > 0: and low-passed) window s; the audio sample that belongs to it is g = s + 100

Two modes for everything that touches an angle:
  exact         true sin / cos / atan2, derotation by the true phase advance 2 pi f hop / rate per window
  as_specified  the reference's approximations evaluated in float64: 24-bit phase accumulator with the truncated
                increment, 256-entry linearly interpolated sin/cos table, the fast-atan2 rational, the
                quadrature formula
"""
import math

import numpy as np

WAVE_RATE = 16000
AGC_EXTRA = 100
MOD_AM, MOD_NFM = 0, 1
SFMT_U8, SFMT_S8, SFMT_S16, SFMT_F32 = 1, 2, 3, 4
PHASE_ONE = 1 << 24

# "Blackman 7": the seven-term cosine-sum window, denominator N - 1
BLACKMAN7 = (0.27105140069342, 0.43329793923448, 0.21812299954311, 0.06592544638803, 0.01081174209837, 0.00077658482522,
             0.00001388721735)


# ------------------------------------------------------------------ stage 1

def hop_of(sample_rate):
    """Input samples between two windows; half-way cases away from zero like C's round()."""
    return int(math.floor(sample_rate / WAVE_RATE + 0.5))


def window(n):
    i = np.arange(n, dtype=np.float64)
    w = np.zeros(n)
    for k, a in enumerate(BLACKMAN7):
        w += (-1) ** k * a * np.cos(2.0 * np.pi * k * i / (n - 1))
    return w


def bin_index(freq, centerfreq, sample_rate, n):
    """The channel's FFT bin: ceil((f + rate - centre) / spacing - 1) mod N with the *integer* spacing rate // N.
    A frequency exactly on the grid therefore lands one bin below its own."""
    spacing = sample_rate // n
    return int(math.ceil((freq + sample_rate - centerfreq) / float(spacing) - 1.0)) % n


def samples_from_bytes(raw, sfmt, fullscale=127.5):
    """Interleaved I/Q bytes -> complex128 samples in [-1, 1)."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    if sfmt == SFMT_U8:
        v = (raw.astype(np.float64) - 127.5) / 127.5
    elif sfmt == SFMT_S8:
        v = raw.view(np.int8).astype(np.float64) / 128.0
    elif sfmt == SFMT_S16:
        v = raw.view(np.int16).astype(np.float64) / float(fullscale)
    elif sfmt == SFMT_F32:
        v = raw.view(np.float32).astype(np.float64) / float(fullscale)
    else:
        raise ValueError(f"sample format {sfmt}")
    return v[0::2] + 1j * v[1::2]


def dft_basis(n, bins):
    """w[m] e^{-2 pi j b m / N} for every bin b: [N][len(bins)]."""
    m = np.arange(n, dtype=np.float64)
    return np.stack([window(n) * np.exp(-2j * np.pi * ((int(b) * m) % n) / n) for b in bins], axis=1)


def channelize_windows(x, sample_rate, n, bins, windows):
    """channelize() for a list of windows that need not be consecutive: X[c][k] of window windows[k]."""
    hop = hop_of(sample_rate)
    x = np.asarray(x, dtype=np.complex128)
    windows = np.asarray(windows, dtype=np.int64)
    if windows.min() < 0 or windows.max() * hop + n > x.size:
        raise ValueError("windows outside the capture")
    frames = x[windows[:, None] * hop + np.arange(n)[None, :]]
    return (frames @ dft_basis(n, bins)).T


def channelize(x, sample_rate, n, bins, first, count, chunk=1024):
    """X[c][i] = sum_m x[(first + i) hop + m] w[m] e^{-2 pi j bins[c] m / N}: one DFT bin per channel as a dot product."""
    hop = hop_of(sample_rate)
    x = np.asarray(x, dtype=np.complex128)
    if first < 0 or (first + count - 1) * hop + n > x.size:
        raise ValueError("windows outside the capture")
    basis = dft_basis(n, bins)
    out = np.zeros((len(bins), count), np.complex128)
    for c0 in range(0, count, chunk):
        c1 = min(count, c0 + chunk)
        seg = x[(first + c0) * hop:(first + c1 - 1) * hop + n]
        frames = np.lib.stride_tricks.as_strided(seg, shape=(c1 - c0, n), strides=(hop * seg.strides[0], seg.strides[0]), writeable=False)
        out[:, c0:c1] = (frames @ basis).T
    return out


def window_dtft(n, sample_rate, offset_hz):
    """W(nu) = sum_m w[m] e^{-2 pi j nu m / rate}.  A unit tone `nu` above the bin centre leaves conj(W(nu)) in the bin; the
    window is symmetric, so W(nu) = e^{-j pi nu (N-1) / rate} times a real gain -- |W| is the sideband gain."""
    m = np.arange(n, dtype=np.float64)
    return complex(np.sum(window(n) * np.exp(-2j * np.pi * offset_hz * m / sample_rate)))


# ------------------------------------------------------------------ AM

def clamp(x, ampfactor):
    return np.clip(np.asarray(x, dtype=np.float64) * ampfactor, -1.0, 1.0)


def am_audio(mag, ampfactor=1.0):
    """mag: |X_w| for w = w0 .. w0 + len.  Returns the audio of g = w0 + 100 .. w0 + len, before and after ampfactor / clamp.
    The slow average takes every sample (the model assumes |X_g| is above the squelch level throughout)."""
    mag = np.asarray(mag, dtype=np.float64)
    out = np.zeros(mag.size - AGC_EXTRA)
    agc = float(np.mean(mag[:AGC_EXTRA]))
    for i in range(out.size):
        g = i + AGC_EXTRA
        agc = 0.995 * agc + 0.005 * mag[g]
        v = (mag[g - AGC_EXTRA] - agc) / (1.5 * agc)
        if abs(v) > 0.8:
            v *= 0.85
            agc *= 1.15
        out[i] = v
    return out, clamp(out, ampfactor)


# ------------------------------------------------------------------ derotation

def phase_advance_exact(freq, centerfreq, sample_rate):
    """Radians by which a carrier at `freq` turns from one window to the next."""
    return 2.0 * np.pi * (freq - centerfreq) * hop_of(sample_rate) / sample_rate


def dm_dphi(freq, centerfreq, sample_rate, with_correction=True):
    """The reference's 24-bit phase increment: the offset in turns per output sample, less the share the rounded hop does
    not make ((rate/16000 - hop) * offset / rate turns ... written as in the reference: 8000 * frac * offset / (rate / 2) Hz),
    fraction kept, scaled by 2^24 and truncated toward zero; negative values wrap into 24 bits when added."""
    off = float(freq - centerfreq)
    dec = sample_rate / float(WAVE_RATE)
    corr = (WAVE_RATE / 2.0) * (dec - math.floor(dec + 0.5)) * off / (sample_rate / 2.0) if with_correction else 0.0
    turns = (off - corr) / WAVE_RATE
    turns -= math.trunc(turns)
    return int(turns * PHASE_ONE) % (1 << 32)


_LUT_ANGLE = 2.0 * np.pi * np.arange(257) / 256.0
_LUT_SIN, _LUT_COS = np.sin(_LUT_ANGLE), np.cos(_LUT_ANGLE)
_LUT_SIN[256], _LUT_COS[256] = _LUT_SIN[0], _LUT_COS[0]


def sincos_lut(phase24):
    """256-entry table, linear interpolation on the low 16 bits of a 24-bit phase."""
    p = np.asarray(phase24, dtype=np.int64) & (PHASE_ONE - 1)
    idx = p >> 16
    fr = (p & 0xffff) / 65536.0
    s = _LUT_SIN[idx] + (_LUT_SIN[idx + 1] - _LUT_SIN[idx]) * fr
    c = _LUT_COS[idx] + (_LUT_COS[idx + 1] - _LUT_COS[idx]) * fr
    return s, c


def derotate(X, freq, centerfreq, sample_rate, mode, first_window=0, phase0=0):
    """X: windows first_window ..; exact: times e^{-j advance w}; as_specified: times (cos - j sin) of the table at the
    accumulator phase0 + i * dm_dphi (mod 2^24), phase0 being the accumulator at X[0]."""
    X = np.asarray(X, dtype=np.complex128)
    i = np.arange(X.size, dtype=np.int64)
    if mode == "exact":
        return X * np.exp(-1j * phase_advance_exact(freq, centerfreq, sample_rate) * (i + first_window))
    if mode != "as_specified":
        raise ValueError(mode)
    s, c = sincos_lut(int(phase0) + i * (dm_dphi(freq, centerfreq, sample_rate) & (PHASE_ONE - 1)))
    return X * (c - 1j * s)


# ------------------------------------------------------------------ NFM

def fast_atan2(y, x):
    """pi/4 - pi/4 (x - |y|) / (x + |y|) for x >= 0, 3 pi/4 - pi/4 (x + |y|) / (|y| - x) otherwise, with the sign of y."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    ya = np.abs(y)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(x >= 0, np.pi / 4 - np.pi / 4 * (x - ya) / (x + ya), 3 * np.pi / 4 - np.pi / 4 * (x + ya) / (ya - x))
    a = np.where((x == 0) & (y == 0), 0.0, a)
    return np.where(y < 0, -a, a)


def discriminator(z, mode, quadri=False):
    """d[i] for i >= 1: the turn of z[i] against z[i-1] in units of pi."""
    z = np.asarray(z, dtype=np.complex128)
    a, b = z[1:], z[:-1]
    if mode == "exact":
        return np.angle(a * np.conj(b)) / np.pi
    if quadri:
        return (b.real * a.imag - a.real * b.imag) / (a.real * a.real + a.imag * a.imag + 1.0) / np.pi
    c = a * np.conj(b)
    return fast_atan2(c.imag, c.real) / np.pi


# ------------------------------------------------------------------ low-pass (bandwidth > 0)

BESSEL2_POLE = complex(-1.10160133059, 0.636009824757)  # second-order Bessel, -3 dB at unit frequency


def lowpass_coeffs(freq, rate=WAVE_RATE):
    """(gain, c0, c1) of the second-order Bessel low-pass at cut-off `freq`: pre-warped alpha = tan(pi f / rate) / pi, poles
    blt(2 pi alpha (-1.1016 +- 0.6360j)) with blt(p) = (2 + p) / (2 - p), a double zero at -1; gain = |top(1) / bot(1)| makes
    the DC gain one, c_i = -bot[i] / bot[2]:  y[n] = (x[n-2] + x[n]) + 2 x[n-1] + c0 y[n-2] + c1 y[n-1], x = input / gain."""
    alpha = math.tan(math.pi * freq / rate) / math.pi
    p = 2.0 * math.pi * alpha * BESSEL2_POLE
    p0, p1 = (2.0 + p) / (2.0 - p), (2.0 + p.conjugate()) / (2.0 - p.conjugate())
    bot = [(p0 * p1).real, -(p0 + p1).real, 1.0]  # (z - p0)(z - p1), coefficients of z^0, z^1, z^2
    gain = abs(4.0 / (bot[0] + bot[1] + bot[2]))  # top(1) = (1 + 1)^2
    return gain, -bot[0] / bot[2], -bot[1] / bot[2]


def lowpass(z, freq, rate=WAVE_RATE):
    """The filter over a complex128 sequence, from rest."""
    gain, c0, c1 = lowpass_coeffs(freq, rate)
    x = np.asarray(z, dtype=np.complex128) / gain
    out = np.zeros(x.size, np.complex128)
    x0 = x1 = y0 = y1 = 0j
    for i in range(x.size):
        x2 = complex(x[i])
        y2 = (x0 + x2) + 2.0 * x1 + c0 * y0 + c1 * y1
        x0, x1 = x1, x2
        y0, y1 = y1, y2
        out[i] = y2
    return out


def lowpass_gain(freq, at_hz, rate=WAVE_RATE):
    """H(e^{jw}) = (1 + 2 z + z^2) / gain / (1 - c1 z - c0 z^2), z = e^{-jw}."""
    gain, c0, c1 = lowpass_coeffs(freq, rate)
    z = np.exp(-2j * np.pi * at_hz / rate)
    return complex((1.0 + 2.0 * z + z * z) / gain / (1.0 - c1 * z - c0 * z * z))


def alpha_for_tau(tau_us):
    return 0.0 if tau_us == 0 else math.exp(-1.0 / (WAVE_RATE * 1e-6 * tau_us))


def alpha_of(dev, chan):
    """Channel tau, else device tau, else the 200 us default."""
    tau = chan.tau if chan.tau >= 0 else (dev.tau if dev.tau >= 0 else 200)
    return alpha_for_tau(tau)


def dc_block_deemphasis(d, alpha):
    """mean <- 0.995 mean + 0.005 d;  v = d - mean;  y <- (1 - alpha) v + alpha y."""
    out = np.zeros(d.size)
    mean = 0.0
    y = 0.0
    for i in range(d.size):
        mean = 0.995 * mean + 0.005 * d[i]
        y = (d[i] - mean) * (1.0 - alpha) + y * alpha
        out[i] = y
    return out


def notch_coeffs(freq, q=10.0, rate=WAVE_RATE):
    """wo = 2 pi f / rate, e = 1 / (1 + tan(wo / 2q)), p = cos wo: d = (e, 2 e p, 2 e - 1)."""
    wo = 2.0 * np.pi * freq / rate
    e = 1.0 / (1.0 + math.tan(wo / (2.0 * q)))
    return e, 2.0 * e * math.cos(wo), 2.0 * e - 1.0


def notch(x, freq, q=10.0):
    """y[n] = d0 x[n] - d1 x[n-1] + d0 x[n-2] + d1 y[n-1] - d2 y[n-2]."""
    d0, d1, d2 = notch_coeffs(freq, q)
    out = np.zeros(x.size)
    x1 = x2 = y1 = y2 = 0.0
    for i in range(x.size):
        y = d0 * x[i] - d1 * x1 + d0 * x2 + d1 * y1 - d2 * y2
        x2, x1 = x1, x[i]
        y2, y1 = y1, y
        out[i] = y
    return out


def notch_gain(freq, at_hz, q=10.0):
    d0, d1, d2 = notch_coeffs(freq, q)
    z = np.exp(-2j * np.pi * at_hz / WAVE_RATE)
    return complex((d0 - d1 * z + d0 * z * z) / (1.0 - d1 * z + d2 * z * z))


# ------------------------------------------------------------------ a channel over a span

def bandwidth_of(chan):
    return int(getattr(chan, "bandwidth", 0))


def needs_raw_iq(chan):
    """NFM, a raw-I/Q output, or the bandwidth key present (any value but the 0 that stands for "absent")."""
    return chan.modulation == MOD_NFM or bool(chan.has_iq_outputs) or bandwidth_of(chan) != 0


def model_channel(x, dev, chan, g0, g1, mode="as_specified", warmup=10000, phase0=None, X=None):
    """The model's output for audio samples g0 .. g1 of one channel.

    x: complex samples of the capture.  dev / chan: objects with the fields of the device and channel configuration.
    warmup: windows before the span over which the recursions (averages, de-emphasis, notch, low-pass) run in.
    phase0: as_specified only -- the 24-bit accumulator at raw-I/Q sample g0 - 100 (the model has no squelch, so it cannot
    know how often the accumulator stepped before the span).
    Returns a dict: audio (after ampfactor / clamp), audio_lin (before), mag (|X| of windows g0-100 .. g1), agc_mag (AM: every
    magnitude the slow average took, warm-up included), iq (derotated and, with bandwidth > 0, low-passed windows g0-100 ..
    g1-100; None for a channel that needs no raw I/Q), bin.
    """
    n = 1 << dev.fft_size_log
    b = bin_index(chan.freq, dev.centerfreq, dev.sample_rate, n)
    w0 = g0 - AGC_EXTRA - warmup
    if X is None:
        X = channelize(x, dev.sample_rate, n, [b], w0, g1 - w0)[0]
    res = {"bin": b, "iq": None, "mag": np.abs(X[warmup:])}
    if not needs_raw_iq(chan):
        lin, out = am_audio(np.abs(X), chan.ampfactor)
        res["audio_lin"], res["audio"], res["agc_mag"] = lin[warmup:], out[warmup:], np.abs(X)
        return res
    # raw I/Q: windows w0 .. g1 - 100
    Z = X[:g1 - AGC_EXTRA - w0]
    if mode == "as_specified":
        if phase0 is None:
            raise ValueError("as_specified needs the accumulator at the start of the span")
        start = (int(phase0) - warmup * dm_dphi(chan.freq, dev.centerfreq, dev.sample_rate)) % PHASE_ONE
        z = derotate(Z, chan.freq, dev.centerfreq, dev.sample_rate, mode, phase0=start)
    else:
        z = derotate(Z, chan.freq, dev.centerfreq, dev.sample_rate, mode, first_window=w0)
    if bandwidth_of(chan) > 0:
        z = lowpass(z, bandwidth_of(chan) / 2.0)
    res["iq"] = z[warmup:]
    if chan.modulation == MOD_AM:
        # m[w + 100] = |z_w|: am_audio's k-th output is audio g = w0 + 200 + k (numerator z_{g-200}, average up to z_{g-100})
        lin, out = am_audio(np.abs(z), chan.ampfactor)
        # (agc_mag: the first 100 magnitudes only seed the average, and a low-pass starting from rest leaves zeros among them)
        res["audio_lin"], res["audio"], res["agc_mag"] = lin[warmup - AGC_EXTRA:], out[warmup - AGC_EXTRA:], np.abs(z)[AGC_EXTRA:]
    else:
        d = discriminator(z, mode, quadri=bool(dev.fm_quadri))  # d[i] belongs to window w0 + 1 + i, audio g = that + 100
        y = dc_block_deemphasis(d, alpha_of(dev, chan))
        if chan.notch_freq > 0:
            y = notch(y, chan.notch_freq, chan.notch_q if chan.notch_q > 0 else 10.0)
        res["audio_lin"] = y[warmup - 1:]
        res["audio"] = clamp(y, chan.ampfactor)[warmup - 1:]
    return res


def accumulator_candidates(freq, centerfreq, sample_rate, steps):
    """Every value the accumulator can hold after 0 .. steps increments from zero."""
    return (np.arange(steps + 1, dtype=np.int64) * (dm_dphi(freq, centerfreq, sample_rate) & (PHASE_ONE - 1))) % PHASE_ONE


def accumulator_at(X0, z0, freq, centerfreq, sample_rate, steps):
    """The accumulator value that turned window X0 into the backend's raw-I/Q sample z0: the candidate (a multiple of the
    increment, at most `steps` of them) nearest to the angle between the two.  The one free integer the model takes from
    the backend; a wrong derotation sign or increment shows in every later sample."""
    want = (-np.angle(complex(z0) * np.conj(complex(X0))) / (2.0 * np.pi)) % 1.0 * PHASE_ONE
    cand = accumulator_candidates(freq, centerfreq, sample_rate, steps)
    dist = np.abs((cand - want + PHASE_ONE / 2) % PHASE_ONE - PHASE_ONE / 2)
    return int(cand[int(np.argmin(dist))])


def accumulator_fit(X, z, freq, centerfreq, sample_rate, steps, lowpass_hz, settle=200, nearest=8):
    """The same integer for a low-passed row, where the backend's raw-I/Q sample is no longer one window times (cos - j sin).
    X: windows s - settle .. s + len(z); z: the backend's raw I/Q from sample s on (a few hundred).  Taken from the backend:
    those samples, used only to choose among the multiples of the increment.  The filter is linear, so a constant offset of
    the accumulator turns its whole output: the turn between z and the model's output at accumulator 0 names the wanted value;
    the `nearest` candidates to it are run through the model (table derotation, low-pass from rest `settle` windows before s --
    the filter's poles have a radius below 0.8) and the one with the smallest residual is returned, as the accumulator at s."""
    X = np.asarray(X, dtype=np.complex128)
    z = np.asarray(z, dtype=np.complex128)
    inc = dm_dphi(freq, centerfreq, sample_rate) & (PHASE_ONE - 1)

    def run(at_s):
        start = (int(at_s) - settle * inc) % PHASE_ONE
        return lowpass(derotate(X, freq, centerfreq, sample_rate, "as_specified", phase0=start), lowpass_hz)[settle:]

    want = (-np.angle(np.vdot(run(0), z)) / (2.0 * np.pi)) % 1.0 * PHASE_ONE
    cand = np.unique(accumulator_candidates(freq, centerfreq, sample_rate, steps))
    dist = np.abs((cand - want + PHASE_ONE / 2) % PHASE_ONE - PHASE_ONE / 2)
    best = [int(c) for c in cand[np.argsort(dist)[:nearest]]]
    return min(best, key=lambda c: rms(run(c) - z))


# ------------------------------------------------------------------ measuring

def tone(x, hz, rate=WAVE_RATE):
    """Complex amplitude of the component at `hz`: a sin(2 pi hz t + p) gives abs = a and angle = p - pi / 2.  No window: use
    spans that hold whole periods."""
    x = np.asarray(x, dtype=np.float64)
    t = np.arange(x.size) / rate
    return 2.0 * np.sum((x - x.mean()) * np.exp(-2j * np.pi * hz * t)) / x.size


def peak_hz(x, rate=WAVE_RATE):
    """Frequency of the largest bin of the (mean-removed) spectrum and the bin width."""
    x = np.asarray(x, dtype=np.float64)
    sp = np.abs(np.fft.rfft(x - x.mean()))
    return float(np.argmax(sp)) * rate / x.size, rate / x.size


def rms(x):
    return float(np.sqrt(np.mean(np.abs(np.asarray(x)) ** 2)))
