"""The oracle against a float64 signal model (tests/signal_model.py), from the IQ bytes.

Bitwise equality with oracle/airband_oracle.c proves the kernels as far as the oracle is proved; its demodulate() glue (AM AGC
and lookahead, both NFM discriminators, mean removal and de-emphasis, the table derotation in front of raw I/Q, ampfactor and
clamp, the notch as it sits in the chain, bin and dm_dphi rules) is restated from the reference's text.  Here that glue is held
to a model written from signal theory:

 (a) the model itself returns the modulating tone of an analytically generated waveform, with the amplitude and phase theory gives;
 (b) the oracle's audio and raw I/Q equal the model's (as_specified mode) from the same bytes, audio to 1e-4 RMS;
 (c) physical facts hold on the oracle's output with no model arithmetic in between.

Both channel sets of tests/signal_cases.py go through (b) and (c): the nine plain rows, and the eight rows on the raw-I/Q path
(AM with its magnitudes overwritten 100 steps late, the Bessel low-pass in front of AM and NFM).  dBFS (every manual squelch
threshold) is held to its closed form and to a carrier bracketed by two thresholds.

tests/test_gpu_signal_model.py runs (b) and (c) on the HIP library with the same code and bounds.
"""
import functools
import os

import numpy as np
import pytest

import libs
import signal_cases as sc
import signal_model as sm
from conftest import load_package

CPU_CASES = ["fft512", "fft512_quadri", "fft512_s16", "fft2048", "fft2048_quadri", "fft1024_2500k", "fft4096"]
ROWS = list(range(len(sc.ROW_NAMES)))
# the second channel set (AM on the raw-I/Q path, the low-pass); fft1024_2500k: a wrong increment leaves the carrier off DC
# and the low-pass eats it; fft2048_quadri: the geometry the GPU file runs the quadrature discriminator behind the low-pass at
FILTERED_CASES = ["fft512", "fft512_quadri", "fft2048", "fft2048_quadri", "fft1024_2500k"]
FILTERED_ROWS = list(range(len(sc.FILTERED_ROW_NAMES)))


@functools.lru_cache(maxsize=None)
def oracle_case(name, rows="plain"):
    pkg = load_package()
    make, names = sc.ROW_SETS[rows]
    dev = libs.device_cfg(centerfreq=sc.CENTRE, **sc.CASES[name])
    chans = make(libs.channel_cfg)
    raw = sc.capture(pkg, dev)
    od = libs.OracleDemod(dev, chans)
    nb, wo, axc, iqo = od.run(raw, sc.NBATCHES, want_iq=True)
    levels = od.squelch_levels()
    od.close()
    assert nb == sc.NBATCHES
    return dev, chans, sc.Backend(f"oracle {name}", wo, axc, iqo, levels, names), sc.Model(dev, chans, raw)


# ---------------------------------------------------------------------------------------------- (a) the model by itself

def atan_bound():
    """Largest distance between the fast-atan2 discriminator and the true angle, in the discriminator's unit (pi)."""
    th = np.linspace(-np.pi, np.pi, 200001)
    return float(np.max(np.abs(sm.fast_atan2(np.sin(th), np.cos(th)) - th))) / np.pi


def audio_bound_from_atan():
    """What the discriminator's bound becomes at the audio: the error e goes through the mean removal e - ema(e), whose impulse
    response (1 - 0.005, -0.005 * 0.995^k ...) has an absolute sum of 0.995 + 0.995 = 1.99, and then through the de-emphasis,
    whose taps are positive and sum to 1.  max |audio error| <= 1.99 max |e|."""
    k = np.arange(1, 20000)
    return atan_bound() * (0.995 + float(np.sum(0.005 * 0.995 ** k)))


def test_fast_atan2_distance_from_the_true_angle():
    """The first-order rational's known worst case: 0.0711 rad (4.07 degrees) near 15.8 and 74.2 degrees of every quadrant, exact
    on the axes and diagonals."""
    b = atan_bound() * np.pi
    assert 0.0710 < b < 0.0713, b
    for deg in (0, 45, 90, 135, 180, -45, -90, -135):
        th = np.deg2rad(deg)
        assert abs(sm.fast_atan2(np.sin(th), np.cos(th)) - th) < 1e-12
    # a quick rotation by a small angle: the two discriminators agree on sign and order
    z = np.exp(1j * np.array([0.0, 0.3, 0.1]))
    d = sm.discriminator(z, "as_specified")
    assert d[0] > 0 > d[1]
    assert np.allclose(sm.discriminator(z, "exact") * np.pi, [0.3, -0.2])


def test_bin_rule_and_phase_increment_closed_forms():
    # off the grid: the bin whose centre is nearest below-or-at; on the grid: one bin down
    assert sm.bin_index(120000000 + 2700, 120000000, 2560000, 512) == 0
    assert sm.bin_index(120000000 + 5000, 120000000, 2560000, 512) == 0
    assert sm.bin_index(120000000 + 5001, 120000000, 2560000, 512) == 1
    assert sm.bin_index(120000000, 120000000, 2560000, 512) == 511
    assert sm.bin_index(120000000 - 377300, 120000000, 2560000, 512) == 436
    # 2.56 MS/s: the hop is exact, the increment is the offset in turns per sample
    assert sm.dm_dphi(120000000 + 4000, 120000000, 2560000) == (1 << 24) // 4
    assert sm.dm_dphi(120000000 - 4000, 120000000, 2560000) & 0xffffff == 3 * (1 << 24) // 4
    # 2.5 MS/s: hop 156 of 156.25; the increment follows the true advance per window to within its truncation
    f = 613700
    adv = sm.phase_advance_exact(120000000 + f, 120000000, 2500000) / (2 * np.pi) % 1.0
    assert abs(sm.dm_dphi(120000000 + f, 120000000, 2500000) / 2.0 ** 24 - adv) < 2.0 ** -24 + 1e-12
    assert abs(sm.dm_dphi(120000000 + f, 120000000, 2500000, with_correction=False) / 2.0 ** 24 - adv) > 1e-3


def fit_phase(z, fm=1000.0):
    """Least squares beta sin(2 pi fm t + p) + c + s t on the unwrapped phase; returns beta, s and their standard errors, the
    latter widened by the residual's own correlation (windows overlap, so neighbouring phase errors are not independent)."""
    ph = np.unwrap(np.angle(z))
    t = np.arange(ph.size, dtype=np.float64)
    w = 2 * np.pi * fm / sm.WAVE_RATE
    A = np.stack([np.sin(w * t), np.cos(w * t), np.ones_like(t), t - t.mean()], axis=1)
    coef, *_ = np.linalg.lstsq(A, ph, rcond=None)
    res = ph - A @ coef
    var = res @ res / (ph.size - 4)
    rho = [float(res[k:] @ res[:-k] / (res @ res)) for k in range(1, 8)]
    inflate = max(1.0, 1.0 + 2.0 * sum(rho))
    cov = np.linalg.inv(A.T @ A) * var * inflate
    beta = float(np.hypot(coef[0], coef[1]))
    beta_se = float(np.sqrt((coef[0] ** 2 * cov[0, 0] + coef[1] ** 2 * cov[1, 1]) / beta ** 2))
    return beta, beta_se, float(coef[3]), float(np.sqrt(cov[3, 3]))


def _analytic(rate, n_windows, nfft, f0, am=0.0, beta=0.0, fm=1000.0):
    t = np.arange(n_windows * sm.hop_of(rate) + nfft) / rate
    return 0.1 * (1.0 + am * np.sin(2 * np.pi * fm * t)) * np.exp(1j * (2 * np.pi * f0 * t + beta * np.sin(2 * np.pi * fm * t)))


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("log2n,delta", [(9, 0.0), (9, 2700.0), (11, 0.0), (11, 400.0)])
def test_model_returns_the_am_tone(log2n, delta):
    """x = (1 + m sin) e^{j 2 pi f0 t}, no noise.  With W the window's DTFT the bin holds W(d) + m/2j (W(d + fm) e^{j psi} -
    W(d - fm) e^{-j psi}); for a symmetric window W(v) = e^{+j pi v (N-1)/rate} Wr(v), so the envelope is 1 + m g sin(psi_w +
    pi fm (N-1)/rate) with g = (Wr(d+fm) + Wr(d-fm)) / 2 Wr(d), plus a quadrature term m (Wr(d+fm) - Wr(d-fm)) / 2 Wr(d) that enters
    the magnitude squared.  The audio is (|X_{g-100}| - agc) / 1.5 agc: amplitude m g / 1.5 after the slow average's own ripple
    H = 0.005 / (1 - 0.995 e^{-jw}) is taken out of the numerator."""
    rate, n, m, fm = 2560000, 1 << log2n, 0.5, 1000.0
    centre = 120000000
    k = 37
    f0 = k * rate / n + delta
    nwin = 4000 + 1600 + 100
    x = _analytic(rate, nwin, n, f0, am=m)
    X = sm.channelize(x, rate, n, [k], 0, nwin)[0]
    audio, _ = sm.am_audio(np.abs(X))
    a = audio[4000:5600]  # g = 4100 .. 5700: 100 whole periods
    hz, width = sm.peak_hz(a)
    assert abs(hz - 1000.0) < width / 2
    wr = lambda v: abs(sm.window_dtft(n, rate, v))
    gp, gm = wr(delta + fm) / wr(delta), wr(delta - fm) / wr(delta)
    g, quad = (gp + gm) / 2, m * abs(gp - gm) / 2
    w = 2 * np.pi * fm / sm.WAVE_RATE
    H = 0.005 / (1 - 0.995 * np.exp(-1j * w))
    # phasor of the envelope at window index g: m g e^{j(w g + pi fm (N-1)/rate)}; audio g uses window g - 100 and subtracts agc_g
    want = m * g / 1.5 * (np.exp(-1j * w * sm.AGC_EXTRA) - H) * np.exp(1j * (w * 4100 + np.pi * fm * (n - 1) / rate))
    got = sm.tone(a, fm) * 1j  # tone() returns a e^{j(p - pi/2)} for a sin(w t + p)
    tol = abs(want) * (quad ** 2 + 2 * m * g * abs(H)) + 1e-6  # second order: quadrature term, ripple of the denominator
    print(f"AM fft {n} delta {delta}: sideband gain {g:.5f}, audio amplitude {abs(got):.5f} (m g / 1.5 = {m * g / 1.5:.5f}), |got - want| {abs(got - want):.2e}, tol {tol:.2e}")
    assert abs(got - want) <= tol
    assert abs(abs(got) - m * g / 1.5) <= 0.02 * m * g / 1.5


def test_model_returns_the_nfm_tone_at_fft_512():
    """x = e^{j(2 pi f0 t + beta sin(2 pi fm t))} at fft 512, where the 5 kHz bin under the wide window passes the 2.5 kHz
    deviation.  The phase difference of consecutive windows is 2 beta sin(pi fm / 16000) cos(..); over pi that is the
    discriminator's amplitude, times the mean removal's gain |1 - H| and the de-emphasis gain (1 - a) / |1 - a e^{-jw}|.  The
    window averages the phase over its own length: the tone is smoothed by 1 - (2 pi fm sigma_t)^2 / 2 with sigma_t the window's
    RMS width -- half of that figure is allowed as what this first-order estimate leaves out."""
    rate, n, beta, fm = 2560000, 512, 2.5, 1000.0
    centre, off = 120000000, 613700
    dev = _Cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9, sfmt=sm.SFMT_U8, fullscale=127.5, tau=-1, fm_quadri=0)
    chan = _Cfg(freq=centre + off, modulation=sm.MOD_NFM, notch_freq=0.0, notch_q=0.0, ampfactor=1.0, tau=-1, has_iq_outputs=1)
    g0, g1, warm = 4200, 5800, 4000
    x = _analytic(rate, g1 + 10, n, off, beta=beta)
    r = sm.model_channel(x, dev, chan, g0, g1, mode="exact", warmup=warm)
    hz, width = sm.peak_hz(r["audio"])
    assert abs(hz - 1000.0) < width / 2
    w = 2 * np.pi * fm / sm.WAVE_RATE
    alpha = sm.alpha_for_tau(200)
    H = 0.005 / (1 - 0.995 * np.exp(-1j * w))
    win = sm.window(n)
    mid = (n - 1) / 2
    sigma_t = np.sqrt(np.sum(win * (np.arange(n) - mid) ** 2) / np.sum(win)) / rate
    smooth = (2 * np.pi * fm * sigma_t) ** 2 / 2
    want = 2 * beta * np.sin(np.pi * fm / sm.WAVE_RATE) / np.pi * abs(1 - H) * (1 - alpha) / abs(1 - alpha * np.exp(-1j * w)) * (1 - smooth)
    got = abs(sm.tone(r["audio"], fm))
    print(f"NFM fft 512: audio amplitude {got:.5f}, theory {want:.5f} (window smoothing {smooth:.4f})")
    assert abs(got - want) <= want * smooth / 2 + 1e-6
    # the derotated I/Q: the phase is the modulation, smoothed like the audio, with no slope (fitted together: a line fitted
    # by itself picks up 6 beta / (pi periods n) from the sine)
    b_fit, _, slope, _ = fit_phase(r["iq"])
    print(f"NFM fft 512: phase deviation after the channelizer {b_fit:.5f} of {beta}, slope {slope:.1e}")
    assert abs(slope) < 2 * np.pi / 2 ** 24 / 10  # a tenth of what the truncated increment may leave
    assert abs(b_fit - beta * (1 - smooth)) < beta * smooth / 2
    t = np.arange(r["iq"].size)
    # as_specified from the same windows: the table derotation leaves the same I/Q to the table's interpolation error
    # (2 pi / 256)^2 / 8 = 7.5e-5, and a residual slope below the truncated increment's 2 pi / 2^24 per sample
    s0 = g0 - sm.AGC_EXTRA
    rs = sm.model_channel(x, dev, chan, g0, g1, mode="as_specified", warmup=warm, phase0=(s0 * sm.dm_dphi(chan.freq, centre, rate)) % sm.PHASE_ONE)
    rot = rs["iq"] / r["iq"]
    assert np.max(np.abs(np.abs(rot) - 1)) < 8e-5
    slope = np.polyfit(t, np.unwrap(np.angle(rot)), 1)[0]  # (no sine in this one: the modulation cancels)
    assert abs(slope) <= 2 * np.pi / 2 ** 24 + 1e-9
    # and the two discriminators differ by no more than the fast-atan2 bound
    assert np.max(np.abs(rs["audio"] - r["audio"])) <= atan_bound()


def test_notch_model_gain():
    """Zeros on the unit circle at the notch frequency, unit gain far from it."""
    assert abs(sm.notch_gain(100.0, 100.0)) < 1e-12
    assert abs(abs(sm.notch_gain(100.0, 1000.0)) - 1.0) < 2e-3
    x = np.sin(2 * np.pi * 100.0 * np.arange(24000) / sm.WAVE_RATE) + 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(24000) / sm.WAVE_RATE)
    y = sm.notch(x, 100.0)[-3200:]
    assert abs(sm.tone(y, 100.0)) < 1e-6 and abs(abs(sm.tone(y, 1000.0)) - 0.5 * abs(sm.notch_gain(100.0, 1000.0))) < 1e-6


GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "components_ref.npz"))


def _lowpass_vectors(name):
    from golden_inputs import FILTER_CASES
    case = FILTER_CASES[name]
    rng = np.random.default_rng(case["seed"])
    x = rng.normal(size=case["n"]).astype(np.float32)
    y = rng.normal(size=case["n"]).astype(np.float32)
    return case["freq"], x, y


@pytest.mark.parametrize("name", ["lp6250", "lp2500", "lp4000"])
def test_lowpass_model_equals_the_reference_filter(name):
    """sm.lowpass over the inputs of the committed low-pass vectors against what the reference's own LowpassFilter made of
    them (float32 state and coefficients), and against the compiled reference itself where it is built.  Bound: 32 ulp of
    float32 (1.9e-6) of the largest output -- eight roundings a step, the recursion's memory a handful of steps (pole radius
    below 0.7 at these cut-offs); measured 2.7e-7 .. 8.5e-7 of outputs that reach 2.3 .. 3.4."""
    freq, x, y = _lowpass_vectors(name)
    out = sm.lowpass(x.astype(np.float64) + 1j * y.astype(np.float64), freq)
    want = GOLD[f"fl_{name}_re"].astype(np.float64) + 1j * GOLD[f"fl_{name}_im"].astype(np.float64)
    err = float(np.max(np.abs(out - want)))
    print(f"{name}: model low-pass against the recorded reference output: max {err:.2e} of max {np.max(np.abs(want)):.3f}")
    assert err <= 32 * 2.0 ** -24 * np.max(np.abs(want))
    r = libs.ref()
    if r is not None:
        a, b = r.lowpass_run(freq, 16000.0, x, y)
        assert np.max(np.abs(out - (a.astype(np.float64) + 1j * b))) <= 32 * 2.0 ** -24 * np.max(np.abs(want))


@pytest.mark.parametrize("bandwidth", [3000, 5000, 7000, 12500])
def test_lowpass_coefficients_against_the_plan_and_the_closed_form(bandwidth):
    """Unit DC gain; |lowpass_gain| is the steady-state response to a complex tone; the host plan's float32 coefficients (it
    shares no code with the model) are the model's, rounded."""
    f = bandwidth / 2.0
    gain, c0, c1 = sm.lowpass_coeffs(f)
    assert abs(sm.lowpass_gain(f, 0.0) - 1.0) < 1e-12
    assert abs(abs(sm.lowpass_gain(f, f)) - 10 ** (-3.0 / 20)) < 0.02  # the Bessel prototype's -3 dB point, pre-warped onto f
    t = np.arange(2400)
    for hz in (-3000.0, 100.0, 1000.0, 2500.0):
        e = np.exp(2j * np.pi * hz * t / sm.WAVE_RATE)
        y = sm.lowpass(e, f)[-1600:]
        assert abs(np.vdot(e[-1600:], y) / 1600 - sm.lowpass_gain(f, hz)) < 1e-12
    pkg = load_package()
    plan = pkg.Plan(pkg.device_cfg(), [pkg.channel_cfg(sc.CENTRE, bandwidth=bandwidth)])
    d = plan.channel(0)
    plan.close()
    assert d.lowpass_enabled and d.needs_raw_iq
    assert np.allclose([d.lowpass_gain, d.lowpass_ycoeffs[0], d.lowpass_ycoeffs[1]], [gain, c0, c1], rtol=2.0 ** -23, atol=0)


# ---------------------------------------------------------------------------------------------- (b) oracle vs model

def check_row(be, model, row, clamp_must_engage=False):
    """Shared with the GPU tests: open throughout, AM headroom, residuals within the bounds.  Returns the figures."""
    chan = model.chans[row]
    g0, g1 = model.span
    sc.assert_open(be, row, chan)
    audio, iq, m = sc.residuals(model, be, row)
    what = f"{be.name} row {be.names[row]}: audio residual {audio:.3e} RMS (bound {sc.AUDIO_BOUND:.0e}, audio RMS {sm.rms(m['audio']):.3f})"
    if iq is not None:
        what += f", raw I/Q residual {iq:.3e} of the model's RMS (bound {sc.iq_bound(chan):.2e})"
    print(what)
    if chan.modulation == sm.MOD_AM:
        sc.assert_am_above_level(model, be, row, m)
    assert sm.rms(m["audio"]) > 0.01, what
    assert audio <= sc.AUDIO_BOUND, what
    if iq is not None:
        assert iq <= sc.iq_bound(chan), what
    if clamp_must_engage:
        hit_model = int((np.abs(m["audio"]) == 1.0).sum())
        hit = int((np.abs(be.waveout[row, g0:g1]) == 1.0).sum())
        assert hit_model > 50 and hit > 50 and np.max(np.abs(m["audio_lin"])) * chan.ampfactor > 1.0, f"{what}: clamp engaged {hit} / {hit_model} times"
    return audio, iq


@pytest.mark.parametrize("row", ROWS, ids=sc.ROW_NAMES)
@pytest.mark.parametrize("case", CPU_CASES)
def test_oracle_equals_the_model(case, row):
    dev, chans, be, model = oracle_case(case)
    check_row(be, model, row, clamp_must_engage=(row == sc.AM_LOUD and dev.fft_size_log == 9))


@pytest.mark.parametrize("row", FILTERED_ROWS, ids=sc.FILTERED_ROW_NAMES)
@pytest.mark.parametrize("case", FILTERED_CASES)
def test_oracle_equals_the_model_on_the_filtered_rows(case, row):
    """AM on the raw-I/Q path (the magnitudes overwritten 100 steps late) and the low-pass.  Rows that emit raw I/Q are
    compared as specified, the AM rows with the bandwidth key alone with true sin / cos (signal_cases.mode_for)."""
    dev, chans, be, model = oracle_case(case, "filtered")
    check_row(be, model, row, clamp_must_engage=(row == sc.F_AM_BW15000_LOUD and dev.fft_size_log == 9))


def old_am_model(model, row):
    """What the model computed for an AM row before it followed the raw-I/Q path: audio from |X|, no further lag."""
    return sm.am_audio(np.abs(model.X[row]), model.chans[row].ampfactor)[1][model.warmup:]


def test_the_lag_of_the_raw_iq_path_is_load_bearing():
    """An AM row with a raw-I/Q output against the model without the lagged overwrite: it must miss by more than 0.1 RMS
    (0.327 against an audio RMS of 0.231), so nobody simplifies the lag away."""
    dev, chans, be, model = oracle_case("fft512", "filtered")
    g0, g1 = model.span
    sc.assert_open(be, sc.F_AM_IQ, chans[sc.F_AM_IQ])
    miss = sm.rms(be.waveout[sc.F_AM_IQ, g0:g1] - old_am_model(model, sc.F_AM_IQ))
    plain = sm.rms(be.waveout[sc.F_AM_PLAIN, g0:g1] - old_am_model(model, sc.F_AM_PLAIN))
    print(f"{be.name}: the model without the lag misses row f_am_iq by {miss:.3f} RMS (the plain row by {plain:.1e})")
    assert miss > 0.1 and plain <= sc.AUDIO_BOUND


@pytest.mark.parametrize("case", ["fft512", "fft2048", "fft1024_2500k"])
def test_oracle_against_the_exact_model(case):
    """exact mode (true sin / cos / atan2, true phase advance) against the oracle's fast-atan2 audio: every sample within the
    fast-atan2 bound computed above, carried through the mean removal (audio_bound_from_atan).  Raw I/Q: the table's interpolation error (2 pi / 256)^2 / 8 in magnitude plus the phase the
    truncated increment loses over the span (2 pi / 2^24 per sample)."""
    dev, chans, be, model = oracle_case(case)
    g0, g1 = model.span
    tol = audio_bound_from_atan()
    for row in (sc.NFM_IQ, sc.NFM_TONE, sc.NFM_TAU75, sc.NFM_TAU0):
        sc.assert_open(be, row, chans[row])
        m = model.row(row, "exact")
        worst = float(np.max(np.abs(be.waveout[row, g0:g1] - m["audio"])))
        z = be.iq[row, g0 - sm.AGC_EXTRA:g1 - sm.AGC_EXTRA]
        rot = z / m["iq"]
        rot = rot / rot[0]  # the accumulator's value at the head of the span is the model's free constant
        mag = float(np.max(np.abs(np.abs(rot) - 1)))
        drift = float(np.max(np.abs(np.angle(rot))))
        print(f"{be.name} row {be.names[row]} vs exact: audio max {worst:.4f} (bound {tol:.4f}), I/Q magnitude {mag:.2e}, phase drift {drift:.2e}")
        assert worst <= tol
        assert mag <= 2 * (2 * np.pi / 256) ** 2 / 8
        assert drift <= (g1 - g0) * 2 * np.pi / 2 ** 24 + 2 * (2 * np.pi / 256) ** 2 / 8 + 1e-5


# ---------------------------------------------------------------------------------------------- (c) physics on the output

def check_tone_peaks(be, chans, span, rows):
    g0 = span[0]
    for row in rows:
        sc.assert_open(be, row, chans[row], g0, g0 + 3200)
        hz, width = sm.peak_hz(be.waveout[row, g0:g0 + 3200])
        assert abs(hz - 1000.0) < width / 2, f"{be.name} row {be.names[row]}: audio peaks at {hz} Hz"


def check_raw_iq_phase(be, chans, span, row=sc.NFM_IQ):
    g0, g1 = span
    sc.assert_open(be, row, chans[row], g0, g1)
    z = be.iq[row, g0 - sm.AGC_EXTRA:g0 - sm.AGC_EXTRA + 3200]
    beta, beta_se, slope, slope_se = fit_phase(z)
    print(f"{be.name} row {be.names[row]}: phase fit beta {beta:.5f} +- {beta_se:.1e}, slope {slope:.3e} +- {slope_se:.1e} rad/sample")
    return beta, beta_se, slope, slope_se


def check_notch_rows(be, chans, span, tol):
    g0 = span[0]
    for row in (sc.NFM_TONE, sc.NFM_TONE_NOTCH):
        sc.assert_open(be, row, chans[row], g0 - sc.OPEN_BEFORE, g0 + 3200)
    plain, notched = be.waveout[sc.NFM_TONE, g0:g0 + 3200], be.waveout[sc.NFM_TONE_NOTCH, g0:g0 + 3200]
    assert abs(sm.tone(plain, 100.0)) > 0.02, "the carrier's 100 Hz tone is in the row without a notch"
    for hz in (100.0, 1000.0):
        ratio = sm.tone(notched, hz) / sm.tone(plain, hz)
        want = sm.notch_gain(100.0, hz)
        print(f"{be.name}: notch row / plain row at {hz:.0f} Hz = {abs(ratio):.5f} (model biquad {abs(want):.5f})")
        assert abs(ratio - want) <= tol, f"{be.name}: {hz} Hz through the notch: {ratio} against {want}"


# The raw-I/Q AM row against the plain row 100 samples earlier: the two differ only in the rounding of a rotated magnitude --
# |X (cos - j sin)| from the interpolated table is |X| times 1 - e, e between 0 and 7.5e-5 with a standard deviation of
# (2 pi / 256)^2 / 2 sqrt(1/180) = 2.2e-5 over a uniform table fraction, which the audio's 1 / 1.5 agc turns into 1.5e-5.
# Measured on the oracle at fft 512: 1.646e-5 RMS (fft 2048: 1.627e-5, fft 1024 at 2.5 MS/s: 1.570e-5); the bound is 4 x that.
LAG_BOUND = 4 * 1.646e-5
# Row f_am_bw3000_iq over row f_am_iq at 1 kHz against the low-pass's H(1 kHz) at a 1.5 kHz cut-off (0.86504, -0.88257 rad), as
# complex numbers: |ratio - H| measured on the oracle at fft 512 is 1.73e-4 (the AGC divides by an average that carries a ripple
# of its own, a second-order term); the bound is 4 x that.
TONE_RATIO_BOUND = 4 * 1.73e-4


def check_lag_of_the_raw_iq_rows(be, chans, span):
    g0, g1 = span
    for row in (sc.F_AM_PLAIN, sc.F_AM_IQ, sc.F_AM_BW_KEY):
        sc.assert_open(be, row, chans[row])
    plain, lagged = be.waveout[sc.F_AM_PLAIN], be.waveout[sc.F_AM_IQ, g0:g1]
    corr = [float(np.dot(lagged - lagged.mean(), plain[g0 - k:g1 - k] - plain[g0 - k:g1 - k].mean())) for k in range(201)]
    diff = sm.rms(lagged - plain[g0 - sm.AGC_EXTRA:g1 - sm.AGC_EXTRA])
    print(f"{be.name}: row f_am_iq correlates best with row f_am_plain {int(np.argmax(corr))} samples earlier; against exactly 100: {diff:.3e} RMS (bound {LAG_BOUND:.2e})")
    assert int(np.argmax(corr)) == sm.AGC_EXTRA
    assert diff <= LAG_BOUND
    assert np.array_equal(be.waveout[sc.F_AM_BW_KEY], be.waveout[sc.F_AM_IQ]), "bandwidth key alone: the same path, the same audio bit for bit"
    assert not be.iq[sc.F_AM_BW_KEY].any(), "bandwidth key alone: no raw-I/Q output"


def check_tone_through_the_lowpass(be, chans, span):
    g0 = span[0]
    for row in (sc.F_AM_IQ, sc.F_AM_BW3000_IQ):
        sc.assert_open(be, row, chans[row], g0 - sc.OPEN_BEFORE, g0 + 4000)
    ratio = sm.tone(be.waveout[sc.F_AM_BW3000_IQ, g0:g0 + 4000], 1000.0) / sm.tone(be.waveout[sc.F_AM_IQ, g0:g0 + 4000], 1000.0)
    want = sm.lowpass_gain(1500.0, 1000.0)
    print(f"{be.name}: 1 kHz in row f_am_bw3000_iq over row f_am_iq: {abs(ratio):.5f} at {np.angle(ratio):.5f} rad; the filter: {abs(want):.5f} at {np.angle(want):.5f} rad; "
          f"|difference| {abs(ratio - want):.2e} (bound {TONE_RATIO_BOUND:.2e})")
    assert abs(ratio - want) <= TONE_RATIO_BOUND


@pytest.mark.parametrize("case", ["fft512", "fft2048", "fft1024_2500k"])
def test_oracle_raw_iq_am_row_is_the_plain_row_100_samples_later(case):
    dev, chans, be, model = oracle_case(case, "filtered")
    check_lag_of_the_raw_iq_rows(be, chans, model.span)


def test_oracle_1_khz_tone_through_the_lowpass():
    dev, chans, be, model = oracle_case("fft512", "filtered")
    check_tone_through_the_lowpass(be, chans, model.span)


@pytest.mark.parametrize("case", FILTERED_CASES)
def test_oracle_filtered_rows_peak_at_1_khz(case):
    dev, chans, be, model = oracle_case(case, "filtered")
    check_tone_peaks(be, chans, model.span, FILTERED_ROWS)


@pytest.mark.parametrize("case", CPU_CASES)
def test_oracle_audio_peaks_at_1_khz(case):
    dev, chans, be, model = oracle_case(case)
    # fft 4096: 625 Hz bins under a 2.5 kHz deviation leave the NFM rows no clean tone (the model follows them all the same)
    check_tone_peaks(be, chans, model.span, ROWS if dev.fft_size_log < 12 else [sc.AM_ON_GRID, sc.AM_OFF_GRID, sc.AM_LOUD])


@functools.lru_cache(maxsize=None)
def beta_after_channelizer(log2n=9, rate=2560000, off=sc.OFF_NFM, beta=2.5):
    """The phase deviation a noise-free beta sin(2 pi 1000 t) carrier keeps behind the window (which averages the phase over
    its length: 2.5 becomes 2.484 at fft 512): the analytic waveform of (a) through the float64 channelizer, fitted like the
    backend's output.  test_model_returns_the_nfm_tone_at_fft_512 holds this figure to the window's RMS width."""
    n = 1 << log2n
    x = _analytic(rate, 3300, n, off, beta=beta)
    X = sm.channelize(x, rate, n, [sm.bin_index(sc.CENTRE + off, sc.CENTRE, rate, n)], 0, 3200)[0]
    return fit_phase(sm.derotate(X, sc.CENTRE + off, sc.CENTRE, rate, "exact"))[0]


def assert_raw_iq_phase(be, chans, span):
    """|slope| <= 2 pi / 2^24 (the increment's truncation) + the fit's standard error; beta within the fit's standard error of
    2.5 as the channelizer passes it."""
    beta, beta_se, slope, slope_se = check_raw_iq_phase(be, chans, span)
    want = beta_after_channelizer()
    assert abs(slope) <= 2 * np.pi / 2 ** 24 + slope_se, f"{be.name}: residual phase slope {slope:.3e} +- {slope_se:.1e} rad/sample"
    assert abs(beta - want) <= beta_se, f"{be.name}: phase deviation {beta:.5f} +- {beta_se:.1e} against {want:.5f}"


def test_oracle_raw_iq_phase_is_the_modulation_and_nothing_else():
    """NFM row at fft 512: the derotated phase is beta sin(2 pi 1000 t), beta = 2.5 less what the window smooths away, and a
    slope of at most the increment's 24-bit truncation (a wrong derotation sign leaves a slope of order 1)."""
    dev, chans, be, model = oracle_case("fft512")
    assert_raw_iq_phase(be, chans, model.span)


def test_oracle_notch_takes_the_100_hz_tone_out():
    dev, chans, be, model = oracle_case("fft512")
    check_notch_rows(be, chans, model.span, atan_bound())


def test_always_on_carrier_at_fft_512_never_opens():
    """Why every case gates its carriers: with the carriers on from the first sample the noise floor learns them and the squelch
    stays shut -- a comparison on such an input would pass on silence."""
    pkg = load_package()
    dev = libs.device_cfg(centerfreq=sc.CENTRE, fft_size_log=9)
    chans = sc.channels(libs.channel_cfg)
    hop = sm.hop_of(dev.sample_rate)
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, seed=0x51C0DE, gate_samples=0, carriers=sc.CARRIERS)
    raw = pkg.iqgen_host(cfg, 0, 0, (6 * sc.WAVE_BATCH + sm.AGC_EXTRA) * hop + 512 + hop)
    od = libs.OracleDemod(dev, chans)
    nb, wo, axc, _ = od.run(raw, 6)
    od.close()
    assert nb == 6 and (axc == ord(" ")).all() and not wo[:, sm.AGC_EXTRA:].any()


# ---------------------------------------------------------------------------------------------- dBFS (util.cpp:163-180)

@pytest.mark.parametrize("log2n", range(8, 14))
def test_dbfs_to_level_closed_form(log2n):
    """10^((dB - (7.54 + 10 log10(N / 2) - 2.38)) / 20) N in float64 against the plan's manual_signal_level and the oracle's
    ao_dbfs_to_level, every whole threshold -1 .. -100.  Tolerance 2e-6 relative: the reference forms the offset in float
    (three roundings at an ulp of 1.9e-6 near 24 .. 32) and divides by 20.0f, a 4e-6 absolute error in the exponent's
    numerator is ln 10 / 20 x 4e-6 = 5e-7 relative, and 2e-6 leaves a factor of 4 over that."""
    pkg = load_package()
    n = 1 << log2n
    dbs = list(range(-1, -101, -1))
    worst = 0.0
    for first in range(0, len(dbs), 50):  # (two plans of 50 channels: a plan holds at most 64)
        part = dbs[first:first + 50]
        plan = pkg.Plan(pkg.device_cfg(fft_size_log=log2n), [pkg.channel_cfg(sc.CENTRE + 1000, squelch_threshold_dbfs=db) for db in part])
        for i, db in enumerate(part):
            want = sc.dbfs_to_level(db, n)
            d = plan.channel(i)
            assert d.using_manual_level
            for got in (d.manual_signal_level, libs.oracle_lib().ao_dbfs_to_level(float(db), n)):
                worst = max(worst, abs(got / want - 1.0))
                assert abs(got / want - 1.0) <= 2e-6, f"fft {n}, {db} dBFS: {got} against {want}"
        plan.close()
    print(f"fft {n}: dBFS_to_level within {worst:.2e} of the closed form (bound 2e-6)")


def test_oracle_manual_threshold_brackets_a_steady_carrier():
    """A threshold 3 dB under the carrier's measured level opens for the whole of its second half, one 3 dB over never does."""
    dev = libs.device_cfg(centerfreq=sc.CENTRE, fft_size_log=9)
    raw = sc.dbfs_capture(dev)
    chans, db, (under, over) = sc.dbfs_bracket(libs.channel_cfg, dev, raw)
    print(f"carrier at {db:.2f} dBFS, thresholds {under} and {over}")
    od = libs.OracleDemod(dev, chans)
    nb, wo, axc, _ = od.run(raw, sc.DBFS_BATCHES)
    levels = od.squelch_levels()
    od.close()
    assert nb == sc.DBFS_BATCHES
    assert np.allclose(levels, [sc.dbfs_to_level(under, 512), sc.dbfs_to_level(over, 512)], rtol=2e-6, atol=0)
    sc.assert_dbfs_bracket(sc.Backend("oracle dBFS bracket", wo, axc, None, levels, ["under", "over"]))
