"""The voice band stage's definition (include/mi_airband.h "voice band stage") restated in numpy, and the audio its tests run on.

The taps come from the formula in float64; the filter is 511 sequential float32 array operations over all outputs of a row at once,
each product and each sum rounded on its own; the clamp is np.clip.  A row is one running sequence: the model pads it with the 510
samples the state carries and filters the whole call in one go, where the device and the twin go block by block."""
import functools

import numpy as np

WAVE_BATCH, WAVE_RATE = 2000, 16000
TAPS, HISTORY, CENTRE = 511, 510, 255
STATE = np.dtype([("x", "<f4", (HISTORY,))])
DEFAULT_ROW = (100, 2500)
PAIRS = [(100, 2500), (300, 3400), (0, 2500), (300, 0)]  # the settings whose response the tests measure
THREE_CLASSES = [(100, 2500), (300, 3400), (0, 0)]


def settings_ok(hp, lp):
    return (hp == 0 or 50 <= hp <= 4000) and (lp == 0 or 500 <= lp <= 7800) and (lp == 0 or lp >= hp + 200)


def design64(hp, lp):
    """g[0 .. 510] in float64: the lower half and the centre from the formula, the upper half their mirror image"""
    k = np.arange(CENTRE + 1, dtype=np.float64)
    c = k - CENTRE
    fl, fh = hp / float(WAVE_RATE), lp / float(WAVE_RATE)
    upper = 2 * fh * np.sinc(2 * fh * c) if lp else (c == 0).astype(np.float64)  # np.sinc(t) = sin(pi t) / (pi t), 1 at 0
    g = (upper - 2 * fl * np.sinc(2 * fl * c)) * (0.42 - 0.5 * np.cos(2 * np.pi * k / HISTORY) + 0.08 * np.cos(4 * np.pi * k / HISTORY))
    return np.concatenate([g, g[-2::-1]])


@functools.lru_cache(maxsize=None)
def taps(hp, lp):
    assert settings_ok(hp, lp)
    h = design64(hp, lp).astype(np.float32)
    assert h.shape == (TAPS,)
    h.setflags(write=False)
    return h


def response_db(h, nfft=1 << 17):
    """(freqs in Hz, |H| in dB) of taps h from an nfft-point float64 FFT at the rate of 16000"""
    mag = np.abs(np.fft.rfft(np.asarray(h, np.float64), nfft))
    return np.arange(nfft // 2 + 1) * (WAVE_RATE / nfft), 20 * np.log10(np.maximum(mag, 1e-300))


def band_figures(h, hp, lp, guard=100.0):
    """(largest |dB| from `guard` Hz inside each edge, largest dB from `guard` Hz outside each edge or None without a stopband)"""
    f, db = response_db(h)
    lo, hi = (hp + guard if hp else 0.0), (lp - guard if lp else WAVE_RATE / 2)
    inside = (f >= lo) & (f <= hi)
    outside = np.zeros(len(f), bool)
    if hp:
        outside |= f <= hp - guard
    if lp:
        outside |= f >= lp + guard
    return float(np.abs(db[inside]).max()), float(db[outside].max()) if outside.any() else None


def fir(x, h):
    """x [..., 510 + n] float32, the samples behind the 510 before them -> y [..., n] float32, before the clamp"""
    n = x.shape[-1] - HISTORY
    acc = np.zeros(x.shape[:-1] + (n,), np.float32)
    for k in range(TAPS):
        acc = acc + h[k] * x[..., HISTORY - k:HISTORY - k + n]
    assert acc.dtype == np.float32
    return acc


def fresh_state(rows):
    return np.zeros(rows, STATE)


def row_settings(cfg, rows):
    """None, one (hp, lp) or one per row -> [(hp, lp)] * rows"""
    if cfg is None:
        cfg = DEFAULT_ROW
    a = np.asarray(cfg, np.int64).reshape(-1, 2)
    assert len(a) in (1, rows)
    return [tuple(int(v) for v in a[r if len(a) > 1 else 0]) for r in range(rows)]


def vband_model(wave, cfg=None, state=None, enabled=None, nbatches=None, out=None):
    """One call: wave [rows][>= nbatches * 2000] float32, cfg as row_settings takes it, state [rows] of STATE or None (fresh), enabled
    [rows] or None (all), out [rows][>= nbatches * 2000] to write into or None (zeros).  Returns (out, the state after the call); a
    disabled row's floats in `out` and its state stay."""
    wave = np.asarray(wave, np.float32)
    rows = wave.shape[0]
    nb = wave.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    n = nb * WAVE_BATCH
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(STATE).reshape(rows)
    enabled = np.ones(rows, bool) if enabled is None else np.asarray(enabled).astype(bool)
    out = np.zeros((rows, n), np.float32) if out is None else np.array(out, copy=True)
    after = state.copy()
    cfgs = row_settings(cfg, rows)
    for r in range(rows):
        if not enabled[r]:
            continue
        x = np.concatenate([state["x"][r], wave[r, :n]])
        out[r, :n] = np.clip(fir(x, taps(*cfgs[r])), np.float32(-1.0), np.float32(1.0))
        after["x"][r] = wave[r, n - HISTORY:n]
    return out, after


# ---------------- audio ----------------

def silence(rows, nb, seed=0):
    return np.zeros((rows, nb * WAVE_BATCH), np.float32)


def minus_zero(rows, nb, seed=0):
    """-0.0 throughout: compares equal to zero, and the definition gives +0.0"""
    return np.full((rows, nb * WAVE_BATCH), np.float32(-0.0))


SQUARE_HALF_PERIODS = (25, 50, 7, 400, 100)


def square(rows, nb, seed=0):
    """full-scale +-1 square waves, row r with half-period SQUARE_HALF_PERIODS[r % 5]: the filter's overshoot passes +-1 and the clamp acts"""
    n = np.arange(nb * WAVE_BATCH)
    out = np.empty((rows, len(n)), np.float32)
    for r in range(rows):
        out[r] = np.where((n // SQUARE_HALF_PERIODS[r % len(SQUARE_HALF_PERIODS)]) % 2 == 0, 1.0, -1.0)
    return out


def subnormal(rows, nb, seed=0):
    """values of subnormal size of both signs with a few of the smallest normal ones between them: every product is subnormal or zero,
    nothing compares equal to zero, and the carried state must hold these bit patterns as they are"""
    rng = np.random.default_rng(2000 + seed)
    bits = rng.integers(1, 1 << 23, (rows, nb * WAVE_BATCH)).astype(np.uint32)
    bits[:, ::97] = 0x00800000  # 2^-126
    bits |= rng.integers(0, 2, bits.shape).astype(np.uint32) << 31
    return bits.view(np.float32)


def noise(rows, nb, seed=0):
    return np.random.default_rng(3000 + seed).uniform(-1.0, 1.0, (rows, nb * WAVE_BATCH)).astype(np.float32)


VOICE_TONE_HZ, VOICE_PROBE_HZ, VOICE_GRID_HZ = 100.0, 1000.0, 50.0


def voice_hum(rows, nb, seed=0):
    """a 1 kHz component of 0.3 and two more voice-band tones of 0.15, plus a 100 Hz tone of 0.2 (a CTCSS tone that leaked through, or
    hum): what (300, 3400) is set for.  Every frequency is a multiple of 50 Hz, so that over a whole number of 320-sample periods
    the components are orthogonal and `projection` measures one of them without the others leaking in."""
    rng = np.random.default_rng(1000 + seed)
    n = np.arange(nb * WAVE_BATCH, dtype=np.float64)
    out = np.zeros((rows, len(n)))
    grid = np.array([f for f in np.arange(400.0, 2801.0, VOICE_GRID_HZ) if f != VOICE_PROBE_HZ])
    for r in range(rows):
        out[r] = 0.3 * np.sin(2 * np.pi * VOICE_PROBE_HZ * n / WAVE_RATE + rng.uniform(0, 6.28))
        for f in rng.choice(grid, 2, replace=False):
            out[r] += 0.15 * np.sin(2 * np.pi * f * n / WAVE_RATE + rng.uniform(0, 6.28))
        out[r] += 0.2 * np.sin(2 * np.pi * VOICE_TONE_HZ * n / WAVE_RATE + rng.uniform(0, 6.28))
    return out.astype(np.float32)


def lone(sample):
    """silence but for one sample of 0.75 at `sample` of every row (negative: counted from the end of the call)"""
    def build(rows, nb, seed=0):
        out = silence(rows, nb)
        out[:, sample] = 0.75
        return out
    return build


# The last four are where the zero-span skip and the seam can go wrong.  The tests run a builder's audio with a last call of one
# batch behind everything else, so "the previous call" exists.  lone_first and lone_last are the only samples of block 0's 2510 that
# are not zero, at its two ends; lone_last is also the newest of the 510 the next block takes from the batch before it (or, in a call
# of one batch, from the state); lone_prev_batch_last is the newest sample the state carries into the last call;
# lone_carried_oldest is the oldest one, which the last call's block reaches with tap 510 of output 0 alone.
BUILDERS = {"silence": silence, "minus_zero": minus_zero, "square": square, "subnormal": subnormal, "noise": noise, "voice_hum": voice_hum,
            "lone_first": lone(0), "lone_last": lone(WAVE_BATCH - 1), "lone_prev_batch_last": lone(-WAVE_BATCH - 1), "lone_carried_oldest": lone(-WAVE_BATCH - HISTORY)}


@functools.lru_cache(maxsize=None)
def audio(name, rows, nb, seed=0):
    a = BUILDERS[name](rows, nb, seed)
    assert a.dtype == np.float32 and a.shape == (rows, nb * WAVE_BATCH) and np.isfinite(a).all() and (np.abs(a) <= 1).all()
    a.setflags(write=False)
    return a


def projection(x, freq_hz, skip=0):
    """amplitude of the `freq_hz` component of x from sample `skip` on, over the longest whole number of periods of VOICE_GRID_HZ that
    fits: the inner products with sin and cos in float64"""
    period = int(WAVE_RATE / VOICE_GRID_HZ)
    span = (len(x) - skip) // period * period
    assert span >= period and freq_hz % VOICE_GRID_HZ == 0
    n = np.arange(skip, skip + span, dtype=np.float64)
    seg = np.asarray(x, np.float64)[skip:skip + span]
    s, c = np.sin(2 * np.pi * freq_hz * n / WAVE_RATE), np.cos(2 * np.pi * freq_hz * n / WAVE_RATE)
    return float(np.hypot(seg @ s, seg @ c) * 2 / span)
