"""The noise reduction stage's definition (include/mi_airband.h "noise reduction stage") restated in numpy, an independent float64
restatement of it, and the audio its tests run on.

The window comes from the formula (math.sin in float64 for i <= 249, mirrored); the spectra -- the frames' and the conjugate ones of
the synthesis -- go through the oracle's ao_fft_forward at log2n 9, bound as survey_model.py binds it; everything else is float32
array operations in the stated order.  A row is one running sequence: the model pads it with the 500 samples the state carries and
transforms every frame of the call once, where the device and the twin go block by block and transform a block's first frame again.
denoise_model64 says the same with numpy.fft.rfft / irfft in float64 throughout: it shares no arithmetic with the model."""
import functools
import math

import numpy as np

import survey_model as sm
import vband_model as vm

WAVE_BATCH, WAVE_RATE = 2000, 16000
HOP, FRAME, FFT_LOG, FFT, BINS, DEPTH = 250, 500, 9, 512, 257, 8
FRAMES = WAVE_BATCH // HOP  # 8 frames begin in a batch; a block is made of 9
STATE = np.dtype([("x", "<f4", (FRAME,)), ("m", "<f4", (DEPTH - 1, BINS))])
assert STATE.itemsize == 9196
DEFAULT_ROW = (12.0, 4.5)
THREE_CLASSES = [(12.0, 4.5), (20.0, 2.0), (6.0, 8.0)]
HZ_PER_BIN = WAVE_RATE / FFT  # 31.25
LOWER = np.abs(np.arange(BINS) - 1)                  # k - 1, mirrored at 0
UPPER = BINS - 1 - np.abs(BINS - 2 - np.arange(BINS))  # k + 1, mirrored at 256
FOLD = np.minimum(np.arange(FFT), FFT - np.arange(FFT))  # min(k, 512 - k)
assert LOWER[0] == 1 and LOWER[1] == 0 and UPPER[256] == 255 and UPPER[255] == 256 and FOLD[257] == 255


def settings_ok(reduction_db, over):
    return 0 <= reduction_db <= 40 and 0 <= over <= 64


def window64():
    """the formula in float64 at every i, not mirrored"""
    return np.array([math.sin(math.pi * (i + 0.5) / FRAME) for i in range(FRAME)], np.float64)


@functools.lru_cache(maxsize=None)
def window():
    half = window64()[:HOP].astype(np.float32)
    w = np.concatenate([half, half[::-1]])
    w.setflags(write=False)
    return w


def g_min(reduction_db):
    return np.float32(10.0 ** (-float(np.float32(reduction_db)) / 20.0))


def fft512(z):
    """z [..., 512, 2] float32 -> the oracle's ao_fft_forward of every [512][2]"""
    z = np.ascontiguousarray(z, np.float32)
    out = np.empty_like(z)
    lib, plan = sm._oracle(), sm.fft_plan(FFT_LOG)
    fwd, pp = lib.ao_fft_forward, sm.C.byref(plan)
    a, b, step = z.ctypes.data, out.ctypes.data, FFT * 2 * 4
    for i in range(z.size // (2 * FFT)):
        fwd(pp, a + i * step, b + i * step)
    return out


def fresh_state(rows):
    s = np.zeros(rows, STATE)
    s["m"] = np.inf
    return s


def row_settings(cfg, rows):
    """None, one (reduction_db, over) or one per row -> float32 [rows][2]"""
    a = np.asarray(DEFAULT_ROW if cfg is None else cfg, np.float32).reshape(-1, 2)
    assert len(a) in (1, rows)
    return np.ascontiguousarray(np.broadcast_to(a, (rows, 2)))


def _frames(x, nb):
    """x [R][500 + nb * 2000] -> [R][8 nb + 1][500], frame j of the call from sample 250 j of x"""
    return np.lib.stride_tricks.sliding_window_view(x, FRAME, axis=1)[:, ::HOP][:, :FRAMES * nb + 1]


def denoise_model(wave, cfg=None, state=None, enabled=None, nbatches=None, out=None):
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
    idx = np.flatnonzero(enabled)
    if not len(idx):
        return out, after
    cfgs = row_settings(cfg, rows)[idx]
    gmin = np.array([g_min(c[0]) for c in cfgs], np.float32)[:, None, None]
    over = cfgs[:, 1].astype(np.float32)[:, None, None]
    w = window()
    x = np.concatenate([state["x"][idx], wave[idx, :n]], axis=1)
    fr = _frames(x, nb)
    silent = (fr == 0).all(axis=-1)
    u = np.zeros(fr.shape[:2] + (FFT, 2), np.float32)
    u[..., :FRAME, 0] = fr * w
    X = fft512(u)
    re, im = X[..., :BINS, 0], X[..., :BINS, 1]
    rr = re * re
    ii = im * im
    P = rr + ii
    T = (P[..., LOWER] + P) + P[..., UPPER]
    S = np.zeros_like(T)
    S[:, 1:] = T[:, :-1] + T[:, 1:]
    counts = np.zeros(silent.shape, bool)
    counts[:, 1:] = ~silent[:, :-1] & ~silent[:, 1:]
    Sc = np.where(counts[..., None], S, np.float32(np.inf))
    M = Sc[:, 1:].reshape(len(idx), nb, FRAMES, BINS).min(axis=2)
    allM = np.concatenate([state["m"][idx], M], axis=1)
    m = np.lib.stride_tricks.sliding_window_view(allM, DEPTH, axis=1).min(axis=-1)  # [R][nb][257]
    with np.errstate(invalid="ignore"):
        N = np.where(np.isinf(m), np.float32(0.0), over * m)
    assert S.dtype == N.dtype == np.float32
    for b in range(nb):
        j0 = FRAMES * b
        Sb = S[:, j0:j0 + FRAMES + 1].copy()
        Sb[:, 0] = Sb[:, 1]  # the block's first frame takes S of the frame behind it
        Nb = np.broadcast_to(N[:, b:b + 1], Sb.shape)
        q = np.zeros_like(Sb)
        np.divide(Nb, Sb, out=q, where=Nb < Sb)
        g = np.where(Nb >= Sb, gmin, np.maximum(gmin, np.float32(1.0) - q))
        assert g.dtype == np.float32
        Y = X[:, j0:j0 + FRAMES + 1] * g[..., FOLD][..., None]
        Y[..., 1] = -Y[..., 1]
        z = fft512(Y)[..., 0] * np.float32(1.0 / FFT)
        v = z[..., :FRAME] * w
        y = v[:, :-1, HOP:] + v[:, 1:, :HOP]  # [R][8][250]: the older frame's second half, the newer one's first
        out[idx, b * WAVE_BATCH:(b + 1) * WAVE_BATCH] = np.clip(y.reshape(len(idx), WAVE_BATCH), np.float32(-1.0), np.float32(1.0))
    after["x"][idx] = wave[idx, n - FRAME:n]
    after["m"][idx] = allM[:, -(DEPTH - 1):]
    return out, after


def denoise_model64(wave, cfg=None, state=None, nbatches=None):
    """The same definition in float64 on numpy.fft.rfft / irfft, every row enabled: (out float64, the state after as (x, m) float64).
    state: (x [rows][500], m [rows][7][257]) or None."""
    wave = np.asarray(wave, np.float64)
    rows = wave.shape[0]
    nb = wave.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    n = nb * WAVE_BATCH
    sx, sm_ = (np.zeros((rows, FRAME)), np.full((rows, DEPTH - 1, BINS), np.inf)) if state is None else state
    cfgs = row_settings(cfg, rows).astype(np.float64)
    gmin = (10.0 ** (-cfgs[:, 0] / 20.0))[:, None, None]
    over = cfgs[:, 1][:, None, None]
    w = window64()
    x = np.concatenate([sx, wave[:, :n]], axis=1)
    fr = _frames(x, nb)
    silent = (fr == 0).all(axis=-1)
    X = np.fft.rfft(fr * w, FFT, axis=-1)
    P = X.real ** 2 + X.imag ** 2
    T = P[..., LOWER] + P + P[..., UPPER]
    S = np.zeros_like(T)
    S[:, 1:] = T[:, :-1] + T[:, 1:]
    counts = np.zeros(silent.shape, bool)
    counts[:, 1:] = ~silent[:, :-1] & ~silent[:, 1:]
    M = np.where(counts[..., None], S, np.inf)[:, 1:].reshape(rows, nb, FRAMES, BINS).min(axis=2)
    allM = np.concatenate([sm_, M], axis=1)
    m = np.lib.stride_tricks.sliding_window_view(allM, DEPTH, axis=1).min(axis=-1)
    N = np.where(np.isinf(m), 0.0, over * np.where(np.isinf(m), 0.0, m))
    out = np.zeros((rows, n))
    for b in range(nb):
        j0 = FRAMES * b
        Sb = S[:, j0:j0 + FRAMES + 1].copy()
        Sb[:, 0] = Sb[:, 1]
        Nb = np.broadcast_to(N[:, b:b + 1], Sb.shape)
        g = np.where(Nb >= Sb, gmin, np.maximum(gmin, 1.0 - Nb / np.where(Nb >= Sb, 1.0, Sb)))
        v = np.fft.irfft(X[:, j0:j0 + FRAMES + 1] * g, FFT, axis=-1)[..., :FRAME] * w
        out[:, b * WAVE_BATCH:(b + 1) * WAVE_BATCH] = np.clip((v[:, :-1, HOP:] + v[:, 1:, :HOP]).reshape(rows, WAVE_BATCH), -1.0, 1.0)
    return out, (wave[:, n - FRAME:n].copy(), allM[:, -(DEPTH - 1):].copy())


# ---------------- audio ----------------

NOISE_SIGMAS = (0.003, 0.03, 0.3)
TONE_HZ = 1000.0  # bin 32


def gaussian(rows, n, sigma, seed):
    """white Gaussian noise of standard deviation sigma, clipped into [-1, 1] (at 0.3 one sample in 1200 is)"""
    return np.clip(np.random.default_rng(seed).normal(0.0, sigma, (rows, n)), -1.0, 1.0).astype(np.float32)


def noise_at(level):
    def build(rows, nb, seed=0):
        return gaussian(rows, nb * WAVE_BATCH, NOISE_SIGMAS[level], 7000 + 10 * seed + level)
    return build


def tone_amplitude(sigma, db=10.0, seconds=1.0):
    """the amplitude of a steady sine whose P in its bin lies `db` above the mean P of white noise of deviation sigma: a frame's noise
    power per bin is sigma^2 sum w^2 = 250 sigma^2, the tone's (A sum w / 2)^2 with sum w = 500 * 2 / pi to a part in 10^6"""
    return math.sqrt(250.0 * sigma * sigma * 10.0 ** (db / 10.0)) * 2.0 / (FRAME * 2.0 / math.pi)


def tone_in_noise(rows, nb, seed=0, sigma=0.03):
    """a 1 kHz tone 10 dB above the noise in its bin"""
    t = np.arange(nb * WAVE_BATCH, dtype=np.float64) / WAVE_RATE
    rng = np.random.default_rng(7100 + seed)
    tone = np.stack([tone_amplitude(sigma) * np.sin(2 * np.pi * TONE_HZ * t + rng.uniform(0, 2 * np.pi)) for _ in range(rows)])
    return np.clip(tone + gaussian(rows, len(t), sigma, 7200 + seed), -1.0, 1.0).astype(np.float32)


def voice_in_noise(rows, nb, seed=0):
    """the voice band stage's voice-like tones at 0.8 of their level over noise of deviation 0.03"""
    return np.clip(0.8 * vm.voice_hum(rows, nb, seed).astype(np.float64) + gaussian(rows, nb * WAVE_BATCH, 0.03, 7300 + seed), -1.0, 1.0).astype(np.float32)


def gated_noise(rows, nb, seed=0):
    """noise of deviation 0.1 that starts and stops on frame and batch boundaries, other ones in every row: silent frames next to
    counting ones, frames that are half silence (not silent, and counting only beside another that is not), whole silent batches"""
    out = gaussian(rows, nb * WAVE_BATCH, 0.1, 7400 + seed)
    rng = np.random.default_rng(7500 + seed)
    for r in range(rows):
        edges = np.sort(rng.choice(np.arange(1, nb * FRAMES), min(6, nb * FRAMES - 1), replace=False)) * HOP
        if r % 2:
            edges = np.unique(np.concatenate([edges, np.arange(1, nb) * WAVE_BATCH]))
        on = r % 3 == 0
        for lo, hi in zip(np.concatenate([[0], edges]), np.concatenate([edges, [nb * WAVE_BATCH]])):
            if not on:
                out[r, lo:hi] = 0.0
            on = not on
    return out


TX_FIRST, TX_BATCHES = 10, 3


def tx_after_silence(rows, nb, seed=0):
    """a transmission of 3 batches (a 1 kHz tone in noise) after 10 of silence, silence behind it: whatever the handle held before has
    left the eight-batch window when the transmission opens, and its first batch has its own minimum as the only evidence"""
    out = np.zeros((rows, nb * WAVE_BATCH), np.float32)
    lo, hi = min(TX_FIRST, nb) * WAVE_BATCH, min(TX_FIRST + TX_BATCHES, nb) * WAVE_BATCH
    if hi > lo:
        out[:, lo:hi] = tone_in_noise(rows, TX_BATCHES, seed)[:, :hi - lo]
    return out


def stepping_noise(rows, nb, seed=0):
    """noise whose level steps down by 20 dB after a third of the call and up again after two thirds (0.1, 0.01, 0.1): m follows the
    step down at once and the step up only when the quiet batches leave the eight-batch window"""
    out = gaussian(rows, nb * WAVE_BATCH, 0.1, 7600 + seed)
    lo, hi = (nb // 3) * WAVE_BATCH, (2 * nb // 3) * WAVE_BATCH
    out[:, lo:hi] *= np.float32(0.1)
    return out


# The tests run a builder's audio with a last call of one batch behind everything else, so "the previous call" exists: lone_newest
# is the newest sample the state carries into the last call and lone_oldest the oldest, which only the last call's first frame holds.
BUILDERS = {"silence": vm.silence, "minus_zero": vm.minus_zero, "subnormal": vm.subnormal, "noise_lo": noise_at(0), "noise_mid": noise_at(1),
            "noise_hi": noise_at(2), "voice_in_noise": voice_in_noise, "tone_in_noise": tone_in_noise, "square": vm.square, "gated_noise": gated_noise,
            "tx_after_silence": tx_after_silence, "lone_0": vm.lone(0), "lone_249": vm.lone(249), "lone_250": vm.lone(250), "lone_1999": vm.lone(1999),
            "lone_newest": vm.lone(-WAVE_BATCH - 1), "lone_oldest": vm.lone(-WAVE_BATCH - FRAME), "stepping_noise": stepping_noise}


@functools.lru_cache(maxsize=None)
def audio(name, rows, nb, seed=0):
    a = BUILDERS[name](rows, nb, seed)
    assert a.dtype == np.float32 and a.shape == (rows, nb * WAVE_BATCH) and np.isfinite(a).all() and (np.abs(a) <= 1).all()
    a.setflags(write=False)
    return a


def level_db(x):
    """10 log10 of the mean square of x, in float64"""
    return 10.0 * math.log10(max(float(np.mean(np.asarray(x, np.float64) ** 2)), 1e-300))


def tone_level(x, hz=TONE_HZ):
    """amplitude of the `hz` component of x by float64 inner products over whole periods (hz divides 16000)"""
    period = int(WAVE_RATE / hz)
    span = len(x) // period * period
    t = np.arange(span, dtype=np.float64) / WAVE_RATE
    seg = np.asarray(x, np.float64)[:span]
    return float(np.hypot(seg @ np.sin(2 * np.pi * hz * t), seg @ np.cos(2 * np.pi * hz * t)) * 2 / span)
