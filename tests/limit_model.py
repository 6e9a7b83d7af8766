"""The peak limiter stage's definition (include/mi_airband.h "peak limiter stage") restated in numpy, and the audio its tests run on.

One float32 multiply and np.abs give a; p is np.max over a sliding_window_view of the row padded with the 1086 samples the state
carries; r is one float32 division under np.where; s is 64 sequential float32 array additions; then the multiply and np.clip.  A row
is one running sequence: the model limits the whole call in one go, where the device goes block by block.  Rows are independent, so
rows with the same samples, state and settings are computed once."""
import functools

import numpy as np

WAVE_BATCH, WAVE_RATE = 2000, 16000
LOOKAHEAD, WINDOW, HISTORY = 63, 1024, 1086
STATE = np.dtype([("x", "<f4", (HISTORY,))])
CEILING = np.float32(0.89125094)
DEFAULT_ROW = (np.float32(1.0), CEILING)
THREE_SETTINGS = [(1.0, float(CEILING)), (2.0, 0.5), (0.5, 0.0625)]
PREGAIN_MIN, PREGAIN_MAX, CEILING_MIN, CEILING_MAX = 2.0 ** -10, 2.0 ** 10, 0.0625, 1.0


def settings_ok(pregain, ceiling):
    return bool(np.isfinite(pregain) and np.isfinite(ceiling) and PREGAIN_MIN <= pregain <= PREGAIN_MAX and CEILING_MIN <= ceiling <= CEILING_MAX)


def fresh_state(rows):
    return np.zeros(rows, STATE)


def row_settings(cfg, rows):
    """None, one (pregain, ceiling) or one per row -> [(float32, float32)] * rows"""
    if cfg is None:
        cfg = DEFAULT_ROW
    a = np.asarray(cfg, np.float32).reshape(-1, 2)
    assert len(a) in (1, rows)
    return [(a[r if len(a) > 1 else 0][0], a[r if len(a) > 1 else 0][1]) for r in range(rows)]


def gains(x, pregain, ceiling):
    """x [1086 + n] float32, the call's samples behind the 1086 before them -> (u [63 + n] from the sample output 0 carries on,
    g [n]: the gain of every output)"""
    pregain, ceiling = np.float32(pregain), np.float32(ceiling)
    n = len(x) - HISTORY
    u = x * pregain
    a = np.abs(u)
    p = np.max(np.lib.stride_tricks.sliding_window_view(a, WINDOW), axis=-1)  # p[j]: the window that ends at a[1023 + j]
    with np.errstate(divide="ignore"):
        r = np.where(p > ceiling, ceiling / p, np.float32(1.0))  # r[j] is the gain value of sample j - 63 of the call
    s = np.zeros(n, np.float32)
    for k in range(LOOKAHEAD + 1):
        s = s + r[k:k + n]
    g = s * np.float32(0.015625)
    assert u.dtype == a.dtype == p.dtype == r.dtype == g.dtype == np.float32 and len(r) == n + LOOKAHEAD
    return u[HISTORY - LOOKAHEAD:], g


def limit_row(x, pregain, ceiling):
    u, g = gains(x, pregain, ceiling)
    c = np.float32(ceiling)
    y = u[:len(g)] * g
    assert y.dtype == np.float32
    return np.clip(y, -c, c)


def limit_model(wave, cfg=None, state=None, enabled=None, nbatches=None, out=None):
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
    seen = {}
    for r in range(rows):
        if not enabled[r]:
            continue
        x = np.concatenate([state["x"][r], wave[r, :n]])
        key = (x.tobytes(), cfgs[r][0].tobytes(), cfgs[r][1].tobytes())
        if key not in seen:
            seen[key] = limit_row(x, *cfgs[r])
        out[r, :n] = seen[key]
        after["x"][r] = wave[r, n - HISTORY:n]
    return out, after


# ---------------- audio ----------------
# Row r of every builder is row r % DISTINCT of it, so that many rows cost the model no more than five.
DISTINCT = 5


def silence(r, n, rng):
    return np.zeros(n, np.float32)


def minus_zero(r, n, rng):
    """-0.0 throughout: under the ceiling, so the output is -0.0 too"""
    return np.full(n, np.float32(-0.0))


def subnormal(r, n, rng):
    """values of subnormal size of both signs with a few of the smallest normal ones between them: a transparent block must carry
    these bit patterns through as they are"""
    bits = rng.integers(1, 1 << 23, n).astype(np.uint32)
    bits[::97] = 0x00800000  # 2^-126
    bits |= rng.integers(0, 2, n).astype(np.uint32) << 31
    return bits.view(np.float32)


def quiet_noise(r, n, rng):
    """uniform noise of +-0.85: under the default ceiling throughout"""
    return rng.uniform(-0.85, 0.85, n).astype(np.float32)


def loud_noise(r, n, rng):
    """uniform noise at three times the default ceiling: every window holds a peak"""
    return rng.uniform(-3.0 * float(CEILING), 3.0 * float(CEILING), n).astype(np.float32)


SQUARE_HALF_PERIODS = (25, 50, 7, 400, 100)


def square(r, n, rng):
    """a full-scale +-1 square wave; its settings put a pregain of 4 in front"""
    return np.where((np.arange(n) // SQUARE_HALF_PERIODS[r]) % 2 == 0, 1.0, -1.0).astype(np.float32)


def voice64(n, rng):
    """something like speech in float64, peak 0.7: harmonics of a wandering pitch under formant-like weights and a syllable envelope"""
    t = np.arange(n) / WAVE_RATE
    pitch = rng.uniform(100.0, 220.0) * (1.0 + 0.08 * np.sin(2 * np.pi * rng.uniform(0.5, 2.0) * t + rng.uniform(0, 6.28)))
    phase = 2 * np.pi * np.cumsum(pitch) / WAVE_RATE
    formants = rng.uniform([400, 1200, 2300], [800, 1800, 2900])
    x = np.zeros(n)
    for h in range(1, 16):
        f = h * float(pitch.mean())
        x += sum(np.exp(-((f - c) / 250.0) ** 2) for c in formants) * np.sin(h * phase + rng.uniform(0, 6.28))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.0, 5.0) * t + rng.uniform(0, 6.28))
    x *= env
    return 0.7 * x / np.abs(x).max()


def voice(r, n, rng):
    return voice64(n, rng).astype(np.float32)


def four_voices(r, n, rng):
    """what a mixer with four inputs open at once writes: the sum of four voices, scaled to reach 2.5"""
    x = sum(voice64(n, rng) for _ in range(4))
    return (2.5 * x / np.abs(x).max()).astype(np.float32)


TONE_HZ = 1000.0


def loud_tone(r, n, rng):
    """a steady 1 kHz tone at twice the default ceiling: one period of 16 samples, repeated as it is"""
    period = int(WAVE_RATE / TONE_HZ)
    one = (2.0 * float(CEILING) * np.sin(2 * np.pi * np.arange(period) / period + 0.3 * r)).astype(np.float32)
    return np.tile(one, n // period)


BED_LOW, BED_HIGH, PEAK = 0.05, 0.3, np.float32(2.0)


def bed(n, rng):
    """a background that is never zero and far under every ceiling the tests set for it: a gain shows as out / in at every sample"""
    return (rng.uniform(BED_LOW, BED_HIGH, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def lone(*samples, value=PEAK):
    """the bed but for `value` at each of `samples` (negative: counted from the end of the audio)"""
    def build(r, n, rng):
        out = bed(n, rng)
        for s in samples:
            out[s] = value if (s + r) % 2 == 0 else -value
        return out
    return build


# The tests run a builder's audio with a last call of one batch behind everything else, so "the previous call" exists: the newest
# sample the state carries into that call is sample -2001, the k-th counting back is -2000 - k, and sample -2000 - 1087 is one beyond
# the history, with no effect on the last call.  Positive indices are in the first block.
LAST = -WAVE_BATCH
BUILDERS = {
    "silence": silence, "minus_zero": minus_zero, "subnormal": subnormal, "quiet_noise": quiet_noise, "loud_noise": loud_noise, "square": square,
    "voice": voice, "four_voices": four_voices, "loud_tone": loud_tone,
    "at_ceiling": lone(700, 2300, value=CEILING), "step_over_ceiling": lone(700, 2300, value=np.nextafter(CEILING, np.float32(2.0))),
    "peaks_64_apart": lone(900, 964), "peaks_1024_apart": lone(500, 1524),
    "lone_0": lone(0), "lone_62": lone(62), "lone_63": lone(63), "lone_64": lone(64), "lone_1936": lone(WAVE_BATCH - 1 - LOOKAHEAD), "lone_1999": lone(WAVE_BATCH - 1),
    "carried_1": lone(LAST - 1), "carried_63": lone(LAST - 63), "carried_1023": lone(LAST - 1023), "carried_1024": lone(LAST - 1024),
    "carried_1086": lone(LAST - HISTORY), "beyond_history": lone(LAST - HISTORY - 1),
}
SETTINGS = {"square": (4.0, float(CEILING))}  # a builder's own settings where they are not the default row's
UNDER_CEILING = ("silence", "minus_zero", "subnormal", "quiet_noise", "voice", "at_ceiling")  # at their own settings: transparent
LONE_PEAKS = {"lone_0": 0, "lone_62": 62, "lone_63": 63, "lone_64": 64, "lone_1936": 1936, "lone_1999": 1999}  # builder -> q


def own_settings(name):
    return SETTINGS.get(name, (1.0, float(CEILING)))


def settings_for(name, rows, kind):
    """the builder's own settings on every row, three settings in turn, or one per row (seven of them in turn)"""
    if kind == "one":
        return [own_settings(name)] * rows
    if kind == "three":
        return [THREE_SETTINGS[r % 3] for r in range(rows)]
    return [(0.5 + 0.25 * (r % 7), 0.3 + 0.1 * (r % 7)) for r in range(rows)]


@functools.lru_cache(maxsize=None)
def audio(name, rows, nb, seed=0):
    n = nb * WAVE_BATCH
    names = list(BUILDERS)
    base = [BUILDERS[name](r, n, np.random.default_rng([names.index(name), r, nb, seed])) for r in range(min(rows, DISTINCT))]
    a = np.stack([base[r % DISTINCT] for r in range(rows)])
    assert a.dtype == np.float32 and a.shape == (rows, n) and np.isfinite(a).all()
    a.setflags(write=False)
    return a
