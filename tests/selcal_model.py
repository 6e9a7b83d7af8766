"""The SELCAL decoder stage (mi_selcal_*, csrc/selcal.hip; definition in include/mi_airband.h "SELCAL decoder stage") restated in numpy,
and the seeded audio its tests share.

The window comes from its formula; every window's y, energy, recurrence, powers and decision are float32 array operations in the
order the header states, vectorised over windows and tones and sequential over the 2000 samples; the decoder is plain Python written
from the header's table, not from the library's text.  Records and the state blob are built as the bytes the library writes."""
import math

import numpy as np

WAVE_BATCH, RATE = 2000, 16000
WINDOW, HOP, HISTORY, MAX_TONES = 2000, 1000, 1002, 32
NONE, NONE8 = 0, 0xFF
IDLE, FIRST, OVER, GAP, SECOND, DONE = range(6)
MODE_16, MODE_32, MODE_CUSTOM = 0, 1, 2
F32 = np.float32

WINDOW_REC = np.dtype([("best", "u1"), ("second", "u1"), ("third", "u1"), ("zero", "u1"), ("p_best", "<f4"), ("p_second", "<f4"), ("p_third", "<f4"),
                       ("energy", "<f4"), ("pair", "<u4")])
CODE_REC = np.dtype([("row", "<u4"), ("seq", "<u4"), ("tone", "u1", (4,)), ("first_window", "<u4"), ("last_window", "<u4"), ("run1", "<u4"),
                     ("gap", "<u4"), ("batch", "<u4")])
STATE = np.dtype([("x", "<f4", (HISTORY,)), ("window", "<u4"), ("seq", "<u4"), ("phase", "<u4"), ("pair1", "<u4"), ("pair2", "<u4"), ("run1", "<u4"),
                  ("run2", "<u4"), ("gap", "<u4"), ("first_window", "<u4"), ("zero", "<u4")])

# The literals of the header, in ascending frequency: the classic sixteen are the even positions.
HZ_32 = [312.6, 329.2, 346.7, 365.2, 384.6, 405.0, 426.6, 449.3, 473.2, 498.3, 524.8, 552.7, 582.1, 613.1, 645.7, 680.0, 716.1, 754.2, 794.3, 836.6, 881.0,
         927.9, 977.2, 1029.2, 1083.9, 1141.6, 1202.3, 1266.2, 1333.5, 1404.4, 1479.1, 1557.8]
LETTERS_32 = "ATBUCVDWEXFYGZH1J2K3L4M5P6Q7R8S9"
HZ_16, LETTERS_16 = HZ_32[::2], LETTERS_32[::2]
DEFAULTS = dict(min_energy=1e-3, min_tonality=0.5, max_twist=8.0, min_separation=4.0, min_run=8, max_run=22, max_gap=8)


def table(mode=MODE_16, freq=None):
    """(freq float32 [n], letters) of a mode"""
    if mode == MODE_CUSTOM:
        return np.array(freq, F32), "?" * len(freq)
    return (np.array(HZ_16, F32), LETTERS_16) if mode == MODE_16 else (np.array(HZ_32, F32), LETTERS_32)


def coeffs(freq):
    return (2.0 * np.cos(2.0 * np.pi * np.asarray(freq, F32).astype(np.float64) / RATE)).astype(F32)


def hann():
    """w[j] = 0.5 - 0.5 cos(2 pi j / 1999) in float64 for j <= 999, cast, and mirrored"""
    half = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WINDOW // 2) / (WINDOW - 1))).astype(F32)
    return np.concatenate([half, half[::-1]])


def tonality_constant(w):
    sw = sw2 = 0.0
    for v in w.astype(np.float64):
        sw += v
        sw2 += v * v
    return F32(sw * sw / (2.0 * sw2))


def settings(**kw):
    s = dict(DEFAULTS)
    s.update({k: v for k, v in kw.items() if v})
    return s


def fresh_state(rows):
    return np.zeros(rows, STATE)


def window_records(frames, coeff, s):
    """frames: float32 [n][2000] -> WINDOW_REC [n] and the powers [n][ntones] (items 0 .. 4 of the header)"""
    w = hann()
    n, nt = frames.shape[0], len(coeff)
    y = frames.astype(F32) * w
    y2 = np.zeros((n, 32 * 64), F32)
    y2[:, :WINDOW] = y * y
    y2 = y2.reshape(n, 32, 64)  # [.., k, l] = the k-th term of s_l; the 48 that do not exist are +0, which changes no sum of squares
    e = y2[:, 0, :].copy()
    for k in range(1, 32):
        e = e + y2[:, k, :]
    for h in (32, 16, 8, 4, 2, 1):
        e = e[:, :h] + e[:, h:2 * h]
    e = e[:, 0]
    p = np.zeros((n, nt), F32)
    live = np.flatnonzero(e != 0)  # a silent window's powers are zero by definition
    if live.size:
        c = coeff[None, :]
        yl = np.ascontiguousarray(y[live].T)  # [2000][live]
        q1 = np.zeros((live.size, nt), F32)
        q2 = np.zeros((live.size, nt), F32)
        for j in range(WINDOW):
            q0 = c * q1 - q2 + yl[j][:, None]
            q2 = q1
            q1 = q0
        p[live] = q1 * q1 + q2 * q2 - q1 * q2 * c
    order = np.argsort(-p, axis=1, kind="stable")[:, :3]
    rec = np.zeros(n, WINDOW_REC)
    rows = np.arange(n)
    rec["best"], rec["second"] = order[:, 0], order[:, 1]
    pb, ps = p[rows, order[:, 0]], p[rows, order[:, 1]]
    if nt > 2:
        rec["third"], pt = order[:, 2], p[rows, order[:, 2]]
    else:
        rec["third"], pt = NONE8, np.zeros(n, F32)
    rec["p_best"], rec["p_second"], rec["p_third"], rec["energy"] = pb, ps, pt, e
    tc = F32(s["min_tonality"]) * tonality_constant(w)
    named = (e >= F32(s["min_energy"])) & (pb + ps >= tc * e) & (pb <= F32(s["max_twist"]) * ps) & (ps >= F32(s["min_separation"]) * pt)
    lo, hi = np.minimum(order[:, 0], order[:, 1]).astype(np.uint32), np.maximum(order[:, 0], order[:, 1]).astype(np.uint32)
    rec["pair"] = np.where(named, lo | hi << 8, NONE)
    return rec, p


class Decoder:
    """The header's table, one row.  feed(pair, n) -> True when window n emits a code."""

    def __init__(self, st, s):
        self.phase, self.pair1, self.pair2, self.run1, self.run2, self.gap, self.first = (int(st[k]) for k in ("phase", "pair1", "pair2", "run1", "run2", "gap",
                                                                                                                 "first_window"))
        self.s = s

    def idle(self, pair, n):
        self.phase, self.pair1, self.pair2, self.run1, self.run2, self.gap, self.first = IDLE, NONE, NONE, 0, 0, 0, 0
        if pair != NONE:
            self.phase, self.pair1, self.run1, self.first = FIRST, pair, 1, n

    def overlong(self):
        if self.run1 > self.s["max_run"]:
            self.phase, self.run1 = OVER, self.s["max_run"] + 1

    def feed(self, pair, n):
        s = self.s
        if self.phase == IDLE:
            self.idle(pair, n)
        elif self.phase == FIRST:
            if pair != NONE and pair == self.pair1:
                self.run1 += 1
                self.overlong()
            elif self.run1 < s["min_run"]:
                self.idle(pair, n)
            elif pair != NONE:
                self.phase, self.pair2, self.run2 = SECOND, pair, 1
            else:
                self.phase, self.gap = GAP, 1
        elif self.phase == OVER:
            if pair != self.pair1:
                self.idle(pair, n)
        elif self.phase == GAP:
            if pair == NONE:
                self.gap += 1
                if self.gap > s["max_gap"]:
                    self.idle(pair, n)
            elif pair == self.pair1:
                self.phase, self.run1, self.gap = FIRST, self.run1 + self.gap + 1, 0
                self.overlong()
            else:
                self.phase, self.pair2, self.run2 = SECOND, pair, 1
        elif self.phase == SECOND:
            if pair != NONE and pair == self.pair2:
                self.run2 += 1
                if self.run2 == s["min_run"]:
                    self.phase = DONE
                    return True
            else:
                self.idle(pair, n)
        else:  # DONE
            if pair != self.pair2:
                self.idle(pair, n)
        return False


def selcal_model(plane, state=None, enabled=None, mode=MODE_16, freq=None, **kw):
    """One call over plane float32 [rows][nb * 2000] -> (codes CODE_REC [k], windows WINDOW_REC [rows][2 nb] (zeros in a disabled row),
    row_first [rows + 1], state after)"""
    plane = np.asarray(plane, F32)
    rows, nb = plane.shape[0], plane.shape[1] // WAVE_BATCH
    s = settings(**kw)
    state = fresh_state(rows) if state is None else state.copy()
    enabled = np.ones(rows, bool) if enabled is None else np.asarray(enabled, bool)
    coeff = coeffs(table(mode, freq)[0])
    on = np.flatnonzero(enabled)
    windows = np.zeros((rows, 2 * nb), WINDOW_REC)
    if on.size:
        x = np.concatenate([state["x"][on][:, HISTORY - HOP:], plane[on, :nb * WAVE_BATCH]], axis=1)
        frames = np.lib.stride_tricks.sliding_window_view(x, WINDOW, axis=1)[:, ::HOP]
        assert frames.shape[1] == 2 * nb
        windows[on] = window_records(frames.reshape(-1, WINDOW), coeff, s)[0].reshape(on.size, 2 * nb)
    codes, row_first = [], np.zeros(rows + 1, np.uint32)
    for r in range(rows):
        row_first[r] = len(codes)
        if not enabled[r]:
            continue
        st = state[r]
        d, n0 = Decoder(st, s), int(st["window"])
        for i in range(2 * nb):
            n = (n0 + i) & 0xFFFFFFFF
            if d.feed(int(windows[r, i]["pair"]), n):
                codes.append((r, int(st["seq"]), (d.pair1 & 0xFF, d.pair1 >> 8, d.pair2 & 0xFF, d.pair2 >> 8), d.first, n, d.run1, d.gap, i // 2))
                st["seq"] = (int(st["seq"]) + 1) & 0xFFFFFFFF
        st["window"] = (n0 + 2 * nb) & 0xFFFFFFFF
        st["phase"], st["pair1"], st["pair2"], st["run1"], st["run2"], st["gap"], st["first_window"] = d.phase, d.pair1, d.pair2, d.run1, d.run2, d.gap, d.first
        st["x"] = plane[r, nb * WAVE_BATCH - HISTORY:nb * WAVE_BATCH]
    row_first[rows] = len(codes)
    return np.array(codes, CODE_REC) if codes else np.zeros(0, CODE_REC), windows, row_first, state


def run_in_calls(plane, cuts, masks=None, **kw):
    """consecutive calls of the lengths `cuts` over the plane: [(codes, windows, row_first, state after)] per call"""
    out, state, done = [], None, 0
    for i, n in enumerate(cuts):
        got = selcal_model(plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], state, None if masks is None else masks[i], **kw)
        out.append(got)
        state, done = got[3], done + n
    return out


def code_text(tones, mode=MODE_16):
    letters = table(mode, [0] * 32)[1]
    return letters[tones[0]] + letters[tones[1]] + "-" + letters[tones[2]] + letters[tones[3]]


# ---------------- seeded audio ----------------
NB = 24  # batches of every builder's rows: 3 s


def tones_at(n, start, length, freqs, amp, rng, ramp=32):
    """`length` samples of the sum of sines at freqs, each of amplitude amp and a drawn phase, from sample `start` of n; a raised-cosine
    edge of `ramp` samples keeps the keying click small"""
    out = np.zeros(n)
    length = min(length, n - start)  # (a pulse the row ends in is cut there)
    t = np.arange(length)
    env = np.ones(length)
    if ramp:
        env[:ramp] = 0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)
        env[-ramp:] = env[:ramp][::-1]
    for f in freqs:
        out[start:start + length] += amp * env * np.sin(2.0 * np.pi * f * t / RATE + rng.uniform(0, 2 * np.pi))
    return out


def code_row(pair1, pair2, hz, start=WAVE_BATCH, pulse=16000, gap=3200, amp=0.25, seed=1, n=NB * WAVE_BATCH, amp2=None):
    """one SELCAL call: tones hz[pair1] for `pulse` samples from `start`, `gap` samples of silence, tones hz[pair2] for `pulse`"""
    rng = np.random.default_rng(seed)
    x = tones_at(n, start, pulse, [hz[i] for i in pair1], amp, rng)
    if pair2 is not None:
        x += tones_at(n, start + pulse + gap, pulse, [hz[i] for i in pair2], amp, rng)
    if amp2 is not None:  # twist: the lower tone of the first pulse at another level
        x += tones_at(n, start, pulse, [hz[pair1[0]]], amp2 - amp, np.random.default_rng(seed))
    return x


def noise(n, sigma, seed):
    return np.random.default_rng(seed).normal(0.0, sigma, n)


def voice_like(n, seed):
    """harmonics of a gliding pitch under a formant-like tilt, keyed in syllables at about 4 Hz"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    x = sum(np.sin(k * ph + rng.uniform(0, 6.28)) / (1.0 + abs(k * 140.0 - 700.0) / 300.0) for k in range(1, 20))
    syll = np.clip(np.sin(2 * np.pi * 4.1 * t + rng.uniform(0, 6.28)) + 0.3, 0.0, 1.0)
    return 0.1 * x * syll


def square(n, f, amp=1.0):
    return amp * np.where(np.sin(2 * np.pi * f * np.arange(n) / RATE) >= 0, 1.0, -1.0)


NOISE_SNR_DB = 6.0  # tools/selcal_classes.py: every code decodes down to 1 dB (both tones' power over white noise's, full band); this is 5 dB above


def builders(mode=MODE_16):
    """[(name, row float64 [NB * 2000], expected code texts)] -- one row each; a positive has one text, a negative none"""
    hz, letters = table(mode)
    hz = hz.astype(np.float64)
    nt, n = len(hz), NB * WAVE_BATCH
    out = []

    def add(name, x, pairs=None):
        want = [] if pairs is None else [code_text((*pairs[0], *pairs[1]), mode)]
        out.append((name, x, want))

    for k in range(nt // 4):  # every tone of the table in one pulse: adjacent tones, the closest a pair gets
        p1, p2 = (4 * k, 4 * k + 1), (4 * k + 2, 4 * k + 3)
        add(f"tones {4 * k}..{4 * k + 3}", code_row(p1, p2, hz, seed=10 + k), (p1, p2))
    far1, far2 = (0, nt - 1), (1, nt // 2)
    add("pulses of 0.75 s", code_row(far1, far2, hz, pulse=12000, seed=30), (far1, far2))
    add("pulses of 1.25 s", code_row(far1, far2, hz, pulse=20000, gap=1600, start=WAVE_BATCH + 1, seed=31), (far1, far2))
    add("a gap of 0.1 s", code_row(far1, far2, hz, gap=1600, seed=32), (far1, far2))
    add("a gap of 0.3 s", code_row(far1, far2, hz, gap=4800, seed=33), (far1, far2))
    for off in (0, 1, 999, 1000, 1999):
        add(f"offset {off}", code_row((2, 5), (3, 7), hz, start=WAVE_BATCH + off, seed=40 + off), ((2, 5), (3, 7)))
    x = code_row((1, 6), (0, 4), hz, seed=50)
    x[WAVE_BATCH + 10000:WAVE_BATCH + 12000] = 0.0  # two windows without the pair inside the first pulse, behind min_run of it
    add("a dropout inside the first pulse", x, ((1, 6), (0, 4)))
    add("a twist of 6 dB", code_row((0, 9), (3, 8), hz, seed=51, amp2=0.125), ((0, 9), (3, 8)))
    sig = code_row((2, 11), (5, 13), hz, seed=52)
    sigma = math.sqrt(0.25 ** 2 / 10 ** (NOISE_SNR_DB / 10))  # both tones' power is amp^2
    add("a code in noise", sig + noise(n, sigma, 53), ((2, 11), (5, 13)))
    # negatives
    add("one tone only", code_row((4,), (9,), hz, seed=60))
    add("one pulse only", code_row((4, 8), None, hz, seed=61))
    add("the same pair twice", code_row((4, 8), (4, 8), hz, seed=62))
    add("an overlong pulse", code_row((4, 8), (5, 9), hz, pulse=28000, gap=1600, seed=63))
    add("a gap beyond max_gap", code_row((4, 8), (5, 9), hz, pulse=14000, gap=12000, seed=64))
    add("silence", np.zeros(n))
    add("-0.0 throughout", np.full(n, -0.0))
    add("subnormal values", np.random.default_rng(65).choice([1e-40, -3e-41, 1e-45, 0.0, 2e-39], n))
    add("white noise", noise(n, 0.2, 66))
    add("voice-like", voice_like(n, 67))
    add("a full-scale square wave", square(n, 400.0))
    return out


def stacked(mode=MODE_16):
    """(names, plane float32 [rows][NB * 2000], expected texts per row) of a mode's builders"""
    b = builders(mode)
    return [x[0] for x in b], np.stack([x[1][:NB * WAVE_BATCH] for x in b]).astype(F32), [x[2] for x in b]


# ---------------- end to end: a call on an AM carrier, as u8 I/Q ----------------
E2E_BATCHES, E2E_CODE, E2E_TONES = 30, "CM-FQ", ((2, 11), (5, 13))


def e2e_setup(pkg):
    """One stream, one AM channel five bins above the centre at fft 512, 2.56 Msps.  The carrier is up from the start and the call
    begins a second later, so the squelch is open when it does: (dev, chans, iq uint8, batches)."""
    from common import AGC_EXTRA
    rate, centre = 2560000, 120000000
    dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9)
    chans = [pkg.channel_cfg(centre + 25000, modulation=pkg.MOD_AM)]
    hop = rate // RATE
    n_audio = E2E_BATCHES * WAVE_BATCH + AGC_EXTRA + 8
    audio = code_row(*E2E_TONES, np.array(HZ_16), start=RATE, amp=0.3, seed=70, n=n_audio)
    n = n_audio * hop
    rng = np.random.default_rng(71)
    env = np.repeat(1.0 + audio, hop).astype(np.float32)
    ph = (2.0 * np.pi * 25000.0 / rate) * (np.arange(n) % (rate // 5000))  # (the offset's period is 512 samples: no phase grows large)
    z = 30.0 * env * np.exp(1j * ph).astype(np.complex64)
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    iq += rng.normal(0.0, 1.5, 2 * n).astype(np.float32)
    return dev, chans, np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8), E2E_BATCHES


SHORT = dict(min_run=2, max_run=3, max_gap=1)


def short_codes(rows=6, nb=18):
    """rows of three short calls each (pulses of 0.2 s) for the settings SHORT: up to three codes a row and call.  Where a pulse
    falls so that four windows name it, it is overlong under SHORT, and in the odd rows the gaps are over max_gap: calls that must
    not decode, between ones that must."""
    hz = np.array(HZ_16)
    out = []
    for r in range(rows):
        x = np.zeros(nb * WAVE_BATCH)
        for k in range(3):
            x += code_row((r, r + 4), (r + 1, r + 7), hz, start=1000 + 12000 * k + 37 * r, pulse=3200, gap=800 + 3400 * (r % 2), seed=80 + 3 * r + k, n=x.size)
        out.append(x)
    return np.stack(out).astype(F32)
