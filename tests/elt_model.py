"""The ELT detector stage (mi_elt_*, csrc/elt.hip; definition in include/mi_airband.h "ELT detector stage") restated in numpy and plain
Python, and the seeded audio its tests share.

The window and the coefficients come from their formulas; every frame's y, energy, recurrence, powers and decision are float32 array
operations in the order the header states, vectorised over frames and bins and sequential over the 256 samples; the walker is plain
Python integers written from the header's rules, not from the library's text.  Records and the state blob are built as the bytes the
library writes."""
import numpy as np

WAVE_BATCH, RATE = 2000, 16000
FRAME, HOP, HISTORY, FRAMES, BINS, BIN0 = 256, 80, 178, 25, 32, 2
BACK = FRAME - HOP  # 176: the samples of a batch's first frame that lie before the batch
NONE8 = 0xFF
ONSET, END = 1, 2
UP, DOWN = 1, 2
M32 = 0xFFFFFFFF
F32 = np.float32

FRAME_REC = np.dtype([("best", "u1"), ("bin", "u1"), ("zero", "<u2"), ("energy", "<f4"), ("p_best", "<f4"), ("p3", "<f4")])
EVENT_REC = np.dtype([("row", "<u4"), ("seq", "<u4"), ("kind", "u1"), ("dir", "u1"), ("bin_from", "u1"), ("bin_to", "u1"), ("frame", "<u4"),
                      ("first_frame", "<u4"), ("last_end", "<u4"), ("sweeps", "<u4"), ("batch", "<u4")])
WALKER_FIELDS = ("open", "start", "first_bin", "last_bin", "last_frame", "dir", "drops", "count", "chain_dir", "chain_first", "last_end", "alarmed",
                 "bin_from", "bin_to")
STATE = np.dtype([("x", "<f4", (HISTORY,)), ("frame", "<u4"), ("seq", "<u4")] + [(n, "<u4") for n in WALKER_FIELDS])
DEFAULTS = dict(min_energy=1e-4, min_tonality=0.5, band_lo=4, band_hi=26, min_span=10, min_len=40, max_len=120, max_step=3, max_drop=2, max_gap=10,
                min_sweeps=6)


def hann():
    """w[j] = 0.5 - 0.5 cos(2 pi j / 255) in float64 for j <= 127, cast, and mirrored"""
    half = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME // 2) / (FRAME - 1))).astype(F32)
    return np.concatenate([half, half[::-1]])


def coeffs():
    return (2.0 * np.cos(2.0 * np.pi * np.arange(BIN0, BIN0 + BINS) / FRAME)).astype(F32)


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


def max_events(nb, s=DEFAULTS):
    return 2 * (1 + (FRAMES * nb - 1) // (s["min_sweeps"] * s["min_len"])) + 1


def fresh_state(rows):
    return np.zeros(rows, STATE)


def frame_records(frames, s):
    """frames: float32 [n][256] -> FRAME_REC [n] and the powers [n][32] (items 0 .. 4 of the header)"""
    w, c = hann(), coeffs()[None, :]
    n = frames.shape[0]
    y = frames.astype(F32) * w
    y2 = (y * y).reshape(n, 4, 64)  # [.., k, l] = the k-th term of s_l
    e = y2[:, 0, :].copy()
    for k in range(1, 4):
        e = e + y2[:, k, :]
    for h in (32, 16, 8, 4, 2, 1):
        e = e[:, :h] + e[:, h:2 * h]
    e = e[:, 0]
    p = np.zeros((n, BINS), F32)
    live = np.flatnonzero(e != 0)  # a silent frame's powers are zero by definition
    if live.size:
        yl = np.ascontiguousarray(y[live].T)  # [256][live]
        q1 = np.zeros((live.size, BINS), F32)
        q2 = np.zeros((live.size, BINS), F32)
        for j in range(FRAME):
            q0 = c * q1 - q2 + yl[j][:, None]
            q2 = q1
            q1 = q0
        p[live] = q1 * q1 + q2 * q2 - q1 * q2 * c
    best = np.argmax(p, axis=1)  # (the first of equal maxima: the lowest bin)
    rows = np.arange(n)
    pad = np.zeros((n, BINS + 2), F32)
    pad[:, 1:-1] = p
    pb = p[rows, best]
    p3 = (pad[rows, best] + pb) + pad[rows, best + 2]
    tc = F32(s["min_tonality"]) * tonality_constant(w)
    bins = best + BIN0
    tonal = (e >= F32(s["min_energy"])) & (p3 >= tc * e) & (bins >= s["band_lo"]) & (bins <= s["band_hi"])
    rec = np.zeros(n, FRAME_REC)
    rec["best"], rec["bin"], rec["energy"], rec["p_best"], rec["p3"] = bins, np.where(tonal, bins, NONE8), e, pb, p3
    return rec, p


class Walker:
    """The header's rules, one row.  feed(b, f) -> what frame f emits, in order: (kind, and the chain's fields as the record takes them)."""

    def __init__(self, st, s):
        for k in WALKER_FIELDS:
            setattr(self, k, int(st[k]))
        self.s = s
        self.closed, self.steps = [], []  # (measurement only) every closed segment as (start, last_frame, first_bin, last_bin, dir, valid, start - last_end
        #                                   of a valid one that met a chain, else None); every following step as (|step|, drops before it)

    def store(self, st):
        for k in WALKER_FIELDS:
            st[k] = getattr(self, k)

    def _emit(self, kind, out):
        out.append((kind, self.chain_dir, self.bin_from, self.bin_to, self.chain_first, self.last_end, self.count))

    def _close(self, out):
        s = self.s
        length = (self.last_frame - self.start + 1) & M32
        valid = self.dir != 0 and abs(self.first_bin - self.last_bin) >= s["min_span"] and s["min_len"] <= length <= s["max_len"]
        self.closed.append((self.start, self.last_frame, self.first_bin, self.last_bin, self.dir, valid,
                            (self.start - self.last_end) & M32 if valid and self.count > 0 else None))
        if self.dir != 0 and abs(self.first_bin - self.last_bin) >= s["min_span"] and s["min_len"] <= length <= s["max_len"]:
            if self.count > 0 and ((self.start - self.last_end) & M32) <= s["max_gap"] and self.dir == self.chain_dir:
                self.count += 1
            else:
                if self.alarmed:  # decided: a chain that begins while an alarmed one stands ends that one first
                    self._emit(END, out)
                    self.alarmed = 0
                self.count, self.chain_first, self.chain_dir = 1, self.start, self.dir
            self.last_end, self.bin_from, self.bin_to = self.last_frame, self.first_bin, self.last_bin
            if not self.alarmed and self.count >= s["min_sweeps"]:
                self.alarmed = 1
                self._emit(ONSET, out)
        self.open = self.start = self.first_bin = self.last_bin = self.last_frame = self.dir = self.drops = 0

    def _open(self, b, f):
        self.open, self.start, self.last_frame, self.first_bin, self.last_bin, self.dir, self.drops = 1, f, f, b, b, 0, 0

    def feed(self, b, f):
        s, out = self.s, []
        if b != NONE8:
            if not self.open:
                self._open(b, f)
            else:
                step = b - self.last_bin
                sd = UP if step > 0 else DOWN if step < 0 else 0
                if abs(step) <= s["max_step"] * (1 + self.drops) and (sd == 0 or self.dir == 0 or sd == self.dir):
                    if self.dir == 0:
                        self.dir = sd
                    self.steps.append((abs(step), self.drops))
                    self.last_bin, self.last_frame, self.drops = b, f, 0
                else:
                    self._close(out)
                    self._open(b, f)
        elif self.open:
            self.drops += 1
            if self.drops > s["max_drop"]:
                self._close(out)
        if self.count > 0:
            alive = ((f - self.last_end) & M32) <= s["max_gap"] or (self.open and ((self.start - self.last_end) & M32) <= s["max_gap"] and
                                                                  ((f - self.start + 1) & M32) <= s["max_len"])
            if not alive:
                if self.alarmed:
                    self._emit(END, out)
                self.count = self.chain_dir = self.chain_first = self.last_end = self.alarmed = self.bin_from = self.bin_to = 0
        return out


def walk(decisions, st, s, row=0):
    """the walker over one row's decisions from the state record st (updated): [event tuples in EVENT_REC's order]"""
    wk, f0, events = Walker(st, s), int(st["frame"]), []
    for i, b in enumerate(decisions):
        f = (f0 + i) & M32
        for kind, cdir, b_from, b_to, first, last_end, count in wk.feed(int(b), f):
            events.append((row, int(st["seq"]), kind, cdir, b_from, b_to, f, first, last_end, count, i // FRAMES))
            st["seq"] = (int(st["seq"]) + 1) & M32
    st["frame"] = (f0 + len(decisions)) & M32
    wk.store(st)
    return events


def elt_model(plane, state=None, enabled=None, **kw):
    """One call over plane float32 [rows][nb * 2000] -> (events EVENT_REC [k], frames FRAME_REC [rows][25 nb] (zeros in a disabled row),
    row_first [rows + 1], state after)"""
    plane = np.asarray(plane, F32)
    rows, nb = plane.shape[0], plane.shape[1] // WAVE_BATCH
    s = settings(**kw)
    state = fresh_state(rows) if state is None else state.copy()
    enabled = np.ones(rows, bool) if enabled is None else np.asarray(enabled, bool)
    on = np.flatnonzero(enabled)
    frames = np.zeros((rows, FRAMES * nb), FRAME_REC)
    if on.size:
        x = np.concatenate([state["x"][on][:, HISTORY - BACK:], plane[on, :nb * WAVE_BATCH]], axis=1)
        fr = np.lib.stride_tricks.sliding_window_view(x, FRAME, axis=1)[:, ::HOP]
        assert fr.shape[1] == FRAMES * nb
        frames[on] = frame_records(fr.reshape(-1, FRAME), s)[0].reshape(on.size, FRAMES * nb)
    events, row_first = [], np.zeros(rows + 1, np.uint32)
    for r in range(rows):
        row_first[r] = len(events)
        if not enabled[r]:
            continue
        events += walk(frames[r]["bin"], state[r], s, r)
        state[r]["x"] = plane[r, nb * WAVE_BATCH - HISTORY:nb * WAVE_BATCH]
    row_first[rows] = len(events)
    return np.array(events, EVENT_REC) if events else np.zeros(0, EVENT_REC), frames, row_first, state


def run_in_calls(plane, cuts, masks=None, state=None, **kw):
    """consecutive calls of the lengths `cuts` over the plane: [(events, frames, row_first, state after)] per call"""
    out, done = [], 0
    for i, n in enumerate(cuts):
        got = elt_model(plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], state, None if masks is None else masks[i], **kw)
        out.append(got)
        state, done = got[3], done + n
    return out


def event_text(e):
    return "%s %s %.1f -> %.1f Hz, %d sweeps, %.3f s" % ("ONSET" if e["kind"] == ONSET else "END", "up" if e["dir"] == UP else "down", 62.5 * e["bin_from"],
                                                        62.5 * e["bin_to"], e["sweeps"], 0.005 * ((int(e["frame"]) - int(e["first_frame"])) & M32))


# ---------------- seeded audio ----------------
NB = 48  # batches of every builder's rows: 6 s


def beacon(n, rate=3.0, f_hi=1500.0, f_lo=500.0, down=True, start=0, stop=None, amp=0.3, sigma=0.0, seed=1, flyback=0.0):
    """A float64 phase-continuous swept tone over samples start .. stop of n: `rate` sweeps a second between f_hi and f_lo, downward or
    upward, each sweep followed by `flyback` seconds of linear return (0: a jump), over seeded white noise of deviation sigma."""
    stop = n if stop is None else stop
    t = np.arange(max(stop - start, 0)) / RATE
    period = 1.0 / rate
    u = np.mod(t, period)
    sweep = period - flyback
    frac = np.where(u < sweep, u / sweep, 1.0 - (u - sweep) / flyback if flyback else 0.0)
    f = f_hi - (f_hi - f_lo) * frac if down else f_lo + (f_hi - f_lo) * frac
    x = np.zeros(n)
    x[start:stop] = amp * np.sin(2.0 * np.pi * np.cumsum(f) / RATE)
    if sigma:
        x += np.random.default_rng(seed).normal(0.0, sigma, n)
    return x


def tone(n, hz, amp=0.3, start=0, stop=None):
    stop = n if stop is None else stop
    x = np.zeros(n)
    x[start:stop] = amp * np.sin(2.0 * np.pi * hz * np.arange(stop - start) / RATE)
    return x


def voice_like(n, seed):
    """harmonics of a gliding pitch under a formant-like tilt, keyed in syllables at about 4 Hz (as the SELCAL stage's)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    x = sum(np.sin(k * ph + rng.uniform(0, 6.28)) / (1.0 + abs(k * 140.0 - 700.0) / 300.0) for k in range(1, 20))
    syll = np.clip(np.sin(2 * np.pi * 4.1 * t + rng.uniform(0, 6.28)) + 0.3, 0.0, 1.0)
    return 0.1 * x * syll


def punched(x, per_sweep, rate=3.0):
    """zeros punched into the middle of every sweep, 80 * per_sweep + 160 samples long: measured on the model, exactly per_sweep frames
    of every sweep then have no bin (the frames that the hole only reaches into keep theirs)"""
    x = x.copy()
    period = int(RATE / rate)
    for s0 in range(0, x.size, period):
        a = s0 + period // 2
        x[a:a + HOP * per_sweep + 160] = 0.0
    return x


def lone(n, at, value=0.5):
    x = np.zeros(n)
    x[at] = value
    return x


def builders():
    """[(name, row float64 [NB * 2000], expected kinds of the row's events)]"""
    n = NB * WAVE_BATCH
    out = []

    def add(name, x, kinds=()):
        out.append((name, x, list(kinds)))

    for rate in (2.0, 3.0, 4.0):
        add(f"a beacon at {rate:g} Hz", beacon(n, rate), [ONSET])
    add("an upward beacon", beacon(n, down=False), [ONSET])
    add("the widest beacon", beacon(n, f_hi=1600.0, f_lo=300.0), [ONSET])
    add("a 700 Hz sweep", beacon(n, f_hi=1400.0, f_lo=700.0), [ONSET])
    add("a 500 Hz sweep", beacon(n, f_hi=1300.0, f_lo=800.0))
    add("a sweep rate of 1 Hz", beacon(n, 1.0))
    add("a sweep rate of 6 Hz", beacon(n, 6.0))
    per = RATE // 3 + 1  # samples of one sweep at 3 Hz (16000 / 3, rounded up)
    add("five sweeps then silence", beacon(n, start=4000, stop=4000 + 5 * per))
    add("six sweeps then silence", beacon(n, start=4000, stop=4000 + 6 * per + 200), [ONSET, END])
    x = beacon(n, stop=40000) + beacon(n, start=40000 + 20 * HOP + FRAME, seed=2)
    add("a beacon that stops and restarts after 20 frames", x, [ONSET, END, ONSET])
    x = beacon(n, stop=48000) + beacon(n, down=False, start=48000)
    add("a beacon whose direction flips", x, [ONSET, END, ONSET])
    add("two frames punched into every sweep", punched(beacon(n), 2), [ONSET])
    add("three frames punched into every sweep", punched(beacon(n), 3))
    add("a beacon at the noise's power", beacon(n, amp=0.3, sigma=0.3 / np.sqrt(2.0), seed=21), [ONSET])
    add("a steady 1 kHz tone", tone(n, 1000.0))
    add("a tone at 2 kHz", tone(n, 2000.0))
    x = np.zeros(n)
    for k, (fa, fb) in enumerate(((312.6, 716.1), (524.8, 1083.9), (881.0, 1479.1))):
        x += tone(n, fa, 0.2, 8000 + 20000 * k, 24000 + 20000 * k) + tone(n, fb, 0.2, 8000 + 20000 * k, 24000 + 20000 * k)
    add("SELCAL-like tone pairs", x)
    add("voice-like", voice_like(n, 67))
    add("white noise", np.random.default_rng(66).normal(0.0, 0.2, n))
    add("silence", np.zeros(n))
    add("-0.0 throughout", np.full(n, -0.0))
    add("subnormal values", np.random.default_rng(65).choice([1e-40, -3e-41, 1e-45, 0.0, 2e-39], n))
    for at in (0, 79, 80, 1999):
        add(f"a lone sample at block index {at}", lone(n, 2 * WAVE_BATCH + at))
    return out


_stacked = None


def stacked():
    """(names, plane float32 [rows][NB * 2000], expected kinds per row) of the builders, built once"""
    global _stacked
    if _stacked is None:
        b = builders()
        _stacked = [x[0] for x in b], np.stack([x[1] for x in b]).astype(F32), [x[2] for x in b]
    return _stacked


def carried_edge_state():
    """a fresh state of two rows but for one carried sample each: the newest (x[177]) and the oldest that weighs (x[3]: x[2] is the
    first sample of a batch's first frame, where the window is 0)"""
    st = fresh_state(2)
    st["x"][0, HISTORY - 1] = 0.5
    st["x"][1, 3] = 0.5
    return st


OFFSET_NB = 20  # batches of the start-offset rows: 2.5 s, seven sweeps and a half


def start_offsets():
    """80 rows, a beacon beginning at every sample offset modulo 80 inside the second batch: float32 [80][OFFSET_NB * 2000]"""
    n = OFFSET_NB * WAVE_BATCH
    return np.stack([beacon(n, start=WAVE_BATCH + k) for k in range(HOP)]).astype(F32)


# ---------------- seeded decision sequences for the walker ----------------
def sweep_bins(first, last, length):
    """`length` decisions that go from bin `first` to bin `last` in even steps"""
    return [int(v) for v in np.rint(np.linspace(first, last, length))]


def chain(nsweeps, first=24, last=8, length=50, gap=2):
    out = []
    for _ in range(nsweeps):
        out += sweep_bins(first, last, length) + [NONE8] * gap
    return out


def walker_sequences():
    """[(name, decisions, settings overrides, expected kinds)]: every transition, and both sides of every settings bound"""
    seqs = []

    def add(name, d, kinds, **kw):
        seqs.append((name, list(d) + [NONE8] * 30, kw, list(kinds)))

    add("six sweeps", chain(6), [ONSET, END])
    add("five sweeps", chain(5), [])
    add("seven sweeps, min_sweeps 7", chain(7), [ONSET, END], min_sweeps=7)
    add("six sweeps, min_sweeps 7", chain(6), [], min_sweeps=7)
    add("span exactly min_span", chain(6, 20, 10), [ONSET, END])
    add("span one under min_span", chain(6, 20, 11), [])
    add("length exactly min_len", chain(6, length=40), [ONSET, END])
    add("length one under min_len", chain(6, length=39), [])
    add("length exactly max_len", chain(7, 26, 4, 120, gap=0), [ONSET, END])  # (followed at once by the retrace: a frame later the chain would expire)
    add("length one over max_len", chain(7, 26, 4, 121, gap=0), [])
    add("length max_len and then a frame without a bin", chain(7, 26, 4, 120, gap=1), [])
    add("steps of exactly max_step", chain(6, 26, 5, 8, gap=1), [ONSET, END], min_len=8)
    add("a step over max_step", chain(6, 26, 4, 8, gap=1)[:-1] + [4], [], min_len=8)  # 26 -> 4 in 7 steps: one of 4
    d = chain(6)
    for k in range(6):
        d[52 * k + 20:52 * k + 22] = [NONE8, NONE8]
    add("max_drop frames dropped inside every sweep", d, [ONSET, END])
    d = chain(6)
    for k in range(6):
        d[52 * k + 20:52 * k + 23] = [NONE8] * 3
    add("one more than max_drop dropped", d, [])
    add("a gap of exactly max_gap", chain(6, gap=9), [ONSET, END])  # start - last_end = gap + 1
    add("a gap one over max_gap", chain(6, gap=10), [])
    add("retraces with no gap at all", chain(8, gap=0), [ONSET, END])
    add("upward sweeps", chain(6, 8, 24), [ONSET, END])
    add("a flip of direction in an alarmed chain", chain(7) + chain(6, 8, 24), [ONSET, END, ONSET, END])
    add("a flip of direction before the alarm", chain(4) + chain(6, 8, 24), [ONSET, END])
    add("a steady bin", [12] * 400, [])
    add("a sweep that turns back", sweep_bins(24, 12, 30) + sweep_bins(13, 24, 30), [])
    add("a long alarm", chain(20), [ONSET, END])
    add("an invalid sweep inside a chain", chain(3) + sweep_bins(24, 22, 4) + [NONE8] * 2 + chain(3), [ONSET, END])
    add("a chain, a pause over max_gap, a chain", chain(6) + [NONE8] * 20 + chain(6), [ONSET, END, ONSET, END])
    rng = np.random.default_rng(77)
    add("seeded random bins", list(rng.choice([NONE8] + list(range(4, 27)), 3000)), [], )
    return seqs


# ---------------- audio that decides each settings bound in the walker ----------------
BOUND_NB = 32  # batches of the bound rows: 4 s


def bound_signals():
    """{name: row float64 [BOUND_NB * 2000]}: beacons whose sweeps the model measures as the comments say (test_elt_model.py asserts it)"""
    n, per3, per4 = BOUND_NB * WAVE_BATCH, RATE // 3 + 1, RATE // 4
    fast = beacon(n, 10.0, f_hi=1600.0, f_lo=300.0)  # sweeps of 20 frames (the first 21) over 19 bins: steps of 0, 1 and 2
    holed = fast.copy()
    for s0 in range(0, n, RATE // 10):  # one frame without a bin in every sweep, the step over it 4 bins
        holed[s0 + 700:s0 + 700 + HOP + 160] = 0.0
    return {
        "4 Hz": beacon(n, 4.0),  # sweeps of 50 frames, the first 51, 16 bins, a retrace at once (start - last_end = 1)
        "700 Hz wide": beacon(n, f_hi=1400.0, f_lo=700.0),  # spans of 11 bins
        "10 Hz": fast,
        "10 Hz, a frame punched": holed,
        "a pause": beacon(n, stop=16040) + beacon(n, start=16040 + 20 * HOP + FRAME, seed=2),  # start - last_end = 24 over the pause, after 3 sweeps
        "three frames punched": punched(beacon(n), 3),
        "two frames punched": punched(beacon(n), 2),
        "five sweeps": beacon(n, start=4000, stop=4000 + 5 * per3),
        "six sweeps": beacon(n, start=4000, stop=4000 + 6 * per3 + 200),
        "six sweeps at 4 Hz, then silence": beacon(n, 4.0, start=4000, stop=4000 + 6 * per4),  # the sixth, 51 frames, is closed by the silence
        "a flip before the alarm": beacon(n, stop=4 * per3) + beacon(n, down=False, start=4 * per3),
        "a narrow sweep inside": beacon(n, stop=3 * per3) + beacon(n, f_hi=1300.0, f_lo=800.0, start=3 * per3, stop=4 * per3) + beacon(n, start=4 * per3),
        # (8 bins, not valid; the next valid sweep starts 68 frames after the last one ended)
    }


def bound_cases():
    """[(name, signal name, settings overrides, expected kinds, expected first_frame of the first event or None)]: each setting exactly
    on what the model measures for the signal, and one beyond"""
    return [
        ("min_len on", "4 Hz", dict(min_len=50), [ONSET], 0),
        ("min_len beyond", "4 Hz", dict(min_len=51), [], None),
        ("max_len on", "4 Hz", dict(max_len=51), [ONSET], 0),
        ("max_len between", "4 Hz", dict(max_len=50), [ONSET], 51),  # (the first sweep, 51 frames, does not count)
        ("max_len beyond", "4 Hz", dict(max_len=49), [], None),
        ("min_span on", "700 Hz wide", dict(min_span=11), [ONSET], 0),
        ("min_span beyond", "700 Hz wide", dict(min_span=12), [], None),
        ("max_step on", "10 Hz", dict(max_step=2, min_len=20, min_sweeps=12), [ONSET], 0),
        ("max_step beyond", "10 Hz", dict(max_step=1, min_len=20, min_sweeps=12), [], None),
        ("max_step * (1 + drops) on", "10 Hz, a frame punched", dict(max_step=2, max_drop=1, min_len=20, min_sweeps=12), [ONSET], 0),
        ("max_step * (1 + drops) beyond", "10 Hz, a frame punched", dict(max_step=1, max_drop=1, min_len=20, min_sweeps=12), [], None),
        ("max_gap on", "a pause", dict(max_gap=24), [ONSET], 0),
        ("max_gap beyond", "a pause", dict(max_gap=23), [ONSET], 224),  # (the chain begins again behind the pause)
        ("max_gap on, over a sweep that is not valid", "a narrow sweep inside", dict(max_gap=68), [ONSET], 0),
        ("max_gap beyond, over a sweep that is not valid", "a narrow sweep inside", dict(max_gap=67), [ONSET], 268),
        ("max_drop on", "three frames punched", dict(max_drop=3), [ONSET], 0),
        ("max_drop beyond", "two frames punched", dict(max_drop=1), [], None),
        ("min_sweeps on", "five sweeps", dict(min_sweeps=5), [ONSET, END], 50),
        ("min_sweeps beyond", "six sweeps", dict(min_sweeps=7), [], None),
        ("max_len and then frames without a bin, on", "six sweeps at 4 Hz, then silence", dict(max_len=53), [ONSET, END], 50),
        ("max_len and then frames without a bin, beyond", "six sweeps at 4 Hz, then silence", dict(max_len=52), [], None),
        ("a flip before the alarm", "a flip before the alarm", {}, [ONSET], 268),
    ]


def refused_states(s=DEFAULTS):
    """[(name, a STATE record's fields that set_state and the twin must refuse)]: seeded from states the walker can be in"""
    seg = dict(frame=100, open=1, start=90, first_bin=20, last_bin=17, last_frame=99, dir=DOWN, drops=0)
    ch = dict(frame=100, count=2, chain_dir=DOWN, chain_first=10, last_end=95, alarmed=0, bin_from=24, bin_to=8)
    al = dict(ch, count=6, alarmed=1)
    good = [("a fresh state", {}), ("an open segment", seg), ("a chain", ch), ("an alarmed chain", al), ("both", dict(seg, **dict(al, last_end=89)))]
    bad = [("open beyond 1", dict(seg, open=2)), ("alarmed beyond 1", dict(al, alarmed=2)), ("a closed segment with a bin", dict(first_bin=5)),
           ("a closed segment with drops", dict(drops=1)), ("first_bin under 2", dict(seg, first_bin=1)), ("last_bin over 33", dict(seg, last_bin=34)),
           ("dir beyond DOWN", dict(seg, dir=3)), ("dir against the bins", dict(seg, dir=UP)), ("dir 0 with a step", dict(seg, dir=0)),
           ("drops over max_drop", dict(seg, drops=3, last_frame=96)), ("drops that are not the frames since last_frame", dict(seg, drops=1)),
           ("a segment of 2^31 frames", dict(seg, start=(90 - 0x80000000) & M32)), ("a cleared chain with a field", dict(last_end=5)),
           ("alarmed without a chain", dict(alarmed=1)), ("chain_dir 0", dict(ch, chain_dir=0)), ("chain_dir against the bins", dict(ch, chain_dir=UP)),
           ("bin_from under 2", dict(ch, bin_from=0)), ("a span under min_span", dict(ch, bin_to=15)), ("alarmed under min_sweeps", dict(ch, alarmed=1)),
           ("not alarmed at min_sweeps", dict(al, alarmed=0)), ("a chain that would have expired", dict(ch, last_end=88)),
           ("a chain that ends before it began", dict(ch, chain_first=96)), ("a segment that began before the chain ended", dict(seg, **dict(ch, last_end=95)))]
    return good, bad


def state_of(rows, row, fields):
    st = fresh_state(rows)
    for k, v in fields.items():
        st[k][row] = v
    return st


# ---------------- end to end: a beacon on an AM carrier, as u8 I/Q ----------------
E2E_BATCHES = 32


def e2e_setup(pkg):
    """One stream, one AM channel five bins above the centre at fft 512, 2.56 Msps, a carrier modulated 80 % by the 3 Hz beacon from the
    start: (dev, chans, iq uint8, batches)."""
    from common import AGC_EXTRA
    rate, centre = 2560000, 120000000
    dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9)
    chans = [pkg.channel_cfg(centre + 25000, modulation=pkg.MOD_AM)]
    hop = rate // RATE
    n_audio = E2E_BATCHES * WAVE_BATCH + AGC_EXTRA + 8
    audio = beacon(n_audio, amp=0.8)
    n = n_audio * hop
    rng = np.random.default_rng(71)
    env = np.repeat(1.0 + audio, hop).astype(np.float32)
    ph = (2.0 * np.pi * 25000.0 / rate) * (np.arange(n) % (rate // 5000))  # (the offset's period is 512 samples: no phase grows large)
    z = 30.0 * env * np.exp(1j * ph).astype(np.complex64)
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    iq += rng.normal(0.0, 1.5, 2 * n).astype(np.float32)
    return dev, chans, np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8), E2E_BATCHES
