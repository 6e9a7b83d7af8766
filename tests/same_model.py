"""The SAME decoder stage (include/mi_airband.h "SAME decoder stage") restated in numpy and plain Python, operation for operation: the
bit bank in float32 with every product and sum rounded on its own, the walker and the assembler in Python integers.  Beside it a
continuous-phase AFSK modulator in float64 and the rows the tests run: builders(), start_unit_rows(), tie_cases(), timing_cases()."""
import functools

import numpy as np

WAVE_BATCH, NTAU, UNITS, BATCH_UNITS, NWORDS, HIST, RAW, MAX_BYTES, DEAF = 2000, 16, 768, 50000, 4, 30, 272, 268, 64
IDLE, BURST, HEADER, EOM = 0, 1, 0, 1
NB = 64  # batches of a builder's row: 8 s
WALKER = ("phase", "u", "kind", "nbits", "cur", "nbytes", "nbad", "plus", "dashes", "deaf", "start_batch", "start_unit", "an", "akind", "alen0", "alen1",
          "atrunc0", "atrunc1", "aidle", "astart_batch", "astart_unit")
MSG_REC = np.dtype([("row", "<u4"), ("kind", "<u4"), ("batch", "<u4"), ("unit", "<u4"), ("end_batch", "<u4"), ("nbursts", "u1"), ("voted", "u1"),
                    ("truncated", "u1"), ("fields_ok", "u1"), ("nbytes", "<u2"), ("agree", "<u2"), ("zero", "<u4"), ("bytes", "u1", (RAW,))])
STATE = np.dtype([("x", "<f4", (HIST,)), ("batch", "<u4"), ("grid", "<u4"), ("hist", "<u8", (NTAU,))] + [(n, "<u4") for n in WALKER + ("zero",)] +
                 [("bytes", "u1", (3, RAW))])
assert MSG_REC.itemsize == 304 and STATE.itemsize == 1160
DEFAULTS = dict(sync_errors=4, max_bad=4, gap_batches=20, min_quality=0.0, space_gain=1.0, hold_timing=False)
M64 = (1 << 64) - 1


def pattern(tail):
    p = 0
    for byte in b"\xab\xab\xab\xab" + tail:
        for i in range(8):
            p = p << 1 | (byte >> i & 1)
    return p


SYNC = (pattern(b"ZCZC"), pattern(b"NNNN"))


def fresh_state(rows):
    return np.zeros(rows, STATE)


@functools.lru_cache(None)
def templates():
    rho = np.arange(UNITS, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * 4 * rho / UNITS), np.sin(2 * np.pi * 4 * rho / UNITS), np.cos(2 * np.pi * 3 * rho / UNITS),
                     np.sin(2 * np.pi * 3 * rho / UNITS)]).astype(np.float32)


def ahead(grid):
    a = grid // 48 + 1
    return 0 if a == NTAU else a


def first(grid, tau):
    c = (48 * tau - grid) % UNITS
    return c - UNITS if c else 0


def count(r0):
    return (BATCH_UNITS - UNITS - r0) // UNITS + 1


@functools.lru_cache(None)
def batch_plan(grid):
    """(r0 [16], cnt [16], and for all bits of the batch in (tau, j) order: index of the first sample in the staged block, rho of it)"""
    r0 = [first(grid, t) for t in range(NTAU)]
    cnt = [count(r) for r in r0]
    r = np.concatenate([r0[t] + UNITS * np.arange(cnt[t]) for t in range(NTAU)])
    n0 = -((-r) // 25)
    return r0, cnt, HIST + 2 + n0, 25 * n0 - r


def bit_bank(staged, grid, space_gain):
    """bits [16] lists, Q [16] float32, words [16][4] of one batch; staged: the 32 floats of the lead and the 2000 of the block"""
    T = templates()
    r0, cnt, idx, rho = batch_plan(grid)
    x = staged[idx]
    S = [x * T[k][rho] for k in range(4)]
    for i in range(1, 30):
        x = staged[idx + i]
        for k in range(4):
            S[k] = S[k] + x * T[k][rho + 25 * i]
    more = rho <= 17
    x = staged[np.minimum(idx + 30, staged.size - 1)]
    for k in range(4):
        S[k] = np.where(more, S[k] + x * T[k][np.minimum(rho + 750, UNITS - 1)], S[k])
    pm, ps = S[0] * S[0] + S[1] * S[1], S[2] * S[2] + S[3] * S[3]
    bit = pm >= np.float32(space_gain) * ps
    q = np.where(pm > ps, pm, ps)
    words, Q, bits, at = np.zeros((NTAU, NWORDS), np.uint32), np.zeros(NTAU, np.float32), [], 0
    for t in range(NTAU):
        b, qt = bit[at:at + cnt[t]], q[at:at + cnt[t]]
        at += cnt[t]
        bits.append([int(v) for v in b])
        for j, v in enumerate(bits[t]):
            words[t, j // 32] |= np.uint32(v << (j % 32))
        words[t, 3] = cnt[t]
        lane = qt[:64].copy()
        lane[:cnt[t] - 64] = lane[:cnt[t] - 64] + qt[64:]
        h = 32
        while h:
            lane[:h] = lane[:h] + lane[h:2 * h]
            h //= 2
        Q[t] = lane[0]
    return bits, Q, words, r0, cnt


def mismatch(h):
    mh, me = bin(h ^ SYNC[0]).count("1"), bin(h ^ SYNC[1]).count("1")
    return (me, EOM) if me < mh else (mh, HEADER)


def pick(mk, Q, sync_errors, min_quality):
    best = -1
    for t in range(NTAU):
        if mk[t][0] > sync_errors or not Q[t] >= np.float32(min_quality):
            continue
        if best < 0 or mk[t][0] < mk[best][0] or (mk[t][0] == mk[best][0] and Q[t] > Q[best]):
            best = t
    return best


def fields_ok(b, kind=HEADER):
    b = bytes(b)
    if kind == EOM:
        return b == b"NNNN"
    n = len(b)
    if n < 42 or (n - 35) % 7 or (n - 35) // 7 > 31:
        return False
    cap, dig = (lambda s: all(65 <= c <= 90 for c in s)), (lambda s: all(48 <= c <= 57 for c in s))
    if b[:5] != b"ZCZC-" or b[8:9] != b"-" or not cap(b[5:8]) or not cap(b[9:12]):
        return False
    i = 12
    while i < n - 23:
        if b[i:i + 1] != b"-" or not dig(b[i + 1:i + 7]):
            return False
        i += 7
    if b[i:i + 1] != b"+" or b[i + 5:i + 6] != b"-" or b[i + 13:i + 14] != b"-" or b[i + 22:i + 23] != b"-":
        return False
    return dig(b[i + 1:i + 5]) and dig(b[i + 6:i + 13]) and all(0x20 <= c <= 0x7E and c != 45 for c in b[i + 14:i + 22])


def message_fields(b):
    """a header's text split as mi_same_message_text does"""
    b = bytes(b).decode("ascii")
    head, tail = b.split("+")
    parts, t = head.split("-"), tail.split("-")
    return dict(originator=parts[1], event=parts[2], locations=parts[3:], purge=t[0], issue=t[1], station=t[2])


class Row:
    """one row's walker and assembler over the state fields"""

    def __init__(self, st, row, cfg, out):
        self.w = {n: int(st[n]) for n in WALKER}
        self.bytes = [bytearray(st["bytes"][i].tobytes()) for i in range(3)]
        self.row, self.cfg, self.out = row, cfg, out

    def close(self, b, n, len2=0, trunc2=0):
        w, (b2, b0, b1) = self.w, self.bytes
        ln, trunc, agree = w["alen0"], w["atrunc0"], 0
        if n == 3:
            ln = sorted((w["alen0"], w["alen1"], len2))[1]
            trunc = int(w["atrunc0"] + w["atrunc1"] + trunc2 >= 2)
        m = np.zeros((), MSG_REC)
        for i in range(ln):
            a, c, d = b0[i], b1[i], b2[i]
            m["bytes"][i] = (a & c) | (a & d) | (c & d) if n == 3 else a
            agree += n == 1 or (a == c and (n == 2 or c == d))
        m["row"], m["kind"], m["batch"], m["unit"], m["end_batch"] = self.row, w["akind"], w["astart_batch"], w["astart_unit"], b
        m["nbursts"], m["voted"], m["truncated"], m["nbytes"], m["agree"] = n, n == 3, trunc, ln, agree
        m["fields_ok"] = fields_ok(m["bytes"][:ln].tobytes(), w["akind"])
        self.out.append(m)
        self.bytes[1], self.bytes[2] = bytearray(RAW), bytearray(RAW)
        for k in ("an", "akind", "alen0", "alen1", "atrunc0", "atrunc1", "aidle", "astart_batch", "astart_unit"):
            w[k] = 0

    def burst_end(self, trunc, b):
        w = self.w
        if w["an"] == 0:
            w["akind"], w["astart_batch"], w["astart_unit"] = w["kind"], w["start_batch"], w["start_unit"]
        if w["an"] == 2:
            self.close(b, 3, w["nbytes"], trunc)
        else:
            self.bytes[1 + w["an"]] = bytearray(self.bytes[0])
            w["alen1" if w["an"] else "alen0"], w["atrunc1" if w["an"] else "atrunc0"] = w["nbytes"], trunc
            w["an"] += 1
            w["aidle"] = 0
        self.bytes[0] = bytearray(RAW)
        for k in ("phase", "u", "kind", "nbits", "cur", "nbytes", "nbad", "plus", "dashes", "start_batch", "start_unit"):
            w[k] = 0
        w["deaf"] = DEAF

    def open(self, u, kind, batch, r, b):
        w = self.w
        if w["an"] and w["akind"] != kind:
            self.close(b, w["an"])
        w.update(phase=BURST, u=u, kind=kind, nbits=0, cur=0, nbad=0, plus=0, dashes=0, deaf=0, nbytes=4)
        self.bytes[0][:4] = b"NNNN" if kind == EOM else b"ZCZC"
        zs = r - 31 * UNITS
        w["start_batch"], w["start_unit"] = ((batch - 1) & 0xFFFFFFFF, zs + BATCH_UNITS) if zs < 0 else (batch, zs)

    def step(self, c, b):
        w, cfg = self.w, self.cfg
        w["cur"] |= c << w["nbits"]
        w["nbits"] += 1
        if w["nbits"] < 8:
            return
        byte, w["cur"], w["nbits"] = w["cur"], 0, 0
        self.bytes[0][w["nbytes"]] = byte
        w["nbytes"] += 1
        if byte & 0x80 or byte < 0x20:
            w["nbad"] += 1
            if w["nbad"] == cfg["max_bad"]:
                for _ in range(cfg["max_bad"]):
                    w["nbytes"] -= 1
                    self.bytes[0][w["nbytes"]] = 0
                return self.burst_end(1, b)
        else:
            w["nbad"] = 0
            if not w["plus"]:
                w["plus"] = int(byte == 0x2B)
            elif byte == 0x2D:
                w["dashes"] += 1
                if w["dashes"] == 3:
                    return self.burst_end(0, b)
        if w["nbytes"] == MAX_BYTES:
            self.burst_end(1, b)

    def retime(self, Q):
        w = self.w
        u = w["u"]
        um, up, v = (u + 15) % 16, (u + 1) % 16, u
        if Q[um] > Q[v]:
            v = um
        if Q[up] > Q[v]:
            v = up
        w["u"] = v
        return "skip" if (u, v) == (15, 0) else "replay" if (u, v) == (0, 15) else None


_memo = {}


def same_model(plane, state=None, enabled=None, **cfg):
    """-> (messages [k] of MSG_REC, bits [rows][nb][16][4], q [rows][nb][16], row_first [rows + 1], state after); plane: float32
    [rows][nb * 2000]; state: STATE [rows] or None; cfg: what DEFAULTS names.  A disabled row's bits and q stay zero."""
    cfg = {**DEFAULTS, **cfg}
    plane = np.ascontiguousarray(plane, np.float32)
    rows, nb = plane.shape[0], plane.shape[1] // WAVE_BATCH
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(STATE).reshape(rows)
    enabled = np.ones(rows, bool) if enabled is None else np.asarray(enabled, bool)
    bits, q = np.zeros((rows, nb, NTAU, NWORDS), np.uint32), np.zeros((rows, nb, NTAU), np.float32)
    msgs, row_first = [], np.zeros(rows + 1, np.uint32)
    for r in range(rows):
        row_first[r] = len(msgs)
        if not enabled[r]:
            continue
        key = (plane[r].tobytes(), state[r].tobytes(), tuple(sorted(cfg.items())))
        if key not in _memo:
            _memo[key] = model_row(plane[r], state[r].copy(), cfg, nb)
        out, bits[r], q[r], state[r] = _memo[key]
        for m in out:
            m = m.copy()
            m["row"] = r
            msgs.append(m)
    row_first[rows] = len(msgs)
    return (np.array(msgs, MSG_REC) if msgs else np.zeros(0, MSG_REC)), bits, q, row_first, state


def model_row(x, st, cfg, nb):
    out, bits, q = [], np.zeros((nb, NTAU, NWORDS), np.uint32), np.zeros((nb, NTAU), np.float32)
    staged = np.concatenate([np.zeros(2, np.float32), st["x"], x[:nb * WAVE_BATCH]])
    walker = Row(st, 0, cfg, out)
    w = walker.w
    hist, grid, batch0 = [int(h) for h in st["hist"]], int(st["grid"]), int(st["batch"])
    for b in range(nb):
        bit, Q, bits[b], r0, cnt = bit_bank(staged[b * WAVE_BATCH:(b + 1) * WAVE_BATCH + HIST + 2], grid, cfg["space_gain"])
        q[b] = Q
        a_in = ahead(grid)
        nxt = (grid + 80) % UNITS
        rounds = {cnt[t] + (t < a_in) - (t < ahead(nxt)) for t in range(NTAU)}
        assert rounds == {cnt[15]}, "every hypothesis decides the same number of indices"
        if w["phase"] == IDLE and w["an"]:
            w["aidle"] += 1
            if w["aidle"] >= cfg["gap_batches"]:
                walker.close(b, w["an"])
        skip = False
        if w["phase"] == BURST and not cfg["hold_timing"]:
            move = walker.retime(Q)
            skip = move == "skip"
            if move == "replay":
                walker.step(hist[15] & 1, b)
        for i in range(cnt[15]):
            c = [0] * NTAU
            for t in range(NTAU):
                j = i - (t < a_in)
                if j >= 0:
                    c[t] = bit[t][j]
                    hist[t] = (hist[t] << 1 | c[t]) & M64
                else:
                    c[t] = hist[t] & 1
            if w["phase"] == BURST:
                if skip:
                    skip = False
                else:
                    walker.step(c[w["u"]], b)
            elif w["deaf"]:
                w["deaf"] -= 1
            else:
                mk = [mismatch(h) for h in hist]
                u = pick(mk, Q, cfg["sync_errors"], cfg["min_quality"])
                if u >= 0:
                    walker.open(u, mk[u][1], (batch0 + b) & 0xFFFFFFFF, r0[u] + UNITS * (i - (u < a_in)), b)
                    if mk[u][1] == EOM:
                        walker.burst_end(0, b)
        for t in range(ahead(nxt)):
            hist[t] = (hist[t] << 1 | bit[t][cnt[t] - 1]) & M64
        grid = nxt
    st["hist"], st["grid"], st["batch"] = hist, grid, (batch0 + nb) & 0xFFFFFFFF
    for n in WALKER:
        st[n] = w[n]
    for i in range(3):
        st["bytes"][i] = np.frombuffer(bytes(walker.bytes[i]), np.uint8)
    st["x"] = x[nb * WAVE_BATCH - HIST:nb * WAVE_BATCH]
    return out, bits, q, st


# ---- the modulator and the rows

HEADER_TEXT = b"ZCZC-WXR-TOR-039173-039051+0030-1591829-KCLE/NWS-"
LONGEST = b"ZCZC-CIV-EVI" + b"".join(b"-%06d" % (1000 * i + 7) for i in range(1, 32)) + b"+0100-3652359-WXYZ/FM -"
PREAMBLE = b"\xab" * 16


def to_bits(data):
    return [byte >> i & 1 for byte in data for i in range(8)]


def modulate(n, bursts, noise=0.0, seed=0, voice=None):
    """float32 [n]: bursts = [(bits, start unit, ppm, amplitude)], continuous-phase AFSK computed in float64: a bit lasts
    768 / (1 + ppm 1e-6) units and turns the phase by 4 (mark) or 3 (space) cycles; seeded Gaussian noise and `voice` added."""
    t = 25.0 * np.arange(n)
    x = np.zeros(n)
    for bits, start, ppm, amp in bursts:
        tb = UNITS / (1 + ppm * 1e-6)
        cyc = np.where(np.array(bits) == 1, 4.0, 3.0)
        cum = np.concatenate([[0.0], np.cumsum(cyc)])
        pos = (t - start) / tb
        k = np.floor(pos).astype(np.int64)
        on = (k >= 0) & (k < len(bits))
        kk = np.clip(k, 0, len(bits) - 1)
        x += np.where(on, amp * np.sin(2 * np.pi * (cum[kk] + cyc[kk] * (pos - kk))), 0.0)
    if noise:
        x += np.random.default_rng(seed).normal(0, noise, n)
    if voice is not None:
        x += voice
    return x.astype(np.float32)


def voice_like(n, seed, start=0, stop=None, level=0.2):
    """voice-like audio: harmonics of a wandering pitch under a syllable envelope, float64 [n], zero outside start .. stop"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6)) + 10 * np.sin(2 * np.pi * 3.1 * t)
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    v = sum(rng.uniform(0.2, 1.0) / h * np.sin(h * ph + rng.uniform(0, 6)) for h in range(1, 24))
    v *= level * (0.5 + 0.5 * np.sin(2 * np.pi * 4.0 * t + 1.0)) ** 2 / 2.0
    stop = n if stop is None else stop
    v[:start] = 0
    v[stop:] = 0
    return v


def burst_bits(text, flips=()):
    bits = to_bits(PREAMBLE + text)
    for f in flips:
        bits[128 + f] ^= 1
    return bits


GAP = int(0.4 * 16000 * 25)  # units between a burst's end and the next one's start in these rows


def train(texts, start=30011, ppm=0.0, amp=0.5, flips=None):
    """bursts one after the other, GAP apart -> [(bits, start, ppm, amp)], and the unit behind the last"""
    out = []
    for i, text in enumerate(texts):
        bits = burst_bits(text, (flips or {}).get(i, ()))
        out.append((bits, start, ppm, amp))
        start += int(len(bits) * UNITS / (1 + ppm * 1e-6)) + GAP
    return out, start


@functools.lru_cache(None)
def builders():
    """-> (names, plane [rows][NB * 2000], expect {name: [(kind, nbursts, voted, truncated, text)]}): the rows the tests run"""
    n = NB * WAVE_BATCH
    rows, expect = [], {}

    def add(name, x, want):
        rows.append((name, np.asarray(x, np.float32)))
        expect[name] = want

    three, end = train([HEADER_TEXT] * 3)
    voice_start = end // 25
    eom, _ = train([b"NNNN"] * 3, start=end + 2 * 16000 * 25 - GAP)
    add("a full alert", modulate(n, three + eom, voice=voice_like(n, 1, voice_start, voice_start + 32000 - GAP // 25)),
        [(HEADER, 3, 1, 0, HEADER_TEXT), (EOM, 3, 1, 0, b"NNNN")])
    add("the longest header", modulate(n, train([LONGEST])[0]), [(HEADER, 1, 0, 0, LONGEST)])
    flips = {1: tuple(range(40, 40 + 12 * 23, 23))}
    add("12 bit errors in one burst of three", modulate(n, train([HEADER_TEXT] * 3, flips=flips)[0]), [(HEADER, 3, 1, 0, HEADER_TEXT)])
    add("two bursts only", modulate(n, train([HEADER_TEXT] * 2)[0]), [(HEADER, 2, 0, 0, HEADER_TEXT)])
    add("one burst only", modulate(n, train([HEADER_TEXT])[0]), [(HEADER, 1, 0, 0, HEADER_TEXT)])
    cut = burst_bits(HEADER_TEXT)[:128 + 8 * 30]
    add("a burst cut off by silence", modulate(n, [(cut, 30011, 0.0, 0.5)]), [(HEADER, 1, 0, 1, HEADER_TEXT[:30])])
    for start in (0, 7, 16, 24, 47):
        add(f"start unit {start} modulo 48", modulate(n, train([HEADER_TEXT] * 3, start=48 * 700 + start)[0]), [(HEADER, 3, 1, 0, HEADER_TEXT)])
    for ppm in (200.0, -200.0):
        add(f"{ppm:+.0f} ppm", modulate(n, train([LONGEST], ppm=ppm)[0]), [(HEADER, 1, 0, 0, LONGEST)])
    add("a full alert in noise", modulate(n, three, noise=0.05, seed=3), [(HEADER, 3, 1, 0, HEADER_TEXT)])
    add("amplitude 1e-3", modulate(n, train([HEADER_TEXT] * 3, amp=1e-3)[0]), [(HEADER, 3, 1, 0, HEADER_TEXT)])
    add("silence", np.zeros(n), [])
    add("-0.0 throughout", np.full(n, -0.0), [])
    add("subnormals", np.random.default_rng(5).choice(np.array([1e-42, -3e-43, 0.0, 7e-45]), n), [])
    add("noise only", np.random.default_rng(6).normal(0, 0.1, n), [])
    add("voice-like only", voice_like(n, 7), [])
    names = [r[0] for r in rows]
    return names, np.stack([r[1] for r in rows]), expect


START_NB, START_CFG = 10, dict(gap_batches=1)  # a burst of 8 batches; the batch behind its end closes the message


@functools.lru_cache(None)
def start_unit_rows():
    """One header burst per row, row s beginning at unit 48 * 41 + s, s = 0 .. 47: every start unit modulo 48 (and so every offset
    to the nearest hypothesis; modulo 25 they give rho of a bit's first sample 0 .. 24 many times over) -> plane [48][10 * 2000]"""
    return np.stack([modulate(START_NB * WAVE_BATCH, train([HEADER_TEXT], start=48 * 41 + s)[0]) for s in range(48)])


def tie_cases():
    """Seeded histories that hold the EOM pattern less its newest bit (a 0) on hypotheses 4 and 11, over a batch of space tone (every
    bit 0) whose level rises or falls along the batch: both hit exactly at the batch's first index, and Q of the later hypothesis, 11,
    is the larger under the rising level, the smaller under the falling one.  -> [(name, state [1], plane [1][2000], settings as a
    function of the batch's Q, the hypothesis that must open the burst)]"""
    st = fresh_state(1)
    st["hist"][0][[4, 11]] = SYNC[1] >> 1
    n = WAVE_BATCH
    tone = modulate(n, [([0] * 70, -2 * UNITS, 0.0, 1.0)]).astype(np.float64)
    rise = (tone * np.linspace(0.1, 0.5, n)).astype(np.float32)[None, :]
    fall = (tone * np.linspace(0.5, 0.1, n)).astype(np.float32)[None, :]
    one = st.copy()
    one["hist"][0][11] ^= np.uint64(1 << 20)  # hypothesis 11 with one mismatch
    mid = lambda Q: dict(min_quality=float((np.float64(Q[4]) + np.float64(Q[11])) / 2))  # noqa: E731
    return [("a larger Q beats a lower tau", st, rise, lambda Q: {}, 11), ("the lower tau has the larger Q", st, fall, lambda Q: {}, 4),
            ("fewer mismatches beat a larger Q", one, rise, lambda Q: {}, 4),
            ("the hypothesis with fewer mismatches lies under min_quality and is no hit", one, rise, mid, 11)]


def tie_start_unit(u):
    """astart_unit of a burst opened on hypothesis u at the first index of a batch whose grid is 0"""
    return 48 * u - UNITS - 31 * UNITS + BATCH_UNITS


def timing_cases():
    """Seeded states that take every timing move in one batch: -> (names, state [rows], plane [rows][2000], moves [(u before, u
    after)]).  Each row is inside a burst on hypothesis u; the batch holds a tone burst placed so that Q peaks on the wanted
    neighbour, or a level that ties."""
    cases = [("u - 1", 5, 4), ("u + 1", 5, 6), ("stay", 5, 5), ("0 -> 15, the carried bit taken again", 0, 15), ("15 -> 0, an index passed over", 15, 0),
             ("1 -> 0", 1, 0), ("14 -> 15", 14, 15), ("the tie of all (silence) stays", 9, 9)]
    st = fresh_state(len(cases))
    plane = np.zeros((len(cases), WAVE_BATCH), np.float32)
    for i, (name, u, v) in enumerate(cases):
        s = st[i]
        s["batch"], s["grid"] = 48 * 5, 0  # (grid 0 goes with a batch count that is a multiple of 48)
        s["phase"], s["u"], s["kind"], s["nbytes"], s["nbits"], s["cur"] = BURST, u, HEADER, 6, 3, 0b101
        s["bytes"][0][:6] = np.frombuffer(b"ZCZC-W", np.uint8)
        s["start_batch"], s["start_unit"] = 48 * 5 - 1, 1234
        s["hist"] = np.arange(1, NTAU + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        if "silence" not in name:
            # alternating bits all through the batch, in step with the hypothesis three beyond u on v's side (with u - 24 units where
            # the row stays: Q's top is broad and lies half a step late): Q falls from there through v to u
            d = 0 if u == v else 1 if (v - u) % NTAU == 1 else -1
            plane[i] = modulate(WAVE_BATCH, [([1, 0] * 36, 48 * (u + 3 * d) - 24 * (d == 0) - 2 * UNITS, 0.0, 0.5)])
    return [c[0] for c in cases], st, plane, [(c[1], c[2]) for c in cases]
