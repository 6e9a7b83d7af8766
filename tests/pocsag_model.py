"""The pager decoder stage's definition (include/mi_airband.h "pager decoder stage") restated in numpy, and the signals its tests use.

The bit bank is array operations in the header's order (float32, one rounding per operation); the sync compare runs over each lane's
whole bit stream at once; the walker is plain Python; the BCH division goes bit by bit and the repair looks the syndrome up in a
dictionary made from all 497 patterns.  The modulator is written independently of the demodulator: codewords from the generator, a
bit sequence, and NRZ levels at every sample time, for any start time and clock offset."""
import numpy as np

F32 = np.float32
RATE, WAVE_BATCH = 16000, 2000
HISTORY, LEAD, MAX_LANES, MAX_WORDS = 34, 36, 30, 80
TWELFTHS = 12 * WAVE_BATCH
IDLE, TRANSMISSION = 0, 1
SYNC, IDLE_WORD, GEN = 0x7CD215D8, 0x7A89C197, 0x769
GEOM = {512: (375, 25, 15, 64, 2), 1200: (160, 16, 10, 150, 5), 2400: (80, 8, 10, 300, 10)}  # L, step, H, B, W
NBATCHES = {512: 30, 1200: 12, 2400: 8}  # what a builder's row lasts
MESSAGE = np.dtype([("row", "<u4"), ("batch", "<u4"), ("twelfth", "<u4"), ("end_batch", "<u4"), ("address", "<u4"), ("function", "u1"), ("nwords", "u1"),
                    ("nbad", "u1"), ("truncated", "u1"), ("corrected", "<u2"), ("inverted", "u1"), ("sync_errors", "u1"), ("lane_sync", "u1"),
                    ("lane_end", "u1"), ("zero", "<u2"), ("bad", "<u4", (3,)), ("zero2", "<u4"), ("words", "<u4", (MAX_WORDS,))])
WALKER = ("lane", "inverted", "pos", "cur", "nbits", "gbad", "lane_sync", "mismatches", "wbatch", "wtwelfth", "open")
STATE = np.dtype([("x", "<f4", (HISTORY,)), ("batch", "<u4"), ("phase", "<u4"), ("hist", "<u8", (MAX_LANES,))] + [(n, "<u4") for n in WALKER + ("zero",)] +
                 [("msg", MESSAGE)])
NUMERIC = "0123456789*U -)("
assert MESSAGE.itemsize == 368 and STATE.itemsize == 800


def fresh_state(rows):
    return np.zeros(rows, STATE)


def max_messages(nbatches, baud=1200):
    return 1 + (nbatches * (GEOM[baud][3] + 1) - 1) // 32


# ---------------- codewords ----------------

def remainder(word):
    """bits 31 .. 1 of a word, as a polynomial, modulo the generator"""
    r = word >> 1
    for i in range(30, 9, -1):
        if r >> i & 1:
            r ^= GEN << (i - 10)
    return r


def codeword(data21):
    w = (data21 & 0x1FFFFF) << 11
    w |= remainder(w) << 1
    return w | bin(w).count("1") & 1


def _patterns():
    t = {0: 0}
    for a in range(1, 32):
        t[remainder(1 << a)] = 1 << a
        for b in range(a + 1, 32):
            t[remainder(1 << a | 1 << b)] = 1 << a | 1 << b
    return t


PATTERNS = _patterns()
assert len(PATTERNS) == 497 and remainder(SYNC) == 0 and remainder(IDLE_WORD) == 0 and bin(SYNC).count("1") % 2 == 0 and bin(IDLE_WORD).count("1") % 2 == 0


def decode(word, correct=1):
    """(good, the word as stored, e)"""
    pat = PATTERNS.get(remainder(word))
    if pat is None:
        return False, word, 3
    f, e = word ^ pat, bin(pat).count("1")
    if bin(f).count("1") & 1:
        f, e = f ^ 1, e + 1
    return (True, f, e) if e <= correct else (False, word, e)


def address_word(address, function):
    return codeword((address >> 3) << 2 | function)


def message_word(payload20):
    return codeword(1 << 20 | payload20 & 0xFFFFF)


def _payloads(bits, fill):
    while len(bits) % 20:
        bits.append(fill[len(bits) % len(fill)] if fill else 0)
    return [int("".join(map(str, bits[i:i + 20])), 2) for i in range(0, len(bits), 20)]


def alpha_words(text):
    """7-bit characters, least significant bit first, across the 20-bit payloads; NUL bits fill the last word"""
    return [message_word(p) for p in _payloads([ord(ch) >> i & 1 for ch in text for i in range(7)], None)]


def numeric_words(text):
    """4-bit BCD digits, least significant bit first; spaces fill the last word"""
    digits = [NUMERIC.index(ch) for ch in text]
    while len(digits) % 5:
        digits.append(NUMERIC.index(" "))
    return [message_word(p) for p in _payloads([d >> i & 1 for d in digits for i in range(4)], None)]


def text_of(m, mode="auto"):
    """a record's text by the header's rule"""
    if mode == "auto":
        mode = "numeric" if m["function"] == 0 else "alpha"
    width = 4 if mode == "numeric" else 7
    n = int(m["nwords"])
    bits = [(int(m["words"][i]) >> (30 - k)) & 1 for i in range(n) for k in range(20)]
    bad = [(int(m["bad"][i // 32]) >> (i % 32)) & 1 for i in range(n) for _ in range(20)]
    vals = [(sum(bits[i + k] << k for k in range(width)), any(bad[i:i + width])) for i in range(0, len(bits) - width + 1, width)]
    if mode == "alpha":
        while vals and not vals[-1][1] and vals[-1][0] in (0, 3, 4):
            vals.pop()
    return "".join("?" if b else NUMERIC[v] if width == 4 else chr(v) if 0x20 <= v <= 0x7E else "." for v, b in vals)


# ---------------- the bit bank ----------------

_TABLES = {}


def _bank_tables(baud):
    if baud not in _TABLES:
        L, step, H, B, _ = GEOM[baud]
        tau = np.arange(H)[:, None]
        j = np.arange(B)[None, :]
        t0 = tau * step + L * (j - (tau > 0))
        n0 = -((-t0) // 12)
        n1 = -((-(t0 + L)) // 12)
        k = n1 - n0
        i = np.arange(k.max())
        idx = LEAD + n0[..., None] + i
        live = i < k[..., None]
        assert idx[live].min() == LEAD + {512: -29, 1200: -12, 2400: -6}[baud] and idx[live].max() == LEAD + WAVE_BATCH - 1
        _TABLES[baud] = np.where(live, idx, 0), live, k.astype(F32)
    return _TABLES[baud]


def tree(a):
    """[..., n >= 64] summed in the header's order: 64 running sums, then the halving tree"""
    n = a.shape[-1]
    s = a[..., :64].copy()
    for p in range(64, n, 64):
        m = min(64, n - p)
        s[..., :m] = s[..., :m] + a[..., p:p + m]
    for h in (32, 16, 8, 4, 2, 1):
        s = s[..., :h] + s[..., h:2 * h]
    return s[..., 0]


def bank(staged, baud):
    """staged float32 [nb, 2036] (the lead's 36, then the block) -> (bits uint8 [nb, 2, H, B], Q float32 [nb, 2, H])"""
    idx, live, k = _bank_tables(baud)
    x = staged[:, idx]  # [nb, H, B, kmax]
    s = x[..., 0]
    for i in range(1, idx.shape[-1]):
        s = np.where(live[..., i], s + x[..., i], s)
    mu = tree(staged[:, LEAD:]) / F32(2000.0)
    v = np.stack([s, s - k * mu[:, None, None]], axis=1)  # [nb, 2, H, B]
    return (v < 0).astype(np.uint8), tree(np.abs(v))


def pack(c, W):
    """bits [..., B] -> words uint32 [..., W]"""
    pad = np.zeros(c.shape[:-1] + (W * 32,), np.uint64)
    pad[..., :c.shape[-1]] = c
    return (pad.reshape(c.shape[:-1] + (W, 32)) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def _popcount32(a):
    b = a.astype(np.uint32).view(np.uint8).reshape(a.shape + (4,))
    return _POP8[b].sum(-1)


_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


# ---------------- the walker ----------------

class Walker:
    def __init__(self, st, correct, sync_errors):
        self.phase = int(st["phase"])
        for n in WALKER:
            setattr(self, n, int(st[n]))
        self.msg = np.array(st["msg"], MESSAGE)
        self.correct, self.sync_errors = correct, sync_errors
        self.out = []

    def idle(self):
        self.phase = IDLE
        for n in WALKER:
            setattr(self, n, 0)

    def close(self):
        if self.open:
            self.out.append((self.msg.copy(), self.lane))
            self.msg = np.zeros((), MESSAGE)
            self.open = 0

    def start(self, lane, inverted, mismatches):
        self.idle()
        self.phase, self.lane, self.lane_sync, self.inverted, self.mismatches = TRANSMISSION, lane, lane, inverted, mismatches

    def take(self, bit, batch, t):
        if self.nbits == 0:
            self.wbatch, self.wtwelfth = ((batch - 1) & 0xFFFFFFFF, t + TWELFTHS) if t < 0 else (batch, t)
        self.cur = self.cur << 1 | bit
        self.nbits += 1
        if self.nbits == 32:
            self.word()

    def word(self):
        word, self.cur, self.nbits = self.cur, 0, 0
        if self.pos == 16:
            if bin(word ^ SYNC).count("1") <= self.sync_errors:
                self.pos = self.gbad = 0
            else:
                self.close()
                self.idle()
            return
        good, stored, e = decode(word, self.correct)
        m = self.msg
        if good and stored == IDLE_WORD:
            self.close()
        elif good and not stored >> 31:
            self.close()
            m = self.msg
            m["batch"], m["twelfth"], m["address"], m["function"] = self.wbatch, self.wtwelfth, (stored >> 13 & 0x3FFFF) << 3 | self.pos >> 1, stored >> 11 & 3
            m["corrected"], m["inverted"], m["sync_errors"], m["lane_sync"] = e, self.inverted, self.mismatches, self.lane_sync
            self.open = 1
        elif self.open:
            i = int(m["nwords"])
            if i == MAX_WORDS:
                m["truncated"] = 1
            else:
                m["words"][i] = stored
                if good:
                    m["corrected"] += e
                else:
                    m["bad"][i // 32] |= 1 << (i % 32)
                    m["nbad"] += 1
                m["nwords"] = i + 1
        self.gbad += 0 if good else 1
        self.pos += 1
        if self.pos == 16 and self.gbad == 16:
            self.close()
            self.idle()

    def store(self, st):
        st["phase"] = self.phase
        for n in WALKER:
            st[n] = getattr(self, n)
        st["msg"] = self.msg


def pocsag_model(plane, state=None, en=None, baud=1200, sync_errors=2, preamble_errors=4, correct=1, hold_timing=False, slicers=(0, 1), chunk=256):
    """One call over plane float32 [rows][nb * 2000] from `state` (None: fresh): (messages, bits uint32 [rows][nb][2][H][W],
    q float32 [rows][nb][2][H], row_first [rows + 1], state after).  A disabled row's bits and q are zeros.  preamble_errors None:
    the condition is off.  slicers: (the tests' own) the slicers whose lanes may hit."""
    plane = np.ascontiguousarray(plane, F32)
    L, step, H, B, W = GEOM[baud]
    lanes = 2 * H
    rows, nb = plane.shape[0], plane.shape[1] // WAVE_BATCH
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1).view(STATE).copy()
    en = np.ones(rows, bool) if en is None else np.asarray(en, bool)
    messages, row_first = [], np.zeros(rows + 1, np.uint32)
    bits_out, q_out = np.zeros((rows, nb, 2, H, W), np.uint32), np.zeros((rows, nb, 2, H), F32)
    for r in range(rows):
        row_first[r] = len(messages)
        if not en[r]:
            continue
        st = state[r]
        seq = np.concatenate([np.zeros(2, F32), st["x"], plane[r, :nb * WAVE_BATCH]])
        c, Q = np.zeros((nb, 2, H, B), np.uint8), np.zeros((nb, 2, H), F32)
        for b0 in range(0, nb, chunk):
            n = min(chunk, nb - b0)
            staged = np.lib.stride_tricks.sliding_window_view(seq[b0 * WAVE_BATCH:(b0 + n) * WAVE_BATCH + LEAD], LEAD + WAVE_BATCH)[::WAVE_BATCH]
            c[b0:b0 + n], Q[b0:b0 + n] = bank(staged, baud)
        bits_out[r], q_out[r] = pack(c, W), Q
        c, Q = c.reshape(nb, lanes, B), Q.reshape(nb, lanes)
        old = np.array([[(int(h) >> (63 - i)) & 1 for i in range(64)] for h in st["hist"][:lanes]], np.uint64)  # oldest first
        stream = np.concatenate([old, c.transpose(1, 0, 2).reshape(lanes, nb * B).astype(np.uint64)], axis=1)  # [lanes, 64 + nb B]
        n = nb * B
        w32 = np.zeros((lanes, n + 33), np.uint64)  # w32[:, i] = stream bits i .. i + 31 as a word, the oldest in bit 31
        for i in range(32):
            w32 |= stream[:, i:i + n + 33] << np.uint64(31 - i)
        new, before = w32[:, 33:], w32[:, 1:n + 1]  # the newest 32 bits at slot s of the call (its bit is stream bit 64 + s), and the 32 before them
        m = _popcount32(new ^ np.uint64(SYNC))
        inv = m > 16
        m = np.where(inv, 32 - m, m)
        p = _popcount32(before ^ np.uint64(0xAAAAAAAA))
        p = np.minimum(p, 32 - p)
        hit = (m <= sync_errors) & ((p <= preamble_errors) if preamble_errors is not None else True)
        hit[[g * H + t for g in (0, 1) if g not in slicers for t in range(H)]] = False
        hit_slots = np.flatnonzero(hit.any(0))
        w = Walker(st, correct, sync_errors)
        batch0 = int(st["batch"])
        done = 0  # messages of w.out already recorded

        def flush(b):
            nonlocal done
            for msg, lane in w.out[done:]:
                msg["row"], msg["end_batch"], msg["lane_end"] = r, b, lane
                messages.append(msg)
            done = len(w.out)

        s = 0
        while s < n:
            if w.phase == IDLE:
                k = np.searchsorted(hit_slots, s)
                if k == len(hit_slots):
                    break
                s = int(hit_slots[k])
                b = s // B
                cands = np.flatnonzero(hit[:, s])
                u = min(cands, key=lambda t: (int(m[t, s]), -float(Q[b][t]), t))
                w.start(int(u), int(inv[u, s]), int(m[u, s]))
                s += 1
                continue
            b, j = divmod(s, B)
            skip = False
            batch = (batch0 + b) & 0xFFFFFFFF
            if j == 0 and w.phase == TRANSMISSION and not hold_timing:
                base, tau = w.lane // H * H, w.lane % H
                v = tau
                if Q[b][base + (tau - 1) % H] > Q[b][base + v]:
                    v = (tau - 1) % H
                if Q[b][base + (tau + 1) % H] > Q[b][base + v]:
                    v = (tau + 1) % H
                w.lane = base + v
                skip = (tau, v) == (0, 1)
                if (tau, v) == (1, 0):
                    w.take(int(stream[w.lane, 64 + s - 1]) ^ w.inverted, batch, -L)
                    flush(b)
            if w.phase == TRANSMISSION and not skip:
                tau = w.lane % H
                w.take(int(stream[w.lane, 64 + s]) ^ w.inverted, batch, tau * step + L * (j - (tau > 0)))
                flush(b)
            s += 1
        st["batch"] = (batch0 + nb) & 0xFFFFFFFF
        hist = st["hist"].copy()
        hist[:lanes] = [int("".join(str(int(x)) for x in h), 2) for h in stream[:, -64:]]
        st["hist"] = hist
        w.store(st)
        st["x"] = plane[r, nb * WAVE_BATCH - HISTORY:nb * WAVE_BATCH]
    row_first[rows] = len(messages)
    return (np.array(messages, MESSAGE) if messages else np.zeros(0, MESSAGE)), bits_out, q_out, row_first, state


def run_in_calls(plane, cuts, state=None, masks=None, **kw):
    """the model over consecutive calls of the lengths `cuts`: [(messages, bits, q, row_first, state after)] per call"""
    out, done = [], 0
    for i, n in enumerate(cuts):
        res = pocsag_model(plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], state, None if masks is None else masks[i], **kw)
        out.append(res)
        state, done = res[4], done + n
    return out


# ---------------- the modulator ----------------

def transmission(pages, preamble=48, tail_groups=0):
    """The bits of a transmission: `preamble` alternating bits, then groups of SYNC and 16 words.  pages: (address, function, message
    words); an address word waits for its frame (address & 7: words 2 f, 2 f + 1), IDLE fills, a message runs on through the
    following groups."""
    words = []
    for address, function, msg in pages:
        while len(words) % 16 != 2 * (address & 7):
            words.append(IDLE_WORD)
        words += [address_word(address, function)] + list(msg)
    words.append(IDLE_WORD)
    while len(words) % 16:
        words.append(IDLE_WORD)
    words += [IDLE_WORD] * (16 * tail_groups)
    return bits_of_words(words, preamble)


def bits_of_words(words, preamble):
    """`preamble` alternating bits, then the words 16 to a group, SYNC before each group"""
    bits = [(i + 1) & 1 for i in range(preamble)]
    for i, wd in enumerate(words):
        if i % 16 == 0:
            bits += [SYNC >> (31 - k) & 1 for k in range(32)]
        bits += [wd >> (31 - k) & 1 for k in range(32)]
    return bits


def render(bits, start_twelfth, n, baud=1200, amp=0.3, ppm=0.0, dc=0.0, inverted=False, noise=0.0, seed=0):
    """float64 [n]: NRZ of the bits from twelfth `start_twelfth` of the row's first sample on, the bit clock fast by ppm: bit 1 is
    -amp (the lower frequency), bit 0 +amp, the other way round if inverted; silence before and behind; dc on every sample."""
    bits = np.asarray(bits, np.int64)
    blen = GEOM[baud][0] / (1.0 + ppm * 1e-6)
    t = 12.0 * np.arange(n, dtype=np.float64) - start_twelfth
    k = np.floor(t / blen).astype(np.int64)
    on = (k >= 0) & (k < len(bits))
    level = np.where(bits[np.clip(k, 0, len(bits) - 1)] == 1, -amp, amp) * (-1.0 if inverted else 1.0)
    x = np.where(on, level, 0.0) + dc
    if noise:
        x = x + np.random.default_rng(seed).normal(0.0, noise, n)
    return x


def noise(n, sigma, seed):
    return np.random.default_rng(seed).normal(0.0, sigma, n)


def voice_like(n, seed):
    """harmonics of a gliding pitch under a formant-like tilt, keyed in syllables at about 4 Hz (the other stages' voice builder)"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    x = sum(np.sin(k * ph + rng.uniform(0, 6.28)) / (1.0 + abs(k * 140.0 - 700.0) / 300.0) for k in range(1, 20))
    syll = np.clip(np.sin(2 * np.pi * 4.1 * t + rng.uniform(0, 6.28)) + 0.3, 0.0, 1.0)
    return 0.1 * x * syll


ALPHA_TEXT = "FIRE ALARM 12 HIGH ST"
LONG_TEXT = "".join(chr(0x20 + (7 * i) % 95) for i in range(60))  # 60 characters, 21 words: from frame 5 on it crosses into the next group
NUMERIC_TEXT = "0123456789*U -)(4207"


def builder_rows(baud):
    """[(name, samples float64 [NBATCHES * 2000], [(address, function, text)] sent)]"""
    n = NBATCHES[baud] * WAVE_BATCH
    L = GEOM[baud][0]
    alpha = (0x12345, 3, alpha_words(ALPHA_TEXT))
    numeric = (0x0ABCD2, 0, numeric_words(NUMERIC_TEXT))
    tone = (0x1F0F6, 2, [])
    longp = (0x1555D, 3, alpha_words(LONG_TEXT))
    text = {id(alpha): ALPHA_TEXT, id(numeric): NUMERIC_TEXT, id(tone): "", id(longp): LONG_TEXT}
    sent = lambda *pages: [(pg[0], pg[1], text[id(pg)]) for pg in pages]  # noqa: E731
    start = 5000 + 7 * L // 3
    rows = [
        ("an alphanumeric page", render(transmission([alpha]), start, n, baud), sent(alpha)),
        ("a numeric page", render(transmission([numeric]), start + 111, n, baud), sent(numeric)),
        ("a tone-only page", render(transmission([tone]), start + 222, n, baud), sent(tone)),
        ("inverted polarity", render(transmission([alpha]), start + 333, n, baud, inverted=True), sent(alpha)),
        ("a DC offset", render(transmission([alpha]), start + 444, n, baud, dc=0.5), sent(alpha)),
        ("a message across two groups", render(transmission([longp]), 1000, n, baud), sent(longp)),
        ("two pages and a tone in one group", render(transmission([(0x10, 1, alpha[2]), (0x0ABCD6, 0, numeric[2]), tone]), start + 555, n, baud),
         [(0x10, 1, ALPHA_TEXT), (0x0ABCD6, 0, NUMERIC_TEXT), (0x1F0F6, 2, "")]),
        ("a clock 100 ppm fast", render(transmission([alpha]), start + 666, n, baud, ppm=100.0), sent(alpha)),
        ("noise 20 dB under the levels", render(transmission([alpha]), start + 777, n, baud, noise=0.03, seed=5), sent(alpha)),
        ("white noise", noise(n, 0.2, 11), []),
        ("silence", np.zeros(n), []),
    ]
    if baud != 512:  # (at 512 baud the full preamble and a group are 17.5 batches: full_preamble() below)
        rows.append(("the full preamble", render(transmission([alpha], preamble=576), 3000, n, baud), sent(alpha)))
    return rows


def full_preamble_512(nb=48):
    """512 baud, 48 batches: the full preamble of 576 bits and two groups, the long page from frame 5 on"""
    longp = (0x1555D, 3, alpha_words(LONG_TEXT))
    return render(transmission([longp], preamble=576), 7000, nb * WAVE_BATCH, 512), [(0x1555D, 3, LONG_TEXT)]


def found(messages, row=None):
    """[(address, function, text)] of the records (of one row)"""
    return [(int(m["address"]), int(m["function"]), text_of(m)) for m in messages if row is None or m["row"] == row]
