"""The packet decoder stage's definition (include/mi_airband.h "packet decoder stage") restated in numpy and plain Python, and the
signals its tests use.

The bit bank is array operations in the header's order (float32, one rounding per operation) over all bits of a batch; the
deframers run lane by lane in Python integers -- the lanes are independent, so each walks the whole call on its own and only the
candidates meet, sorted by slot and lane, in the ordering rule --; the CRC goes bit by bit.  The modulator is written independently
of the demodulator: HDLC bits, NRZI tones, the phase at every bit's start accumulated in float64, and the sine of the phase at every
sample time, for any start time, clock offset and per-tone level."""
import numpy as np

F32 = np.float32
RATE, WAVE_BATCH, NB = 16000, 2000, 48
HISTORY, LEAD, NTAU, NSLICERS, NLANES, NBITS, NWORDS, MIN_BYTES, MAX_BYTES, RAW = 14, 16, 10, 3, 30, 150, 5, 17, 330, 332
THIRDS = 3 * WAVE_BATCH
WAIT, FRAME = 0, 1
RESIDUE = 0xF0B8
FRAME_REC = np.dtype([("row", "<u4"), ("batch", "<u4"), ("third", "<u4"), ("end_batch", "<u4"), ("nbytes", "<u2"), ("lane", "u1"), ("naddr", "u1"),
                      ("bytes", "u1", (RAW,))])
LANE_FIELDS = ("start", "nbytes", "crc", "prev", "ones", "phase", "nbits", "cur")
STATE = np.dtype([("x", "<f4", (HISTORY,)), ("batch", "<u8"), ("last_end", "<u8"), ("start", "<u8", (NLANES,)), ("nbytes", "<u2", (NLANES,)),
                  ("crc", "<u2", (NLANES,)), ("prev", "u1", (NLANES,)), ("ones", "u1", (NLANES,)), ("phase", "u1", (NLANES,)), ("nbits", "u1", (NLANES,)),
                  ("cur", "u1", (NLANES,)), ("zero", "u1", (2,)), ("bytes", "u1", (NLANES, RAW))])
assert STATE.itemsize == 10544 and FRAME_REC.itemsize == 352


def fresh_state(rows):
    return np.zeros(rows, STATE)


def max_frames(nb):
    return 1 + NBITS * nb // 143


def templates():
    rho = np.arange(40, dtype=np.float64)
    return np.stack([np.cos(2 * np.pi * 1200.0 * rho / 48000.0), np.sin(2 * np.pi * 1200.0 * rho / 48000.0),
                     np.cos(2 * np.pi * 2200.0 * rho / 48000.0), np.sin(2 * np.pi * 2200.0 * rho / 48000.0)]).astype(F32)


def crc_register(bits, crc=0xFFFF):
    """the frame check's register over bits, one at a time: it shifts right, the data enter least significant bit first"""
    for d in bits:
        fb = (crc ^ d) & 1
        crc >>= 1
        if fb:
            crc ^= 0x8408
    return crc


def bits_of(data):
    return [(b >> i) & 1 for b in data for i in range(8)]


def crc_x25(data):
    """CRC-16/X.25 as it is sent: the register from 0xFFFF, complemented"""
    return crc_register(bits_of(data)) ^ 0xFFFF


FLAG_RESIDUE = crc_register([0, 1, 1, 1, 1, 1], RESIDUE)


# ---------------- the bit bank ----------------

def _bank_tables():
    tau = np.arange(NTAU)[:, None]
    j = np.arange(NBITS)[None, :]
    t0 = 4 * tau + 40 * (j - (tau > 0))
    n0 = -((-t0) // 3)  # ceil
    rho0 = 3 * n0 - t0
    i = np.arange(14)
    idx = LEAD + n0[..., None] + i
    rho = rho0[..., None] + 3 * i
    fourteen = rho0 == 0
    assert idx.min() == LEAD - 12 and idx[..., :13].max() <= LEAD + WAVE_BATCH - 1 and idx[fourteen].max() <= LEAD + WAVE_BATCH - 1 and rho[fourteen].max() == 39
    # every bit's last sample lies in the batch, and the bit after the last slot's does not
    last = n0 + np.where(fourteen, 13, 12)
    assert last.min() >= 0 and last.max() <= WAVE_BATCH - 1
    idx[..., 13] = np.where(fourteen, idx[..., 13], 0)  # (a bit of thirteen samples: the fourteenth product is not taken)
    rho[..., 13] = np.where(fourteen, rho[..., 13], 0)
    return idx, rho, fourteen


_IDX, _RHO, _FOURTEEN = _bank_tables()


def bank(staged, gain):
    """staged float32 [..., 2016] (the lead's 16, then the block) -> tone bits uint8 [..., 3, 10, 150]"""
    x = staged[..., _IDX]  # [..., 10, 150, 14]
    sums = []
    for h in templates():
        p = x * h[_RHO]
        s = p[..., 0]
        for i in range(1, 13):
            s = s + p[..., i]
        sums.append(np.where(_FOURTEEN, s + p[..., 13], s))
    pm = sums[0] * sums[0] + sums[1] * sums[1]
    ps = sums[2] * sums[2] + sums[3] * sums[3]
    assert pm.dtype == F32 and ps.dtype == F32
    return np.stack([(pm >= F32(g) * ps) for g in gain], axis=-3).astype(np.uint8)


def pack(t):
    """tone bits [..., 150] -> words uint32 [..., 5]"""
    pad = np.zeros(t.shape[:-1] + (NWORDS * 32,), np.uint64)
    pad[..., :NBITS] = t
    return (pad.reshape(t.shape[:-1] + (NWORDS, 32)) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


# ---------------- the deframers and the ordering rule ----------------

def call_char(byte):
    c = byte >> 1
    return 0x41 <= c <= 0x5A or 0x30 <= c <= 0x39 or c == 0x20


def naddr_of(b):
    """the number of addresses of a frame (bytes, the check included) whose address field is well formed, else 0"""
    last = next((i for i in range(min(70, len(b) - 3)) if b[i] & 1), None)
    if last is None or last % 7 != 6 or last < 13:
        return 0
    return (last + 1) // 7 if all(call_char(b[k]) for k in range(last) if k % 7 != 6) else 0


def slot_end(tau, j):
    return 4 * tau + 40 * (j + 1 - (tau > 0))


def run_lane(st, l, tones, base):
    """deframer l of the row state st over its tone bits of the call (a list), slot 0 of the call's first batch ending at
    base + slot_end(tau, 0): the candidates [(global slot, l, start, end, bytes)], the lane's state written back"""
    tau = l % NTAU
    prev, ones, phase, nbits, cur, crc, start = (int(st[n][l]) for n in ("prev", "ones", "phase", "nbits", "cur", "crc", "start"))
    data = [int(v) for v in st["bytes"][l][:int(st["nbytes"][l])]]
    cands = []
    for s, t in enumerate(tones):
        d = 1 if t == prev else 0
        prev, n = t, ones
        ones = min(n + 1, 7) if d else 0
        if n >= 5:
            if n == 6 and d:
                phase, nbits, cur, crc, start, data = WAIT, 0, 0, 0, 0, []
            elif n == 6:
                end = base + (s // NBITS) * THIRDS + slot_end(tau, s % NBITS)
                if phase == FRAME and nbits == 6 and len(data) >= MIN_BYTES and crc == FLAG_RESIDUE:
                    cands.append((s, l, start, end, data))
                phase, nbits, cur, crc, start, data = FRAME, 0, 0, 0xFFFF, end, []
            continue
        if phase != FRAME:
            continue
        cur |= d << nbits
        fb = (crc ^ d) & 1
        crc >>= 1
        if fb:
            crc ^= 0x8408
        nbits += 1
        if nbits == 8:
            if len(data) == MAX_BYTES:
                phase, nbits, cur, crc, start, data = WAIT, 0, 0, 0, 0, []
            else:
                data.append(cur)
                nbits = cur = 0
    for n, v in (("prev", prev), ("ones", ones), ("phase", phase), ("nbits", nbits), ("cur", cur), ("crc", crc), ("start", start), ("nbytes", len(data))):
        st[n][l] = v
    st["bytes"][l] = data + [0] * (RAW - len(data))
    return cands


def ax25_model(plane, state=None, en=None, gain=None, strict=True):
    """One call over plane float32 [rows][nb * 2000] from `state` (None: fresh): (frames, bits uint32 [rows][nb][3][10][5],
    row_first [rows + 1], state after).  A disabled row's bits are zeros."""
    plane = np.ascontiguousarray(plane, F32)
    rows, nb = plane.shape[0], plane.shape[1] // WAVE_BATCH
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1).view(STATE).copy()
    en = np.ones(rows, bool) if en is None else np.asarray(en, bool)
    gain = DEFAULT_GAIN if gain is None else gain
    frames, row_first = [], np.zeros(rows + 1, np.uint32)
    bits_out = np.zeros((rows, nb, NSLICERS, NTAU, NWORDS), np.uint32)
    for r in range(rows):
        row_first[r] = len(frames)
        if not en[r]:
            continue
        st = state[r]
        seq = np.concatenate([np.zeros(2, F32), st["x"], plane[r, :nb * WAVE_BATCH]])
        staged = np.stack([seq[b * WAVE_BATCH:b * WAVE_BATCH + LEAD + WAVE_BATCH] for b in range(nb)])
        t = bank(staged, gain)  # [nb, 3, 10, 150]
        bits_out[r] = pack(t)
        base = THIRDS * int(st["batch"])
        cands = []
        for l in range(NLANES):
            cands += run_lane(st, l, t[:, l // NTAU, l % NTAU, :].reshape(-1).tolist(), base)
        last_end = int(st["last_end"])
        for s, l, start, end, data in sorted(cands, key=lambda c: c[:2]):
            if start + 40 < last_end:
                continue
            a = naddr_of(data)
            if strict and not a:
                continue
            f = np.zeros((), FRAME_REC)
            f["row"], f["batch"], f["third"], f["end_batch"] = r, (start // THIRDS) & 0xFFFFFFFF, start % THIRDS, s // NBITS
            f["nbytes"], f["lane"], f["naddr"] = len(data), l, a
            f["bytes"][:len(data)] = data
            frames.append(f)
            last_end = end
        st["last_end"] = last_end
        st["batch"] = int(st["batch"]) + nb
        st["x"] = plane[r, nb * WAVE_BATCH - HISTORY:nb * WAVE_BATCH]
    row_first[rows] = len(frames)
    return (np.array(frames, FRAME_REC) if frames else np.zeros(0, FRAME_REC)), bits_out, row_first, state


def run_in_calls(plane, cuts, state=None, masks=None, **kw):
    """the model over consecutive calls of the lengths `cuts`: [(frames, bits, row_first, state after)] per call"""
    out, done = [], 0
    for i, n in enumerate(cuts):
        res = ax25_model(plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], state, None if masks is None else masks[i], **kw)
        out.append(res)
        state, done = res[3], done + n
    return out


def tnc2(f):
    """a record's TNC2 line"""
    b = [int(v) for v in f["bytes"][:int(f["nbytes"])]]
    a = naddr_of(b)
    assert a

    def call(k):
        txt = "".join(chr(v >> 1) for v in b[7 * k:7 * k + 6]).rstrip(" ")
        ssid = b[7 * k + 6] >> 1 & 15
        return txt + (f"-{ssid}" if ssid else "")

    heard = [k for k in range(2, a) if b[7 * k + 6] & 0x80]
    path = "".join("," + call(k) + ("*" if heard and k == heard[-1] else "") for k in range(2, a))
    at = 7 * a + (2 if b[7 * a] | 0x10 == 0x13 else 1)
    return f"{call(1)}>{call(0)}{path}:" + "".join(chr(v) if 0x20 <= v <= 0x7E else "." for v in b[at:-2])


# ---------------- the modulator ----------------

def address(callsign, ssid=0, last=False, heard=False):
    return [ord(ch) << 1 for ch in callsign.ljust(6)] + [0x60 | ssid << 1 | (1 if last else 0) | (0x80 if heard else 0)]


def ui_frame(src="N0CALL", dst="APRS", digis=(), info=b"", src_ssid=0, dst_ssid=0, control=0x03, pid=0xF0):
    """the bytes of a UI frame with its check behind it.  digis: [(callsign, ssid, heard)]"""
    body = address(dst, dst_ssid) + address(src, src_ssid, last=not digis)
    for k, (call, ssid, heard) in enumerate(digis):
        body += address(call, ssid, last=k == len(digis) - 1, heard=heard)
    body += [control, pid] + list(info)
    crc = crc_x25(body)
    return body + [crc & 0xFF, crc >> 8]


def stuffed(data):
    out, run = [], 0
    for d in bits_of(data):
        out.append(d)
        run = run + 1 if d else 0
        if run == 5:
            out.append(0)
            run = 0
    return out


FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def burst_bits(frames, before=8, after=2, between=1):
    """HDLC data bits: `before` flags, the frames stuffed with `between` flags between them, `after` flags"""
    bits = FLAG * before
    for k, f in enumerate(frames):
        if k:
            bits = bits + FLAG * between
        bits = bits + stuffed(f)
    return bits + FLAG * after


def modulate(bits, start_third, n, amp=0.3, ppm=0.0, space_gain=1.0, noise=0.0, seed=0):
    """float64 [n]: continuous-phase AFSK of the HDLC data bits from third `start_third` of the row's first sample on (any real
    number), the bit clock fast by ppm.  NRZI: a 0 changes the tone, a 1 keeps it; the tone before the first bit is mark (1200 Hz).
    The space tone (2200 Hz) is sent at space_gain times the level.  Silence before and behind; seeded white noise of sigma `noise`
    over all of it."""
    bits = np.asarray(bits, np.int64)
    tone = np.cumsum(1 - bits) % 2  # 0 = mark, 1 = space
    freq = np.where(tone == 1, 2200.0, 1200.0)
    blen = 40.0 / (1.0 + ppm * 1e-6)  # thirds a bit
    adv = 2.0 * np.pi * freq * blen / 48000.0
    phase0 = np.concatenate([[0.0], np.cumsum(adv)[:-1]])
    t = 3.0 * np.arange(n, dtype=np.float64) - start_third
    k = np.floor(t / blen).astype(np.int64)
    on = (k >= 0) & (k < len(bits))
    kk = np.clip(k, 0, len(bits) - 1)
    x = np.where(on, amp * np.where(tone[kk] == 1, space_gain, 1.0) * np.sin(phase0[kk] + 2.0 * np.pi * freq[kk] * (t - kk * blen) / 48000.0), 0.0)
    if noise:
        x = x + np.random.default_rng(seed).normal(0.0, noise, n)
    return x


def voice_like(n, seed):
    """harmonics of a gliding pitch under a formant-like tilt, keyed in syllables at about 4 Hz"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6.28))
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    x = sum(np.sin(k * ph + rng.uniform(0, 6.28)) / (1.0 + abs(k * 140.0 - 700.0) / 300.0) for k in range(1, 20))
    syll = np.clip(np.sin(2 * np.pi * 4.1 * t + rng.uniform(0, 6.28)) + 0.3, 0.0, 1.0)
    return 0.1 * x * syll


# tools/ax25_classes.py: the power tilt between 1200 and 2200 Hz behind the project's NFM path for a flat-deviation
# transmitter is gain[2]; gain[1] is its square root.
DEFAULT_GAIN = (1.0, 1.6432, 2.7)
TILT_DOWN, TILT_UP = "space down by the tilt, 6 dB over the noise", "space 26 dB up"
SLICERS_ALONE = {TILT_DOWN: [False, True, True], TILT_UP: [True, True, False]}  # which slicer decodes the row with the other two out of reach
DIGIS8 = [(f"DIGI{k}", k, k < 3) for k in range(1, 9)]
SHORT = dict(src="N0CALL", src_ssid=7, dst="APRS", info=b"!4903.50N/07201.75W-hello")
LONGEST = dict(src="LONG", src_ssid=15, dst="APZ123", digis=DIGIS8, info=bytes((37 * i + 11) % 256 for i in range(256)))


def builders():
    """[(name, row float64 [NB * 2000], the frames' bytes a default handle must find, in order; those only strict off finds)]"""
    n = NB * WAVE_BATCH
    out = []

    def add(name, x, found=(), loose=()):
        out.append((name, x, list(found), list(loose)))

    def line(f):
        return bytes(f)

    def one(f, start, **kw):
        return modulate(burst_bits([f]), start, n, **kw)

    base = 3 * 900
    short, longest = ui_frame(**SHORT), ui_frame(**LONGEST)
    assert len(longest) == MAX_BYTES
    add("a short UI frame", one(short, base), [line(short)])
    add("the same inverted", -one(short, base + 17), [line(short)])
    add("the longest frame", one(longest, base + 5), [line(longest)])
    ff = ui_frame(src="FF", dst="STUFF", info=b"\xff" * 60)
    add("information of all 0xFF", one(ff, base + 9), [line(ff)])
    f1, f2 = ui_frame(src="ONE", info=b"first"), ui_frame(src="TWO", src_ssid=2, info=b"second")
    add("two frames sharing one flag", modulate(burst_bits([f1, f2], between=1), base + 2, n), [line(f1), line(f2)])
    add("two frames 50 flags apart", modulate(burst_bits([f1, f2], between=50), base + 22, n), [line(f1), line(f2)])
    half = stuffed(short)[:100]
    add("an abort inside a frame", modulate(FLAG * 8 + half + [1] * 9 + FLAG * 3 + stuffed(f2) + FLAG * 2, base + 31, n), [line(f2)])
    flipped = burst_bits([short])
    flipped[64 + 90] ^= 1
    add("one flipped bit", modulate(flipped, base + 13, n))
    f16 = ui_frame(src="A", dst="B", info=b"")[:-3]
    f16 = f16[:14] + [crc_x25(f16[:14]) & 0xFF, crc_x25(f16[:14]) >> 8]
    assert len(f16) == 16 and crc_register(bits_of(f16)) == RESIDUE
    add("a 16-byte frame", one(f16, base + 3))
    f17 = ui_frame(src="A", dst="B", info=b"", pid=0)[:-3]
    f17 = f17[:15] + [crc_x25(f17[:15]) & 0xFF, crc_x25(f17[:15]) >> 8]
    assert len(f17) == MIN_BYTES
    add("a 17-byte frame", one(f17, base + 7), [line(f17)])
    f331 = ui_frame(**dict(LONGEST, info=LONGEST["info"] + b"!"))
    assert len(f331) == MAX_BYTES + 1
    add("a 331-byte frame", one(f331, base + 11))
    bad = ui_frame(src="n0call", info=b"lower case")
    add("a bad callsign byte", one(bad, base + 19), [], [line(bad)])
    g = 10 ** (-6 / 20)
    add("space 6 dB down", one(short, base + 6, space_gain=g), [line(short)])
    add("space 6 dB up", one(short, base + 14, space_gain=1 / g), [line(short)])
    add("a clock 50 ppm fast", one(longest, base + 1, ppm=50.0), [line(longest)])
    add("a clock 50 ppm slow", one(longest, base + 1, ppm=-50.0), [line(longest)])
    cut = one(short, base + 4)
    cut[900 + 2000:] = 0.0
    add("a frame cut by silence", cut)
    add("a frame across batch 20 and 21", one(short, 21 * THIRDS - 40 * 200), [line(short)])
    add("amplitude 1e-3", one(short, base + 12, amp=1e-3), [line(short)])
    add("a frame in noise", one(short, base + 16, noise=0.3 / np.sqrt(2) / 10 ** (20 / 20), seed=201), [line(short)])
    # one slicer loses a frame that another keeps (seeds chosen on the model, tools/ax25_classes.py has the statistics): the space tone
    # down by the measured tilt 6 dB over the noise is lost on the flat slicer 0 and kept on 1 and 2; a space tone 26 dB up is kept on
    # 0 and 1 and lost on 2, on noise-free audio
    add(TILT_DOWN, one(short, base + 2, space_gain=1.0 / np.sqrt(DEFAULT_GAIN[2]), noise=0.3 / np.sqrt(2) / 10 ** (6 / 20), seed=402), [line(short)])
    add(TILT_UP, one(short, base + 13, space_gain=10 ** (26 / 20)), [line(short)])
    add("silence", np.zeros(n))
    add("-0.0 throughout", np.full(n, -0.0))
    add("subnormal values", np.random.default_rng(204).choice([1e-40, -3e-41, 1e-45, 0.0, 2e-39], n))
    add("white noise", np.random.default_rng(202).normal(0.0, 0.2, n))
    add("voice-like", voice_like(n, 203))
    return out


def stacked():
    """(names, plane float32 [rows][NB * 2000], found per row, loose per row)"""
    b = builders()
    return [x[0] for x in b], np.ascontiguousarray(np.stack([x[1] for x in b]).astype(F32)), [x[2] for x in b], [x[3] for x in b]


START_BATCHES = 3


def start_thirds():
    """(plane float32 [40][3 * 2000], the frame's bytes): the short frame at every start third modulo 40, in rows of their own"""
    f = ui_frame(**SHORT)
    return np.stack([modulate(burst_bits([f]), 600 + s, START_BATCHES * WAVE_BATCH) for s in range(40)]).astype(F32), bytes(f)


# ---------------- seeded states: the ordering rule, branch by branch, and the capacity bound ----------------

def seed_lane(st, l, frame, k, start, extra=()):
    """Lane l of the row state st inside `frame` with its first k bytes whole and the bits `extra` of the running byte behind them,
    opened at `start`, the previous tone mark.  Returns the HDLC bits the lane has yet to see up to the frame's last."""
    sent = stuffed(frame[:k])
    run = 0
    for d in sent + list(extra):
        run = run + 1 if d else 0
    assert run < 5, "cut where no stuffed bit is pending"
    st["phase"][l], st["nbytes"][l], st["prev"][l], st["ones"][l], st["start"][l] = FRAME, k, 1, run, start
    st["crc"][l] = crc_register(bits_of(frame[:k]) + list(extra))
    st["nbits"][l], st["cur"][l] = len(extra), sum(d << i for i, d in enumerate(extra))
    st["bytes"][l][:k] = frame[:k]
    return stuffed(frame)[len(sent):]


SEED_BATCH = 5
SEED_START = SEED_BATCH * THIRDS - 40 * 400
ORDER_CASES = [("two lanes close in one slot", (0, 10), 0, 1), ("a duplicate one slot later", (0, 1), 0, 1),
               ("a frame that begins exactly at the last record's end", (0,), SEED_START, 1),
               ("a frame that begins one bit before the last record's end", (0,), SEED_START + 40, 1),
               ("a frame that begins two bits before the last record's end", (0,), SEED_START + 80, 0)]


def ordering_cases():
    """(names, state [rows], plane float32 [rows][2000], records expected per row): every row's seeded lanes are 30 bytes into the
    short frame, whose rest the plane sends on hypothesis 0's grid; last_end is seeded around the frame's start"""
    f = ui_frame(**SHORT)
    st = fresh_state(len(ORDER_CASES))
    rest = None
    for r, (_, lanes, last_end, _) in enumerate(ORDER_CASES):
        st[r]["batch"], st[r]["last_end"] = SEED_BATCH, last_end
        for l in lanes:
            rest = seed_lane(st[r], l, f, 30, SEED_START)
    x = modulate(rest + FLAG * 3, 0, WAVE_BATCH).astype(F32)
    return [c[0] for c in ORDER_CASES], st, np.stack([x] * len(ORDER_CASES)), [c[3] for c in ORDER_CASES]


MINIMAL = ui_frame(src="A", dst="B", info=b"", pid=0)[:15]
MINIMAL = MINIMAL + [crc_x25(MINIMAL) & 0xFF, crc_x25(MINIMAL) >> 8]


def capacity_case(nb):
    """(state [1], plane float32 [1][nb * 2000]): lane 0 holds a whole 17-byte frame and the first three bits of its closing flag,
    which ends in the call's slot 4; behind it 17-byte frames sharing their flags, one closing every 144 slots:
    1 + (150 nb - 5) // 144 records, which is max_frames(nb) for nb = 1, 2"""
    assert len(MINIMAL) == MIN_BYTES and naddr_of(MINIMAL) == 2
    st = fresh_state(1)
    st[0]["batch"] = SEED_BATCH
    rest = seed_lane(st[0], 0, MINIMAL, MIN_BYTES, SEED_START, extra=(0, 1, 1))
    assert rest == []
    bits = [1, 1, 1, 1, 0] + (stuffed(MINIMAL) + FLAG) * (nb + 1)
    return st, modulate(bits, 0, nb * WAVE_BATCH).astype(F32)[None, :]


BAD_BLOBS = [("prev", 2, "a counter beyond its range"), ("ones", 8, "a counter beyond its range"), ("nbits", 8, "a counter beyond its range"),
             ("cur", 8, "a counter beyond its range"), ("nbytes", 331, "a counter beyond its range"), ("phase", 2, "an unknown lane phase"),
             ("crc", 0x1234, "a crc that the bytes do not give"), ("start", SEED_BATCH * THIRDS + 1, "a frame begins behind the row's last batch"),
             ("start", SEED_BATCH * THIRDS + slot_end(3, -1) - 40 * (8 * 9 + 3) + 40, "later than its collected bits allow")]


def bad_blobs():
    """[(what, blob of one row, the refusal's words)]: a good mid-frame blob with one field made impossible at a time"""
    good = fresh_state(1)
    good[0]["batch"] = SEED_BATCH
    seed_lane(good[0], 3, ui_frame(**SHORT), 9, SEED_START, extra=(1, 0, 1))
    out = [("the good blob", good, None)]
    latest = good.copy()
    latest[0]["start"][3] = SEED_BATCH * THIRDS + slot_end(3, -1) - 40 * (8 * 9 + 3)
    out.append(("the latest start its bits allow", latest, None))
    for field, value, words in BAD_BLOBS:
        b = good.copy()
        b[0][field][3] = value
        out.append((f"{field} = {value}", b, words))
    for what, field, value, words in (("a byte behind the ones taken", "bytes", None, "a byte set behind the ones taken"),
                                      ("a waiting lane with a crc", "crc", None, "a waiting lane with a frame field set"),
                                      ("zero not 0", "zero", None, "the zero field is not 0"), ("batch 2^40", "batch", 1 << 40, "a batch count at or beyond 2^40"),
                                      ("last_end behind the last batch", "last_end", SEED_BATCH * THIRDS + 1, "the last record ends behind the row's last batch")):
        b = good.copy()
        if field == "bytes":
            b[0]["bytes"][3][9] = 1
        elif field == "crc":
            b[0]["crc"][4] = 1
        elif field == "zero":
            b[0]["zero"][1] = 1
        else:
            b[0][field] = value
        out.append((what, b, words))
    return out
