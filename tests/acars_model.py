"""The ACARS decoder stage's definition (include/mi_airband.h "ACARS decoder stage") restated in numpy, and the signals its tests use.

The bit bank is array operations in the header's order (float32, one rounding per operation); the sync compare is a sliding window
over each hypothesis' change bits; the walker is plain Python; the CRC goes bit by bit.  The modulator is written independently of
the demodulator: a bit sequence, the phase at every bit's start accumulated in float64, and the sine of the phase at every sample
time, for any start time and clock offset."""
import math

import numpy as np

F32 = np.float32
RATE, WAVE_BATCH, NB = 16000, 2000, 12
HISTORY, LEAD, NTAU, NBITS, NWORDS, SYNC_BITS, HEAD, MAX_BYTES, RAW = 6, 8, 20, 300, 10, 39, 12, 240, 248
THIRDS = 3 * WAVE_BATCH
IDLE, FRAME = 0, 1
ETX, ETB, SOH, SYN, DEL = 0x03, 0x17, 0x01, 0x16, 0x7F
FRAME_REC = np.dtype([("row", "<u4"), ("batch", "<u4"), ("third", "<u4"), ("tau_sync", "u1"), ("tau_end", "u1"), ("sync_errors", "u1"), ("crc_ok", "u1"),
                      ("nbytes", "<u2"), ("parity_errors", "u1"), ("end", "u1"), ("end_batch", "<u4"), ("bytes", "u1", (RAW,))])
WALKER = ("u", "prev", "nbits", "cur", "nbytes", "tail", "crc", "parity_errors", "start_batch", "start_third", "tau_sync", "mismatches", "end")
STATE = np.dtype([("x", "<f4", (HISTORY,)), ("batch", "<u4"), ("phase", "<u4"), ("hist", "<u8", (NTAU,))] + [(n, "<u4") for n in WALKER + ("zero",)] +
                 [("bytes", "u1", (RAW,))])
MASK38 = (1 << 38) - 1


def fresh_state(rows):
    return np.zeros(rows, STATE)


def templates():
    rho = np.arange(20, dtype=np.float64)
    return np.sin(np.pi * rho / 20.0).astype(F32), np.sin(2.0 * np.pi * rho / 20.0).astype(F32)


def with_parity(ch):
    """7 bits and odd parity in bit 7"""
    ch &= 0x7F
    return ch | (0x80 if bin(ch).count("1") % 2 == 0 else 0)


def crc_kermit(data):
    """CRC-16/KERMIT, one bit at a time: the register shifts right, the data enter least significant bit first"""
    crc = 0
    for byte in data:
        for i in range(8):
            fb = (crc ^ (byte >> i)) & 1
            crc >>= 1
            if fb:
                crc ^= 0x8408
    return crc


def crc_other_order(data):
    """the same polynomial with the other bit order (CRC-16/XMODEM): what the stage's checksum must not be"""
    crc = 0
    for byte in data:
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021 if crc & 0x8000 else crc << 1) & 0xFFFF
    return crc


SYNC_CHARS = [with_parity(ord("+")), with_parity(ord("*")), SYN, SYN, SOH]
assert SYNC_CHARS == [0xAB, 0x2A, 0x16, 0x16, 0x01]


def bits_of(data):
    return [(b >> i) & 1 for b in data for i in range(8)]


def sync_pattern():
    """the 39 changes inside the 40 sync bits, oldest first"""
    b = bits_of(SYNC_CHARS)
    return np.array([b[i] ^ b[i - 1] for i in range(1, 40)], np.uint8)


# ---------------- the bit bank ----------------

def _bank_tables():
    tau = np.arange(NTAU)[:, None]
    j = np.arange(NBITS)[None, :]
    t0 = tau + 20 * (j - (tau > 0))
    n0 = -((-t0) // 3)  # ceil
    rho0 = 3 * n0 - t0
    i = np.arange(7)
    idx = LEAD + n0[..., None] + i
    rho = rho0[..., None] + 3 * i
    seven = rho0 <= 1
    assert idx.min() == 2 and idx[..., :6].max() == LEAD + WAVE_BATCH - 1 and idx[seven].max() == LEAD + WAVE_BATCH - 1 and rho[seven].max() == 19
    idx[..., 6] = np.where(seven, idx[..., 6], 0)  # (a bit of six samples: the seventh product is not taken)
    rho[..., 6] = np.where(seven, rho[..., 6], 0)
    return idx, rho, seven


_IDX, _RHO, _SEVEN = _bank_tables()


def bank(staged):
    """staged float32 [..., 2008] (the lead's 8, then the block) -> (change bits uint8 [..., 20, 300], Q float32 [..., 20])"""
    h1, h2 = templates()
    x = staged[..., _IDX]  # [..., 20, 300, 7]
    r = []
    for h in (h1, h2):
        p = x * h[_RHO]
        s = p[..., 0]
        for i in range(1, 6):
            s = s + p[..., i]
        r.append(np.where(_SEVEN, s + p[..., 6], s))
    r1, r2 = r
    c = (np.abs(r1) >= np.abs(r2)).astype(np.uint8)
    q = np.maximum(r1 * r1, r2 * r2)
    s = q[..., 0:64].copy()
    for p in range(1, 4):
        s = s + q[..., 64 * p:64 * p + 64]
    s[..., :44] = s[..., :44] + q[..., 256:300]
    for h in (32, 16, 8, 4, 2, 1):
        s = s[..., :h] + s[..., h:2 * h]
    return c, s[..., 0]


def pack(c):
    """change bits [..., 300] -> words uint32 [..., 10]"""
    pad = np.zeros(c.shape[:-1] + (NWORDS * 32,), np.uint64)
    pad[..., :NBITS] = c
    return (pad.reshape(c.shape[:-1] + (NWORDS, 32)) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


# ---------------- the walker ----------------

class Walker:
    def __init__(self, st):
        self.phase = int(st["phase"])
        for n in WALKER:
            setattr(self, n, int(st[n]))
        self.bytes = [int(b) for b in st["bytes"]]

    def idle(self):
        self.phase = IDLE
        for n in WALKER:
            setattr(self, n, 0)
        self.bytes = [0] * RAW

    def open(self, u, mismatches, batch, j):
        self.idle()
        self.phase, self.u, self.tau_sync, self.mismatches = FRAME, u, u, mismatches
        t = u + 20 * (j + 1 - (u > 0))
        self.start_batch, self.start_third = ((batch + 1) & 0xFFFFFFFF, t - THIRDS) if t >= THIRDS else (batch, t)

    def step(self, c):
        """one change bit: None, "done" (the frame is whole) or "dropped" """
        self.prev ^= c
        self.cur |= self.prev << self.nbits
        self.nbits += 1
        if self.nbits < 8:
            return None
        byte, self.cur, self.nbits = self.cur, 0, 0
        self.crc = crc_kermit_step(self.crc, byte)
        if self.tail:
            self.bytes[self.nbytes + self.tail - 1] = byte
            self.tail += 1
            return "done" if self.tail == 3 else None
        self.bytes[self.nbytes] = byte
        self.nbytes += 1
        if bin(byte).count("1") % 2 == 0:
            self.parity_errors += 1
        if self.nbytes > HEAD and byte & 0x7F in (ETX, ETB):
            self.end, self.tail = byte & 0x7F, 1
        elif self.nbytes == MAX_BYTES:
            self.idle()
            return "dropped"
        return None

    def record(self, row, end_batch):
        f = np.zeros((), FRAME_REC)
        f["row"], f["batch"], f["third"], f["tau_sync"], f["tau_end"] = row, self.start_batch, self.start_third, self.tau_sync, self.u
        f["sync_errors"], f["crc_ok"], f["nbytes"], f["parity_errors"], f["end"], f["end_batch"] = self.mismatches, self.crc == 0, self.nbytes, self.parity_errors, self.end, end_batch
        f["bytes"] = self.bytes
        return f

    def store(self, st):
        st["phase"] = self.phase
        for n in WALKER:
            st[n] = getattr(self, n)
        st["bytes"] = self.bytes


def crc_kermit_step(crc, byte):
    for i in range(8):
        fb = (crc ^ (byte >> i)) & 1
        crc >>= 1
        if fb:
            crc ^= 0x8408
    return crc


def acars_model(plane, state=None, en=None, sync_errors=2, keep_bad=False, min_quality=0.0, hold_timing=False):
    """One call over plane float32 [rows][nb * 2000] from `state` (None: fresh): (frames, bits uint32 [rows][nb][20][10],
    q float32 [rows][nb][20], row_first [rows + 1], state after).  A disabled row's bits and q are zeros."""
    plane = np.ascontiguousarray(plane, F32)
    rows, nb = plane.shape[0], plane.shape[1] // WAVE_BATCH
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1).view(STATE).copy()
    en = np.ones(rows, bool) if en is None else np.asarray(en, bool)
    pat = sync_pattern()
    frames, row_first = [], np.zeros(rows + 1, np.uint32)
    bits_out, q_out = np.zeros((rows, nb, NTAU, NWORDS), np.uint32), np.zeros((rows, nb, NTAU), F32)
    min_quality = F32(min_quality)
    for r in range(rows):
        row_first[r] = len(frames)
        if not en[r]:
            continue
        st = state[r]
        seq = np.concatenate([np.zeros(2, F32), st["x"], plane[r, :nb * WAVE_BATCH]])
        staged = np.stack([seq[b * WAVE_BATCH:b * WAVE_BATCH + LEAD + WAVE_BATCH] for b in range(nb)])
        c, Q = bank(staged)  # [nb, 20, 300], [nb, 20]
        bits_out[r], q_out[r] = pack(c), Q
        hist = np.array([[(int(h) >> (37 - i)) & 1 for i in range(38)] for h in st["hist"]], np.uint8)  # oldest first
        w = Walker(st)
        batch0 = int(st["batch"])

        def event(ev, b):
            if ev == "done":
                if w.crc == 0 or keep_bad:
                    frames.append(w.record(r, b))
                w.idle()

        for b in range(nb):
            stream = np.concatenate([hist, c[b]], axis=1)  # [20, 338]
            mism = (np.lib.stride_tricks.sliding_window_view(stream, SYNC_BITS, axis=1) != pat).sum(-1)  # [20, 300]: the window that ends in slot j
            hit = (mism <= sync_errors) & (Q[b] >= min_quality)[:, None]
            anyhit = hit.any(0)
            skip = False
            if w.phase == FRAME and not hold_timing:
                u = w.u
                v = u
                if Q[b][(u - 1) % 20] > Q[b][v]:
                    v = (u - 1) % 20
                if Q[b][(u + 1) % 20] > Q[b][v]:
                    v = (u + 1) % 20
                w.u = v
                skip = (u, v) == (0, 1)
                if (u, v) == (1, 0):
                    event(w.step(int(hist[0, -1])), b)
            for j in range(NBITS):
                if w.phase == FRAME:
                    if skip:
                        skip = False
                    else:
                        event(w.step(int(c[b, w.u, j])), b)
                elif anyhit[j]:
                    cands = [t for t in range(NTAU) if hit[t, j]]
                    u = min(cands, key=lambda t: (int(mism[t, j]), -float(Q[b][t]), t))
                    w.open(u, int(mism[u, j]), (batch0 + b) & 0xFFFFFFFF, j)
            hist = stream[:, -38:]
        st["batch"] = (batch0 + nb) & 0xFFFFFFFF
        st["hist"] = [int("".join(map(str, h)), 2) for h in hist]
        w.store(st)
        st["x"] = plane[r, nb * WAVE_BATCH - HISTORY:nb * WAVE_BATCH]
    row_first[rows] = len(frames)
    return (np.array(frames, FRAME_REC) if frames else np.zeros(0, FRAME_REC)), bits_out, q_out, row_first, state


def run_in_calls(plane, cuts, state=None, masks=None, **kw):
    """the model over consecutive calls of the lengths `cuts`: [(frames, bits, q, row_first, state after)] per call"""
    out, done = [], 0
    for i, n in enumerate(cuts):
        res = acars_model(plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], state, None if masks is None else masks[i], **kw)
        out.append(res)
        state, done = res[4], done + n
    return out


def frame_fields(f):
    """a record's printable fields, parity stripped"""
    b = [int(x) & 0x7F for x in f["bytes"][:int(f["nbytes"])]]
    txt = lambda v: "".join(chr(x) if 0x20 <= x <= 0x7E else "." for x in v)  # noqa: E731
    return dict(mode=txt(b[0:1]), address=txt(b[1:8]), ack=txt(b[8:9]), label=txt(b[9:11]), block_id=txt(b[11:12]), text=txt(b[12:-1]), end=b[-1])


# ---------------- the modulator ----------------

def frame_bytes(mode="2", address=".N123AB", ack="\x15", label="H1", block_id="3", text="", end=ETX, parity_slip=None):
    """Mode .. ETX / ETB with parity, then the BCS low byte first.  parity_slip: index of a byte sent with the wrong parity, the BCS
    made over what is sent."""
    assert len(address) == 7 and len(label) == 2
    body = [with_parity(ord(ch)) for ch in mode + address + ack + label + block_id + text] + [with_parity(end)]
    if parity_slip is not None:
        body[parity_slip] ^= 0x80
    crc = crc_kermit(body)
    return body + [crc & 0xFF, crc >> 8]


def burst_bits(frames, prekey=64, between=0):
    """the bit values of a burst: pre-key of ones (no change: 2400 Hz), then per frame the sync characters and the frame's bytes;
    `between` ones between frames"""
    bits = [1] * prekey
    for k, f in enumerate(frames):
        if k:
            bits += [1] * between
        bits += bits_of(SYNC_CHARS + list(f))
    return bits


def modulate(bits, start_third, n, amp=0.3, ppm=0.0, first_prev=1):
    """float64 [n]: continuous-phase MSK of the bit values from third `start_third` of the row's first sample on (any real number), the
    bit clock fast by ppm.  A bit that differs from the one before is half a cycle of 1200 Hz, one that repeats it a full cycle of
    2400 Hz; the phase at each bit's start is accumulated in float64.  Silence before and behind."""
    bits = np.asarray(bits, np.int64)
    change = bits ^ np.concatenate([[first_prev], bits[:-1]])
    adv = np.where(change == 1, np.pi, 2.0 * np.pi)
    phase0 = np.concatenate([[0.0], np.cumsum(adv)[:-1]])
    blen = 20.0 / (1.0 + ppm * 1e-6)  # thirds a bit
    t = 3.0 * np.arange(n, dtype=np.float64) - start_third
    k = np.floor(t / blen).astype(np.int64)
    on = (k >= 0) & (k < len(bits))
    kk = np.clip(k, 0, len(bits) - 1)
    frac = t / blen - kk
    return np.where(on, amp * np.sin(phase0[kk] + adv[kk] * frac), 0.0)


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


# tools/acars_classes.py: MIN_SNR_DB is the lowest level (tone power over full-band white noise) at which 20 of 20
# frames decode; the sweep is not monotonic (19 of 20 from 11 to 19 dB: bursts that begin 1 .. 3 thirds behind a slot open early), so
# it is no level of reliable decoding.  The builder sits 3 dB above it.  TRACK_LIMIT_PPM is the offset up to which the longest frame
# decodes at every start time tried; the early-sync case sets it, not the tracker (drift_rows below follows 150 ppm).  The builder
# uses half.
MIN_SNR_DB = 10.0
NOISE_SNR_DB = MIN_SNR_DB + 3.0
TRACK_LIMIT_PPM = 20.0
LONG_TEXT = "".join(chr(0x20 + (7 * i) % 95) for i in range(MAX_BYTES - HEAD - 1))  # 227 characters: 240 bytes with ETX
TAIL_BATCHES = 4  # what the builder "cut by the end of the plane" goes on for behind NB


def random_text(rng, n):
    return "".join(chr(c) for c in rng.integers(0x20, 0x7F, n))


def builders():
    """[(name, row float64 [(NB + TAIL_BATCHES) * 2000], the frames sent as (fields, crc_ok) in order -- the ones a default handle must
    find within the first NB batches --, kept: the ones only keep_bad finds)]"""
    n = (NB + TAIL_BATCHES) * WAVE_BATCH
    out = []

    def sent(text="", **kw):
        f = dict(mode="2", address=".N123AB", ack="\x15", label="H1", block_id="3", text=text, end=ETX)
        f.update(kw)
        return f

    def fields(f):
        return {k: "".join(ch if 0x20 <= ord(ch) <= 0x7E else "." for ch in v) if isinstance(v, str) else v for k, v in f.items()}

    def add(name, x, found=(), kept=()):
        out.append((name, x, [fields(f) for f in found], [fields(f) for f in kept]))

    def one(f, start, **kw):
        return modulate(burst_bits([frame_bytes(**f)]), start, n, **kw)

    rng = np.random.default_rng(100)
    f0 = sent(random_text(rng, 20))
    base = 3 * 700
    add("a clean frame", one(f0, base), [f0])
    add("the same inverted", -one(f0, base), [f0])
    for s in range(0, 23):
        f = sent(random_text(rng, 8), block_id=chr(0x41 + s))
        add(f"start at third {s}", one(f, base + s), [f])
    add("start between thirds", one(f0, base + 7.5), [f0])
    # the first bit behind SOH is slot 298 of batch 2: 64 pre-key bits and 40 of sync in front of it
    f = sent(random_text(rng, 12))
    add("a frame that starts in the last bits of a batch", one(f, 3 * THIRDS - 40 - 20 * 104), [f])
    add("SOH across the boundary of batch 4 and 5", one(f, 5 * THIRDS - 20 * (64 + 36)), [f])
    flong = sent(LONG_TEXT)
    add("the longest frame", one(flong, base + 3), [flong])
    fe = sent("")
    add("an empty text", one(fe, base + 11), [fe])
    fb = sent(random_text(rng, 30), end=ETB)
    add("ETB", one(fb, base + 5), [fb])
    f1, f2 = sent(random_text(rng, 15), block_id="1"), sent(random_text(rng, 25), block_id="2")
    add("two frames back to back", modulate(burst_bits([frame_bytes(**f1), frame_bytes(**f2)]), base + 2, n), [f1, f2])
    fs = sent("AB+*\x16\x16\x01" + random_text(rng, 20))
    add("a sync inside the text", one(fs, base + 9), [fs])
    bits = burst_bits([frame_bytes(**f0)])
    bits[64 + 40 + 8 * 15 + 2] ^= 1
    add("one flipped bit in the text", modulate(bits, base + 4, n), [], [f0])
    add("a parity error under a matching BCS", modulate(burst_bits([frame_bytes(**f0, parity_slip=14)]), base + 6, n), [f0])
    body = [with_parity(ord(ch)) for ch in "2.N123AB\x15H13" + random_text(rng, 260)]
    add("no ETX in 240 bytes", modulate(burst_bits([body]), base + 8, n))
    fc = sent(random_text(rng, 200))
    add("cut by the end of the plane", one(fc, (NB - 3) * THIRDS + 13), [])
    add("a fast clock at half the tracking limit", one(flong, base + 1, ppm=TRACK_LIMIT_PPM / 2), [flong])
    add("a slow clock at half the tracking limit", one(flong, base + 1, ppm=-TRACK_LIMIT_PPM / 2), [flong])
    add("a DC offset", one(f0, base + 10) + 0.2, [f0])
    add("amplitude 1e-3", one(f0, base + 12, amp=1e-3), [f0])
    add("amplitude 1.0", one(f0, base + 14, amp=1.0), [f0])
    sigma = math.sqrt(0.3 ** 2 / 2 / 10 ** (NOISE_SNR_DB / 10))
    add("a frame in noise", one(f0, base + 16) + noise(n, sigma, 101), [f0])
    add("white noise", noise(n, 0.2, 102))
    add("voice-like", voice_like(n, 103))
    add("a steady 2400 Hz tone", 0.3 * np.sin(2 * np.pi * 2400.0 * np.arange(n) / RATE + 0.4))
    add("silence", np.zeros(n))
    add("-0.0 throughout", np.full(n, -0.0))
    add("subnormal values", np.random.default_rng(104).choice([1e-40, -3e-41, 1e-45, 0.0, 2e-39], n))
    return out


CUT_ROW = "cut by the end of the plane"


def stacked():
    """(names, plane float32 [rows][NB * 2000], the tail float32 [rows][TAIL_BATCHES * 2000], found per row, kept per row)"""
    b = builders()
    full = np.stack([x[1] for x in b]).astype(F32)
    return [x[0] for x in b], np.ascontiguousarray(full[:, :NB * WAVE_BATCH]), np.ascontiguousarray(full[:, NB * WAVE_BATCH:]), [x[2] for x in b], [x[3] for x in b]


# ---------------- end to end: a frame on an AM carrier, as u8 I/Q ----------------
E2E_BATCHES = 14
E2E_FRAME = dict(mode="2", address=".D-ABCD", ack="\x15", label="Q0", block_id="7", text="END TO END", end=ETX)


def e2e_setup(pkg):
    """One stream, one AM channel five bins above the centre at fft 512, 2.56 Msps.  The carrier is up from the start and the burst
    begins half a second later, when the AGC has settled: (dev, chans, iq uint8, batches)."""
    from common import AGC_EXTRA
    rate, centre = 2560000, 120000000
    dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=9)
    chans = [pkg.channel_cfg(centre + 25000, modulation=pkg.MOD_AM)]
    hop = rate // RATE
    n_audio = E2E_BATCHES * WAVE_BATCH + AGC_EXTRA + 8
    audio = modulate(burst_bits([frame_bytes(**E2E_FRAME)], prekey=128), 3 * 8000 + 5, n_audio, amp=0.5)
    n = n_audio * hop
    rng = np.random.default_rng(71)
    env = np.repeat(1.0 + audio, hop).astype(np.float32)
    ph = (2.0 * np.pi * 25000.0 / rate) * (np.arange(n) % (rate // 5000))  # (the offset's period is 512 samples: no phase grows large)
    z = 30.0 * env * np.exp(1j * ph).astype(np.complex64)
    iq = np.empty(2 * n, np.float32)
    iq[0::2], iq[1::2] = z.real, z.imag
    iq += rng.normal(0.0, 1.5, 2 * n).astype(np.float32)
    return dev, chans, np.clip(np.rint(iq + 127.5), 0, 255).astype(np.uint8), E2E_BATCHES


# ---------------- the timing moves, one by one: a frame continued from a seeded blob over a plane with one impulse ----------------
# One sample x at n in an otherwise silent batch gives Q[tau] = x^2 max(h1[rho]^2, h2[rho]^2) with rho = (3 n - tau) mod 20, exactly
# (every other term is +0).  rho = 10 under a hypothesis makes it the largest, so an impulse at rho = 9 under u favours u - 1, at
# rho = 11 u + 1; at rho = 0 Q[u] is 0 and Q[u - 1] == Q[u + 1] bit for bit (|h2[1]| == |h2[19]|): the neighbours' tie.
TRACK_FRAME = dict(mode="2", address=".TRACK1", ack="\x15", label="5Z", block_id="9", text="TRK", end=ETX)
#             (name, u, rho under u or None for silence, whole bytes taken, bits of the next, u after, bits taken in the batch, frames)
TRACK_CASES = [("u -> u - 1", 10, 9, 5, 3, 9, 300, 0), ("u -> u + 1", 10, 11, 5, 3, 11, 300, 0), ("0 -> 19", 0, 9, 5, 3, 19, 300, 0),
               ("19 -> 0", 19, 11, 5, 3, 0, 300, 0), ("0 -> 1 passes over a slot", 0, 11, 5, 3, 1, 299, 0),
               ("1 -> 0 retakes a bit", 1, 9, 5, 3, 0, 301, 0), ("1 -> 0, the bit retaken ends a byte", 1, 9, 5, 7, 0, 301, 0),
               ("1 -> 0, the bit retaken ends the frame", 1, 9, 17, 7, 0, 1, 1), ("the neighbours tie above u", 10, 0, 5, 3, 9, 300, 0),
               ("all tie in silence", 10, None, 5, 3, 10, 300, 0), ("2 -> 1", 2, 9, 5, 3, 1, 300, 0), ("1 -> 2", 1, 11, 5, 3, 2, 300, 0)]


def tracker_cases():
    """(names, state blob [rows], plane float32 [rows][2000], cases): every row inside TRACK_FRAME with `bytes taken` whole bytes and
    `bits` of the next one read, on hypothesis u, hypothesis 0's newest carried bit being the frame's next change bit"""
    fb = frame_bytes(**TRACK_FRAME)
    assert len(fb) == 18
    bits = bits_of(fb)
    st = fresh_state(len(TRACK_CASES))
    plane = np.zeros((len(TRACK_CASES), WAVE_BATCH), F32)
    for r, (_, u, rho, done, nbits, _, _, _) in enumerate(TRACK_CASES):
        body = len(fb) - 2
        taken = 8 * done + nbits
        s = st[r]
        s["batch"], s["phase"], s["u"], s["tau_sync"], s["prev"], s["nbits"] = 7, FRAME, u, u, bits[taken - 1], nbits
        s["cur"] = sum(bits[8 * done + i] << i for i in range(nbits))
        s["nbytes"], s["tail"] = min(done, body), max(0, done - body + 1) if done >= body else 0
        s["end"] = ETX if done >= body else 0
        s["crc"], s["start_batch"], s["start_third"] = crc_kermit(fb[:done]), 6, 4321
        s["bytes"][:done] = fb[:done]
        s["hist"][:] = 0x2AAAAAAAAA  # (far from the sync pattern)
        s["hist"][0] = 0x2AAAAAAAAA & ~1 | (bits[taken] ^ bits[taken - 1])
        if rho is not None:
            plane[r, (7 * (u + rho)) % 20 + 1000] = 0.5
    return [c[0] for c in TRACK_CASES], st, plane, TRACK_CASES


# ---------------- the timing moves on a drifting burst ----------------
DRIFT_BATCHES = 8
#        (name, clock offset in ppm, start in thirds, u at the end of each of the 8 batches, -1 = idle)
DRIFTS = [("a clock 150 ppm fast from third 5", 150.0, 2105, [5, 4, 3, 2, 1, 0, 19, -1]),
          ("a clock 150 ppm slow from third 16", -150.0, 2116, [16, 17, 18, 19, 0, 1, 2, -1])]


def drift_rows():
    """The longest frame at a clock offset of 0.9 third a batch, near what a move a batch can follow (167 ppm), from start times the
    first-slot rule opens on the right hypothesis: the walker follows down through 1 -> 0 and 0 -> 19, and up through 19 -> 0 and
    0 -> 1.  plane float32 [2][8 * 2000]"""
    f = dict(mode="2", address=".N123AB", ack="\x15", label="H1", block_id="3", text=LONG_TEXT, end=ETX)
    bits = burst_bits([frame_bytes(**f)])
    return np.stack([modulate(bits, start, DRIFT_BATCHES * WAVE_BATCH, ppm=ppm) for _, ppm, start, _ in DRIFTS]).astype(F32)
