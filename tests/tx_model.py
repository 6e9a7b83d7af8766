"""The yardstick of the transmission-splitter tests: split_on_transmission restated in signal time, in plain Python, one row and one
batch at a time, plus the order of `energy` in numpy float64.  It does not call into the library.

  close_if_necessary   src/output.cpp:367-375   close when duration > max, or duration > min and idle > idle
  skip                 src/output.cpp:518-520   a silent batch behind a silent batch is not written (but the close check runs)
  output_file_ready    src/output.cpp:404-414   the check runs again, then a file is opened if none is; :454 both stamps = now
  after a write        src/output.cpp:560-561   active = (axcindicate != NO_SIGNAL); last write = now

Time is the row's batch clock: batch b is handled at t0 + b * WAVE_BATCH / WAVE_RATE.  The reference's constants 1.0 s, 0.5 s and
3600 s are 8, 4 and 28800 batches of 2000 samples at 16 kHz; every comparison is a strict `>` as in the reference.

The walk yields, per batch, the file number the batch is written to (0: not written) and the (batch, file) pairs of the closes.
Records are derived from those two afterwards, not while walking.
"""
import numpy as np

from gate_model import NO_SIGNAL, SYMBOLS, WAVE_BATCH, draw_flags

WAVE_RATE = 16000
DEFAULT_CFG = (1 * WAVE_RATE // WAVE_BATCH, WAVE_RATE // 2 // WAVE_BATCH, 3600 * WAVE_RATE // WAVE_BATCH)  # min, idle, max: 8, 4, 28800
SMALL_CFG = (3, 2, 10)
NONE = 0xFFFFFFFF
RECORD = np.dtype([("row", "<u4"), ("seq", "<u4"), ("first_block", "<u4"), ("nblocks", "<u4"), ("first_batch", "<u4"), ("close_batch", "<u4"),
                   ("flags", "<u4"), ("peak", "<f4"), ("energy", "<f8")])
STATE = np.dtype([("clock", "<u8"), ("opened", "<u8"), ("last_write", "<u8"), ("seq", "<u4"), ("open", "u1"), ("active", "u1"), ("zero", "<u2")])
assert RECORD.itemsize == 40 and STATE.itemsize == 32
GAPS = (1, 3, 4, 5, 6, 7, 8, 9, 12)
BURST_SHAPES = [(1, 1), (1, 130), (3, 64), (3, 65), (65, 3), (1025, 3)]  # rows x batches, as the gate's


def fresh_state(rows):
    return np.zeros(rows, STATE)


def walk_row(flags, st, cfg=DEFAULT_CFG):
    """One row over `flags` (uint8 [n]) from state `st` (a dict, updated in place).  Returns (file [n]: the file number each batch is
    written to, 0 = not written; closes: [(batch, file number)])."""
    lo, idle, hi = cfg
    file_of, closes = np.zeros(len(flags), np.int64), []

    def check(b):
        if st["open"]:
            d, i = st["clock"] - st["opened"], st["clock"] - st["last_write"]
            if d > hi or (d > lo and i > idle):
                st["open"] = False
                closes.append((b, st["seq"]))

    for b, f in enumerate(flags):
        signal = f != NO_SIGNAL
        if not signal and not st["active"]:
            check(b)
        else:
            check(b)
            if not st["open"]:
                st["seq"] += 1
                st["open"] = True
                st["opened"] = st["last_write"] = st["clock"]
            file_of[b] = st["seq"]
            st["active"] = bool(signal)
            st["last_write"] = st["clock"]
        st["clock"] += 1
    return file_of, closes


def block_energy(blocks):
    """sum of x * x of each block [k][WAVE_BATCH] in the defined order: 256 partial sums (float4 number t, then number 256 + t for
    t < 244, four elements each in sequence), then acc[t] += acc[t + d] for t < d, d = 128 .. 1.  float64 throughout."""
    q = np.asarray(blocks, np.float32).astype(np.float64).reshape(-1, WAVE_BATCH // 4, 4)
    q = q * q
    acc = np.zeros((q.shape[0], 256), np.float64)
    for e in range(4):
        acc += q[:, :256, e]
    for e in range(4):
        acc[:, :WAVE_BATCH // 4 - 256] += q[:, 256:, e]
    d = 128
    while d >= 1:
        acc[:, :d] += acc[:, d:2 * d]
        d //= 2
    return acc[:, 0].copy()


def tx_model(axc, state=None, enabled=None, wave=None, cfg=DEFAULT_CFG):
    """axc uint8 [rows][nbatches]; state: STATE array [rows] or None (fresh); enabled: truth value per row or None (all); wave:
    float32 [rows][>= nbatches * WAVE_BATCH] or None (peak = energy = 0).
    Returns (records RECORD [k], row_first_record [rows + 1], state after, file_of [rows][nbatches], closes [(row, batch, file)])."""
    axc = np.asarray(axc, np.uint8)
    rows, nb = axc.shape
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(STATE).reshape(rows)
    enabled = np.ones(rows, bool) if enabled is None else np.asarray(enabled, bool)
    records, row_first = [], np.zeros(rows + 1, np.uint32)
    file_of, all_closes = np.zeros((rows, nb), np.int64), []
    for r in range(rows):
        row_first[r] = len(records)
        if not enabled[r]:
            continue
        st = dict(clock=int(state[r]["clock"]), opened=int(state[r]["opened"]), last_write=int(state[r]["last_write"]), seq=int(state[r]["seq"]),
                  open=bool(state[r]["open"]), active=bool(state[r]["active"]))
        carried = st["seq"] if st["open"] else None
        file_of[r], closes = walk_row(axc[r], st, cfg)
        closed_at = {seq: b for b, seq in closes}
        assert len(closed_at) == len(closes), "a file closes once"
        written = np.flatnonzero(file_of[r])  # the row's travelling batches; a block's rank is its position here
        for seq in sorted(set(file_of[r][written]) | set(closed_at)):
            mine = np.flatnonzero(file_of[r][written] == seq)
            assert len(mine) == 0 or (np.diff(mine) == 1).all(), "a file's blocks are one slice"
            rec = np.zeros((), RECORD)
            rec["row"], rec["seq"] = r, seq
            rec["first_block"], rec["nblocks"] = (mine[0] if len(mine) else 0), len(mine)
            rec["first_batch"] = written[mine[0]] if len(mine) else NONE
            rec["close_batch"] = closed_at.get(seq, NONE)
            rec["flags"] = 1 if seq == carried else 0
            if wave is not None and len(mine):
                blocks = np.asarray(wave, np.float32)[r, :nb * WAVE_BATCH].reshape(nb, WAVE_BATCH)[written[mine]]
                rec["peak"] = np.abs(blocks).max()
                total = np.float64(0.0)
                for s in block_energy(blocks):
                    total = total + s
                rec["energy"] = total
            records.append(rec)
        all_closes += [(r, b, seq) for b, seq in closes]
        for k in ("clock", "opened", "last_write", "seq", "open", "active"):
            state[r][k] = st[k]
    row_first[rows] = len(records)
    return np.array(records, RECORD).reshape(-1), row_first, state, file_of, all_closes


def letters(file_of_row):
    """file numbers of one row as a string: '.' = not written, 'a' = file 1, 'b' = file 2, ..."""
    return "".join("." if f == 0 else chr(ord("a") + int(f) - 1) for f in file_of_row)


def flags_of(text):
    """'*' / ' ' string -> uint8 [1][n]"""
    return np.frombuffer(text.encode(), np.uint8).reshape(1, -1).copy()


# the six hand cases: (flags, cfg, file letters, batches at which a file closes)
HAND_CASES = [
    ("**" + " " * 12 + "*", DEFAULT_CFG, "aaa...........b", [9]),
    ("**" + " " * 5 + "**" + " " * 7, DEFAULT_CFG, "aaa....aaa......", [14]),
    ("**" + " " * 6 + "**" + " " * 6, DEFAULT_CFG, "aaa.....aaa.....", [15]),
    ("*" * 12 + " " * 3 + "*" * 3 + " " * 8, DEFAULT_CFG, "a" * 13 + ".." + "aaaa" + "." * 7, [23]),
    ("*" * 12 + " " * 6 + "*" * 3 + " " * 9, DEFAULT_CFG, "a" * 13 + "." * 5 + "bbbb" + "." * 8, [17, 27]),
    ("*" * 30, (DEFAULT_CFG[0], DEFAULT_CFG[1], 10), "a" * 11 + "b" * 11 + "c" * 8, [11, 22]),
]


def draw_bursts(rng, rows, nbatches):
    """axc [rows][nbatches]: transmissions of 1 .. 20 batches separated by gaps drawn from GAPS, so that idle > 4 and duration > 8
    are grazed from both sides; a row starts inside a gap of random length"""
    axc = np.full((rows, nbatches), NO_SIGNAL, np.uint8)
    for r in range(rows):
        b = int(rng.integers(0, 4))
        while b < nbatches:
            n = int(rng.integers(1, 21))
            axc[r, b:b + n] = SYMBOLS[rng.integers(0, 3, len(axc[r, b:b + n]))]
            b += n + int(rng.choice(GAPS))
    return axc


def draw_audio(rng, rows, floats):
    """audio as the demodulator bounds it: uniform in [-1, 1], with +-0, +-1 and a few subnormals planted in every row"""
    wave = rng.uniform(-1.0, 1.0, (rows, floats)).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 1e-40, -3e-42, 1.4e-45], np.float32)
    for r in range(rows):
        at = rng.choice(floats, size=min(floats, 3 * len(special)), replace=False)
        wave[r, at] = np.resize(special, len(at))
    return wave


FAMILIES = ["p0", "p05", "p50", "p100", "bursts"]


def draw_family(name, rng, rows, nbatches):
    if name == "bursts":
        return draw_bursts(rng, rows, nbatches)
    return draw_flags(rng, rows, nbatches, {"p0": 0.0, "p05": 0.05, "p50": 0.5, "p100": 1.0}[name])


def run_in_calls(axc, cuts, cfg=DEFAULT_CFG, wave=None, enabled=None):
    """the model over consecutive calls of the lengths `cuts` (sum = axc's width), state carried.
    Returns ([(first batch, records, row_first_record)], state after, file_of [rows][n], closes in uncut batch numbers)"""
    assert sum(cuts) == axc.shape[1]
    state, done, calls, files, closes = None, 0, [], [], []
    for n in cuts:
        w = None if wave is None else wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        rec, first, state, file_of, cl = tx_model(axc[:, done:done + n], state, enabled, w, cfg)
        calls.append((done, rec, first))
        files.append(file_of)
        closes += [(r, b + done, seq) for r, b, seq in cl]
        done += n
    return calls, state, np.concatenate(files, axis=1), sorted(closes)


def features(axc, cuts, cfg):
    """which of the things a case is there to provoke it does provoke (names -> bool), on the model alone"""
    calls, _, file_of, closes = run_in_calls(axc, cuts, cfg)
    got = dict(idle_close=False, appended=False, max_split=False, empty_record=False, across_calls=False)
    for r, b, seq in closes:
        first = np.flatnonzero(file_of[r] == seq)[0]  # (every file here was opened inside the run: its clock starts at 0)
        got["max_split" if b - first > cfg[2] else "idle_close"] = True
    for r in range(axc.shape[0]):
        for seq in set(file_of[r][file_of[r] > 0]):
            mine = np.flatnonzero(file_of[r] == seq)
            got["appended"] |= bool((np.diff(mine) > 1).any())  # unwritten batches inside one file: a later transmission joined it
    for _, rec, _ in calls:
        got["empty_record"] |= bool((rec["nblocks"] == 0).any())
        got["across_calls"] |= bool(((rec["flags"] & 1 == 1) & (rec["nblocks"] > 0)).any())
    return got
