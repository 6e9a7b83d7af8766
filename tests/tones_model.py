"""The yardstick of the tone-finder tests: the definition of include/mi_airband.h "CTCSS tone finder" in numpy and plain Python.  It
does not call into the library.

  ToneDetector::ToneDetector   src/ctcss.cpp:31-42    k = (int)(0.5 + W * f / rate), omega = (float)(2 pi k / W), coeff = (float)(2 cos(omega))
  process_sample               src/ctcss.cpp:44-49    q0 = coeff * q1 - q2 + x; q2 = q1; q1 = q0
  relative_power               src/ctcss.cpp:51-55    q1 * q1 + q2 * q2 - q1 * q2 * coeff
  CTCSS::reset                 src/ctcss.cpp:165-172  on the way to CLOSED (squelch.cpp:287): here at every NO_SIGNAL batch

Every operation is a numpy float32 operation of its own, so it rounds on its own.  The walk goes over a row's batches in plain Python
and cuts the call into the windows' sample ranges; the recurrence then runs over all ranges at once, vectorised over ranges and the
51 tones and sequential over samples.  cos() of a float is the C library's cosf, as it is for the reference.
"""
import ctypes
import ctypes.util

import numpy as np

from tx_model import NO_SIGNAL, SYMBOLS, WAVE_BATCH, draw_flags  # noqa: F401  (draw_flags: re-exported for the tests)

WAVE_RATE = 16000
NTONES, LANES = 51, 64
DEFAULT_WINDOW = int(WAVE_RATE * 0.4)  # squelch.cpp:115
STANDARD_TONES = np.array([67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0,
                           127.3, 131.8, 136.5, 141.3, 146.2, 150.0, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5,
                           186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1], np.float32)
assert len(STANDARD_TONES) == NTONES
RECORD = np.dtype([("row", "<u4"), ("seq", "<u4"), ("end_batch", "<u4"), ("end_sample", "<u4"), ("best", "<u4"), ("second", "<u4"),
                   ("best_power", "<f4"), ("second_power", "<f4"), ("mean_power", "<f4"), ("zero", "<u4")])
STATE = np.dtype([("count", "<u4"), ("seq", "<u4"), ("q1", "<f4", (LANES,)), ("q2", "<f4", (LANES,))])
assert RECORD.itemsize == 40 and STATE.itemsize == 520

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.argtypes, _libm.cosf.restype = [ctypes.c_float], ctypes.c_float


def coeff_of(freq, window, rate=WAVE_RATE):
    """ToneDetector's coefficient, type by type: the product and the quotient are float, the rest double"""
    ratio = np.float32(np.float32(np.float32(window) * np.float32(freq)) / np.float32(rate))
    k = int(0.5 + float(ratio))
    omega = np.float32((2.0 * np.pi * k) / window)
    return np.float32(2.0 * float(_libm.cosf(float(omega))))


def coeffs(window):
    return np.array([coeff_of(f, window) for f in STANDARD_TONES], np.float32)


def alias_of(window):
    c = coeffs(window)
    return np.array([int(np.flatnonzero(c == c[t])[0]) for t in range(NTONES)], np.uint32)


def fresh_state(rows):
    return np.zeros(rows, STATE)


def run_bank(xs, q1, q2, coeff):
    """The recurrence over the sample ranges xs (a list of float32 arrays) from q1 / q2 [len(xs)][51], all ranges side by side and
    sample by sample.  Returns q1, q2 after each range's last sample."""
    n = len(xs)
    q1, q2 = np.array(q1, np.float32).reshape(n, NTONES), np.array(q2, np.float32).reshape(n, NTONES)
    if n == 0:
        return q1, q2
    lens = np.array([len(x) for x in xs])
    order = np.argsort(-lens, kind="stable")  # the longest first: the ranges still running at step i are the first `active[i]`
    longest = int(lens.max())
    xt = np.zeros((longest, n), np.float32)
    for pos, k in enumerate(order):
        xt[:lens[k], pos] = xs[k]
    a, b = q1[order], q2[order]
    active = n - np.searchsorted(np.sort(lens), np.arange(longest), side="right")
    c = np.broadcast_to(np.asarray(coeff, np.float32), (n, NTONES))
    t = np.empty((n, NTONES), np.float32)
    for i in range(longest):
        m = active[i]
        np.multiply(c[:m], a[:m], out=t[:m])
        np.subtract(t[:m], b[:m], out=t[:m])
        np.add(t[:m], xt[i, :m, None], out=t[:m])
        b[:m] = a[:m]
        a[:m] = t[:m]
    q1[order], q2[order] = a, b
    return q1, q2


def powers_of(q1, q2, coeff):
    c = np.asarray(coeff, np.float32)
    return (q1 * q1 + q2 * q2) - (q1 * q2) * c


def tones_model(axc, wave, state=None, enabled=None, window=DEFAULT_WINDOW):
    """axc uint8 [rows][nbatches]; wave float32 [rows][>= nbatches * WAVE_BATCH]; state: STATE array [rows] or None (fresh); enabled:
    truth value per row or None (all).  Returns (records RECORD [k], powers float32 [k][64], row_first_record [rows + 1], state after)."""
    axc = np.asarray(axc, np.uint8)
    wave = np.asarray(wave, np.float32)
    rows, nb = axc.shape
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(STATE).reshape(rows)
    enabled = np.ones(rows, bool) if enabled is None else np.asarray(enabled, bool)
    coeff = coeffs(window)
    zeros = np.zeros(NTONES, np.float32)
    ranges, q1s, q2s, what = [], [], [], []  # what: (row, seq, end_batch, end_sample) of a window, (row, count, seq) of what is left
    row_first, nrec = np.zeros(rows + 1, np.uint32), 0
    for r in range(rows):
        row_first[r] = nrec
        if not enabled[r]:
            continue
        count, seq = int(state[r]["count"]), int(state[r]["seq"])
        q1, q2 = state[r]["q1"][:NTONES].copy(), state[r]["q2"][:NTONES].copy()
        parts = []  # the running window's samples inside this call
        for b in range(nb):
            if axc[r, b] == NO_SIGNAL:
                count, q1, q2, parts = 0, zeros, zeros, []
                continue
            at = 0
            while at < WAVE_BATCH:
                n = min(window - count, WAVE_BATCH - at)
                parts.append(wave[r, b * WAVE_BATCH + at:b * WAVE_BATCH + at + n])
                count += n
                at += n
                if count == window:
                    ranges.append(np.concatenate(parts))
                    q1s.append(q1)
                    q2s.append(q2)
                    what.append((r, seq, b, at - 1))
                    nrec += 1
                    count, seq, q1, q2, parts = 0, seq + 1, zeros, zeros, []
        ranges.append(np.concatenate(parts) if parts else np.zeros(0, np.float32))
        q1s.append(q1)
        q2s.append(q2)
        what.append((r, count, seq))
    row_first[rows] = nrec
    q1, q2 = run_bank(ranges, q1s, q2s, coeff)
    records, powers = np.zeros(nrec, RECORD), np.zeros((nrec, LANES), np.float32)
    k = 0
    for i, w in enumerate(what):
        if len(w) == 3:
            r, count, seq = w
            state[r]["count"], state[r]["seq"] = count, seq
            state[r]["q1"][:NTONES], state[r]["q2"][:NTONES] = q1[i], q2[i]
            continue
        p = powers_of(q1[i], q2[i], coeff)
        total = np.float32(0.0)
        for t in range(NTONES):
            total = np.float32(total + p[t])
        best = int(np.argmax(p))  # (the first of equals)
        others = p.copy()
        others[best] = -np.inf
        second = int(np.argmax(others))
        records[k] = (w[0], w[1], w[2], w[3], best, second, p[best], p[second], np.float32(total / np.float32(51.0)), 0)
        powers[k, :NTONES] = p
        k += 1
    assert k == nrec
    return records, powers, row_first, state


def run_in_calls(axc, wave, cuts, window=DEFAULT_WINDOW, enabled=None, state=None, masks=None):
    """the model over consecutive calls of the lengths `cuts` (sum = axc's width), state carried.  masks: the enabled rows of each
    call, in place of one `enabled` for all of them.
    Returns ([(first batch, records, powers, row_first_record, state after)], state after the last)"""
    assert sum(cuts) == axc.shape[1] and (masks is None or len(masks) == len(cuts))
    done, calls = 0, []
    for i, n in enumerate(cuts):
        en = enabled if masks is None else masks[i]
        rec, pw, first, state = tones_model(axc[:, done:done + n], wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], state, en, window)
        calls.append((done, rec, pw, first, state))
        done += n
    return calls, state


# ---------------- the oracle's detector set, rebuilt from the bank's powers ----------------

def detector_set(target, window):
    """indices of the tones CTCSS::CTCSS gives a detector for target tone number `target` (ctcss.cpp:61-73, 105-122): the target, then
    the table's tones at least 5 Hz away, each unless an earlier detector has its coefficient"""
    c = coeffs(window)
    chosen = [target]
    for t in range(NTONES):
        if abs(np.float32(STANDARD_TONES[target] - STANDARD_TONES[t])) < 5:
            continue
        if not any(c[u] == c[t] for u in chosen):
            chosen.append(t)
    return chosen


def has_tone(p, chosen):
    """CTCSS::process_audio_sample's decision at a window's end (ctcss.cpp:137-158) from the powers p [51] of the full bank"""
    total = np.float32(0.0)
    for t in chosen:
        total = np.float32(total + p[t])
    avg = np.float32(total / np.float32(len(chosen)))
    target = p[chosen[0]]
    return bool(target == max(p[t] for t in chosen) and target > avg)


# ---------------- the vote ----------------

def vote(records, min_windows=2, min_share_permille=500):
    """(windows, votes, tone, freq_hz, share, found) for one row's records"""
    votes = [0] * NTONES
    for r in records:
        if r["best_power"] > r["mean_power"]:
            votes[int(r["best"])] += 1
    tone = max(range(NTONES), key=lambda t: (votes[t], -t))
    n, v = len(records), votes[tone]
    found = n >= min_windows and v * 1000 >= min_share_permille * n
    if v == 0:
        return n, 0, 0, 0.0, 0.0, int(found)
    return n, v, tone, float(STANDARD_TONES[tone]), v / n, int(found)


# ---------------- audio ----------------

def tone_audio(rng, n, freq, amp=0.1, sigma=0.05, phase=0.0):
    """a tone of `amp` plus seeded Gaussian noise of `sigma`, clipped to the demodulator's [-1, 1]"""
    t = np.arange(n, dtype=np.float64) / WAVE_RATE
    x = amp * np.sin(2.0 * np.pi * freq * t + phase) + (rng.normal(0.0, sigma, n) if sigma else 0.0)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def two_tone_audio(rng, n, f1, f2, a1=0.1, a2=0.07, sigma=0.02):
    return np.clip(tone_audio(rng, n, f1, a1, sigma).astype(np.float64) + tone_audio(rng, n, f2, a2, 0.0), -1.0, 1.0).astype(np.float32)


def silence(n):
    return np.zeros(n, np.float32)


def full_scale_audio(rng, n):
    """every sample +1 or -1: the largest input the demodulator can write"""
    return rng.choice(np.array([-1.0, 1.0], np.float32), n)


def draw_audio(rng, rows, floats):
    """one kind of audio per row in turn: a table tone in noise, two tones, noise alone, full scale, silence"""
    wave = np.zeros((rows, floats), np.float32)
    for r in range(rows):
        kind = r % 5
        if kind == 0:
            wave[r] = tone_audio(rng, floats, float(STANDARD_TONES[rng.integers(0, NTONES)]))
        elif kind == 1:
            f = rng.choice(NTONES, 2, replace=False)
            wave[r] = two_tone_audio(rng, floats, float(STANDARD_TONES[f[0]]), float(STANDARD_TONES[f[1]]))
        elif kind == 2:
            wave[r] = tone_audio(rng, floats, 100.0, amp=0.0)
        elif kind == 3:
            wave[r] = full_scale_audio(rng, floats)
    return wave


# ---------------- designed planes for calls longer than one 64-batch trip of the walk ----------------

LONG_PRELUDE = 3  # batches of the call before the long one, all signal: the long call begins in the carried state
LONG_ROWS = {name: r for r, name in enumerate("ABCDHEFGI")}  # (draw_audio's silent row, 4, is H: every designed row has audio)


def long_call_planes(nb, window, seed=0):
    """(axc [9][LONG_PRELUDE + nb], wave) for two calls (LONG_PRELUDE, nb) on one handle, one row per flag pattern (LONG_ROWS), batch
    numbers those of the long call:
      A  every batch signals                              E  NO_SIGNAL except batches 62..66 (clipped to nb)
      B  every batch is NO_SIGNAL                         F  batches 0..63 NO_SIGNAL, the rest signal (B where nb == 64)
      C  signal except batch 63                           G, H  draw_flags at p_open 0.85 and 0.5
      D  signal except batch 64 (A where nb == 64)        I  drawn flags; the row the long call disables (long_call_masks)"""
    assert nb >= 64
    rng = np.random.default_rng([seed, nb, window])
    rows = len(LONG_ROWS)
    long = np.full((rows, nb), SYMBOLS[0], np.uint8)
    long[LONG_ROWS["B"]] = NO_SIGNAL
    long[LONG_ROWS["C"], 63] = NO_SIGNAL
    if nb > 64:
        long[LONG_ROWS["D"], 64] = NO_SIGNAL
    long[LONG_ROWS["E"]] = NO_SIGNAL
    long[LONG_ROWS["E"], 62:min(nb, 67)] = SYMBOLS[0]
    long[LONG_ROWS["F"], :64] = NO_SIGNAL
    long[LONG_ROWS["G"]] = draw_flags(rng, 1, nb, 0.85)[0]
    long[LONG_ROWS["H"]] = draw_flags(rng, 1, nb, 0.5)[0]
    long[LONG_ROWS["I"]] = draw_flags(rng, 1, nb, 0.85)[0]
    axc = np.concatenate([np.full((rows, LONG_PRELUDE), SYMBOLS[0], np.uint8), long], axis=1)
    return axc, draw_audio(rng, rows, (LONG_PRELUDE + nb) * WAVE_BATCH)


def long_call_masks():
    """the enabled rows of the two calls: all of them, then all but I"""
    second = np.ones(len(LONG_ROWS), np.uint8)
    second[LONG_ROWS["I"]] = 0
    return [np.ones(len(LONG_ROWS), np.uint8), second]
