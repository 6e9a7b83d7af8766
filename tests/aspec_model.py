"""The audio spectrum stage's definition (include/mi_airband.h "audio spectrum stage") restated in numpy, and the audio its tests run on.

The window comes from the formula (math.cos in float64 for i <= 999, mirrored); the multiply is one float32 array operation; the
spectra go through the oracle's ao_fft_forward at log2n 11, bound as survey_model.py binds it; P is three float32 array operations;
the reductions are plain Python loops over Python floats (exact images of the float32 values, added in float64) in the stated
order; the vote is float64 Python."""
import functools
import math

import numpy as np

import survey_model as sm

WAVE_BATCH, WAVE_RATE = 2000, 16000
FFT_LOG, FFT, BINS, LINE_HALF, THREADS = 11, 2048, 1024, 2, 256
HZ_PER_BIN = WAVE_RATE / FFT  # 7.8125
NONE = 0xFFFFFFFF
RECORD = np.dtype([("row", "<u4"), ("batch", "<u4"), ("peak_bin", "<u4"), ("peak_power", "<f4"), ("band_power", "<f8"), ("line_power", "<f8")])
assert RECORD.itemsize == 32
DEFAULT_LO_HZ, DEFAULT_HI_HZ = 60, 3800
DEFAULT_MIN_BLOCKS, DEFAULT_RATIO = 8, 16.0


def band(lo_hz=0, hi_hz=0):
    """(lo_bin, hi_bin), or None where the configuration is refused"""
    lo = ((lo_hz or DEFAULT_LO_HZ) * FFT + WAVE_RATE - 1) // WAVE_RATE
    hi = (hi_hz or DEFAULT_HI_HZ) * FFT // WAVE_RATE
    return (lo, hi) if 1 <= lo <= hi <= BINS - 1 else None


def window64():
    """the formula in float64 at every i, not mirrored"""
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * i / (WAVE_BATCH - 1)) for i in range(WAVE_BATCH)], np.float64)


@functools.lru_cache(maxsize=None)
def window():
    half = window64()[:WAVE_BATCH // 2].astype(np.float32)
    w = np.concatenate([half, half[::-1]])
    w.setflags(write=False)
    return w


def windowed(x):
    """x [k][2000] float32 -> u [k][2048] float32"""
    x = np.asarray(x, np.float32)
    u = np.zeros((len(x), FFT), np.float32)
    u[:, :WAVE_BATCH] = x * window()[None, :]
    return u


def spectra(u):
    """u [k][2048] float32 -> X [k][2048][2] float32 through the oracle's ao_fft_forward"""
    xin = np.zeros((len(u), FFT, 2), np.float32)
    xin[:, :, 0] = u
    out = np.empty_like(xin)
    lib, plan = sm._oracle(), sm.fft_plan(FFT_LOG)
    pp = sm.C.byref(plan)
    for i in range(len(u)):
        lib.ao_fft_forward(pp, xin[i].ctypes.data, out[i].ctypes.data)
    return out


def powers(x):
    """x [k][2000] float32 -> P [k][1024] float32"""
    z = spectra(windowed(x))[:, :BINS]
    re, im = z[..., 0], z[..., 1]
    rr = re * re
    ii = im * im
    p = rr + ii
    assert p.dtype == np.float32
    return p


def reduce_block(p, lo, hi):
    """(peak_bin, peak_power, band_power, line_power) of one P[1024]"""
    v = [float(x) for x in p]
    acc = [0.0] * THREADS
    for t in range(THREADS):
        for b in (t, t + 256, t + 512, t + 768):
            if lo <= b <= hi:
                acc[t] += v[b]
    d = THREADS // 2
    while d >= 1:
        for t in range(d):
            acc[t] += acc[t + d]
        d //= 2
    peak = lo
    for b in range(lo + 1, hi + 1):
        if v[b] > v[peak]:
            peak = b
    line = 0.0
    for b in range(max(lo, peak - LINE_HALF), min(hi, peak + LINE_HALF) + 1):
        line += v[b]
    return peak, p[peak], acc[0], line


def row_means(power, row_first, rows, stored):
    """(row_mean [rows][1024] float32, row_blocks [rows] uint32) from the stored power rows"""
    mean = np.zeros((rows, BINS), np.float32)
    blocks = np.zeros(rows, np.uint32)
    for r in range(rows):
        first, last = min(int(row_first[r]), stored), min(int(row_first[r + 1]), stored)
        n = max(last - first, 0)
        blocks[r] = n
        if n:
            s = np.zeros(BINS, np.float64)
            for k in range(first, first + n):
                s = s + power[k].astype(np.float64)
            mean[r] = (s / n).astype(np.float32)
    return mean, blocks


def aspec_model(wave, index, row_first=None, lo_hz=0, hi_hz=0, nbatches=None, stored=None):
    """One call: wave [rows][>= nbatches * 2000] float32, index [k][2] = (row, batch), of which the first `stored` (default all) are
    stored; row_first [rows + 1] or None.  Returns (records [stored] of RECORD, power [stored][1024], row_mean [rows][1024] or None,
    row_blocks [rows] or None)."""
    wave = np.asarray(wave, np.float32)
    rows = wave.shape[0]
    nb = wave.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    lo, hi = band(lo_hz, hi_hz)
    index = np.asarray(index, np.int64).reshape(-1, 2)
    stored = len(index) if stored is None else min(stored, len(index))
    index = index[:stored]
    ok = (index[:, 0] < rows) & (index[:, 1] < nb)
    x = np.zeros((stored, WAVE_BATCH), np.float32)
    for k, (row, batch) in enumerate(index):
        if ok[k]:
            x[k] = wave[row, batch * WAVE_BATCH:(batch + 1) * WAVE_BATCH]
    power = powers(x)
    power[~ok] = 0.0
    records = np.zeros(stored, RECORD)
    for k, (row, batch) in enumerate(index):
        records[k] = (row, batch, *reduce_block(power[k], lo, hi)) if ok[k] else (row, batch, NONE, 0.0, 0.0, 0.0)
    if row_first is None:
        return records, power, None, None
    mean, blocks = row_means(power, row_first, rows, stored)
    return records, power, mean, blocks


def notch_model(mean, row_blocks, records=(), lo_hz=0, hi_hz=0, min_blocks=0, ratio=0.0):
    """dict(found, bin, freq_hz, peak, floor, votes, blocks) from one row's mean spectrum"""
    lo, hi = band(lo_hz, hi_hz)
    mean = np.asarray(mean, np.float32)
    m = [float(x) for x in mean]
    p = lo
    for j in range(lo + 1, hi + 1):
        if m[j] > m[p]:
            p = j
    around = sorted(m[j] for j in range(lo, hi + 1) if 3 <= abs(j - p) <= 34)
    floor = around[(len(around) - 1) // 2] if around else 0.0
    threshold = float(np.float32(ratio or DEFAULT_RATIO) * np.float32(floor))
    num = den = 0.0
    for j in range(max(lo, p - 1), min(hi, p + 1) + 1):
        num += j * m[j]
        den += m[j]
    votes = sum(1 for r in records if abs(int(r["peak_bin"]) - p) <= 1)
    found = row_blocks >= (min_blocks or DEFAULT_MIN_BLOCKS) and m[p] > 0 and m[p] > threshold
    return dict(found=int(found), bin=p, freq_hz=HZ_PER_BIN * (num / den if den > 0 else p), peak=m[p], floor=floor, votes=votes, blocks=int(row_blocks))


# ---------------- indices ----------------

def full_index(rows, nb):
    """every (row, batch), rows ascending and batches ascending within a row, and its row_first: what MI_GATE_ALL packs"""
    idx = np.stack(np.meshgrid(np.arange(rows), np.arange(nb), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.uint32)
    return idx, (np.arange(rows + 1) * nb).astype(np.uint32)


def foreign_audio(group, rows, nbatches, max_batches):
    """the audio of the foreign-index cases (pcm_model.foreign_index): row r takes builder (rows * group + r) mod 13, so groups 0 .. 4
    of three rows go through all thirteen; laid out for max_batches with pcm_model.FOREIGN_FILL behind the call"""
    from pcm_model import foreign_wave
    names = list(BUILDERS)
    wave = np.stack([audio(names[(rows * group + r) % len(names)], 1, nbatches, group)[0] for r in range(rows)])
    return foreign_wave(wave, nbatches, max_batches)


FOREIGN_GROUPS = 5


@functools.lru_cache(maxsize=None)
def foreign_reference(case, group, lo_hz=0, hi_hz=0):
    """(wave, index, count, row_first, max_blocks, stored, the model's (records, power, mean, row counts)) of one foreign-index case,
    computed once for the tests that compare the twin and the device with it"""
    import pcm_model as pm
    rows, nb, mb = pm.FOREIGN_SHAPE
    index, count, row_first, cap, stored = pm.foreign_case(case, rows, nb, mb)
    wave = foreign_audio(group, rows, nb, mb)
    want = aspec_model(wave, index, row_first, lo_hz, hi_hz, nbatches=nb, stored=stored)
    for a in (wave, index, count, row_first) + want:
        a.setflags(write=False)
    return wave, index, count, row_first, cap, stored, want


# ---------------- audio ----------------

def _time(nb):
    return np.arange(nb * WAVE_BATCH, dtype=np.float64) / WAVE_RATE


def tone_rows(rows, nb, hz, amp=0.5, seed=0):
    """one steady sine per row, the same frequency in every row, a phase of its own"""
    rng = np.random.default_rng(6000 + seed)
    t = _time(nb)
    return np.stack([amp * np.sin(2 * np.pi * hz * t + rng.uniform(0, 2 * np.pi)) for _ in range(rows)]).astype(np.float32)


def silence(rows, nb, seed=0):
    """every P is 0: peak_bin == lo_bin"""
    return np.zeros((rows, nb * WAVE_BATCH), np.float32)


def constant(rows, nb, seed=0):
    """0.5 throughout: the energy lies below the band, what the band sees is the window's side lobes"""
    return np.full((rows, nb * WAVE_BATCH), np.float32(0.5))


def tone_on_bin(rows, nb, seed=0):
    """exactly on bin 128 = 1000 Hz"""
    return tone_rows(rows, nb, 128 * HZ_PER_BIN, seed=seed)


def tone_between(rows, nb, seed=0):
    """half way between bins 128 and 129"""
    return tone_rows(rows, nb, 128.5 * HZ_PER_BIN, seed=seed)


def tone_lo(rows, nb, seed=0):
    """on the default lo_bin 8: the line sum is clipped below"""
    return tone_rows(rows, nb, 8 * HZ_PER_BIN, seed=seed)


def tone_lo1(rows, nb, seed=0):
    """on lo_bin + 1: one bin of the line sum is clipped"""
    return tone_rows(rows, nb, 9 * HZ_PER_BIN, seed=seed)


def tone_hi(rows, nb, seed=0):
    """on the default hi_bin 486: the line sum is clipped above"""
    return tone_rows(rows, nb, 486 * HZ_PER_BIN, seed=seed)


OUTSIDE_BIN, INSIDE_BIN = 600, 200


def outside_strong(rows, nb, seed=0):
    """0.8 on bin 600, outside the default band, beside 0.01 on bin 200 inside it: the weak one is the band's peak"""
    return (tone_rows(rows, nb, OUTSIDE_BIN * HZ_PER_BIN, 0.8, seed) + tone_rows(rows, nb, INSIDE_BIN * HZ_PER_BIN, 0.01, seed + 1)).astype(np.float32)


SQUARE_HALF_PERIODS = (25, 50, 7, 400, 100)


def square(rows, nb, seed=0):
    """full-scale +-1 square waves, row r with half-period SQUARE_HALF_PERIODS[r % 5]"""
    n = np.arange(nb * WAVE_BATCH)
    return np.stack([np.where((n // SQUARE_HALF_PERIODS[r % 5]) % 2 == 0, 1.0, -1.0) for r in range(rows)]).astype(np.float32)


def subnormal(rows, nb, seed=0):
    """values of subnormal size of both signs: every product with the window is subnormal or zero, every P is 0"""
    rng = np.random.default_rng(2000 + seed)
    bits = rng.integers(1, 1 << 23, (rows, nb * WAVE_BATCH)).astype(np.uint32)
    bits |= rng.integers(0, 2, bits.shape).astype(np.uint32) << 31
    return bits.view(np.float32)


def noise(rows, nb, seed=0):
    return np.random.default_rng(3000 + seed).uniform(-1.0, 1.0, (rows, nb * WAVE_BATCH)).astype(np.float32)


WHISTLE_HZ = 1000.0


def voice(rows, nb, seed=0, whistle_db=None, whistle_hz=WHISTLE_HZ):
    """Voice-like: 24 harmonics of a pitch that glides between 80 and 160 Hz a few times a second, weighted by three formants, under a
    syllable envelope, peak 0.8.  Nothing in it stands still, so the long-term spectrum has no line.  whistle_db: a steady sine at
    whistle_hz whose power is that many dB relative to the voice's mean power (-20: a hundredth)."""
    rng = np.random.default_rng(5000 + seed)
    t = _time(nb)
    out = np.zeros((rows, len(t)))
    for r in range(rows):
        f0 = 120.0 + 40.0 * np.sin(2 * np.pi * rng.uniform(1.5, 4.0) * t + rng.uniform(0, 2 * np.pi))
        phase = 2 * np.pi * np.cumsum(f0) / WAVE_RATE
        formants = rng.uniform((400.0, 1200.0, 2200.0), (800.0, 1800.0, 3000.0))
        v = np.zeros(len(t))
        for h in range(1, 25):
            a = sum(1.0 / (1.0 + ((h * 120.0 - f) / 150.0) ** 2) for f in formants)
            v += a * np.sin(h * phase + rng.uniform(0, 2 * np.pi))
        v *= 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(2.0, 5.0) * t + rng.uniform(0, 2 * np.pi))
        v *= 0.8 / np.abs(v).max()
        if whistle_db is not None:
            amp = math.sqrt(2.0 * np.mean(v * v) * 10.0 ** (whistle_db / 10.0))
            v = v + amp * np.sin(2 * np.pi * whistle_hz * t + rng.uniform(0, 2 * np.pi))
        out[r] = v
    return out.astype(np.float32)


def voice_whistle(rows, nb, seed=0):
    """the voice-like signal with a steady whistle 20 dB below it at 1000 Hz"""
    return voice(rows, nb, seed, whistle_db=-20.0)


BUILDERS = {"silence": silence, "constant": constant, "tone_on_bin": tone_on_bin, "tone_between": tone_between, "tone_lo": tone_lo, "tone_lo1": tone_lo1,
            "tone_hi": tone_hi, "outside_strong": outside_strong, "square": square, "subnormal": subnormal, "noise": noise, "voice": voice,
            "voice_whistle": voice_whistle}


@functools.lru_cache(maxsize=None)
def audio(name, rows, nb, seed=0):
    if name == "mixed":  # row r from builder r mod 13, so that one call holds them all
        names = list(BUILDERS)
        a = np.stack([audio(names[r % len(names)], 1, nb, seed + r // len(names))[0] for r in range(rows)])
    else:
        a = BUILDERS[name](rows, nb, seed)
    assert a.dtype == np.float32 and a.shape == (rows, nb * WAVE_BATCH) and np.isfinite(a).all() and (np.abs(a) <= 1).all()
    a.setflags(write=False)
    return a
