"""The PCM stage's definition (include/mi_airband.h "PCM stage") restated in numpy, and the audio its tests run on.

The taps come from the formula in float64; the filter is 63 sequential float32 array operations over all outputs at once, each
product and each sum rounded on its own; the quantiser is np.rint; the IMA encoder is a plain integer loop over the 24 steps of a
sub-block, vectorised over sub-blocks.  The decoder is written from the format's description, not from the encoder."""
import functools

import numpy as np

WAVE_BATCH, WAVE_RATE = 2000, 16000
TAPS, HISTORY = 63, 62
S16, IMA4 = 1, 2
IMA_SAMPLES, IMA_BYTES = 25, 16
CONFIGS = [(8000, S16), (8000, IMA4), (16000, S16), (16000, IMA4)]
STATE = np.dtype([("x", "<f4", (HISTORY,))])
STEPS = np.array([7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
                  157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
                  1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442,
                  11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], np.int64)
INDEX_STEP = np.array([-1, -1, -1, -1, 2, 4, 6, 8], np.int64)
assert len(STEPS) == 89


def samples_per_block(rate):
    return {8000: WAVE_BATCH // 2, 16000: WAVE_BATCH}[rate]


def block_bytes(rate, fmt):
    s = samples_per_block(rate)
    return 2 * s if fmt == S16 else IMA_BYTES * s // IMA_SAMPLES


def design64():
    """g[k] / sum g in float64, the even offsets from the centre exactly zero"""
    k = np.arange(TAPS, dtype=np.float64)
    c = k - 31
    g = 0.5 * np.sinc(c / 2) * (0.42 - 0.5 * np.cos(2 * np.pi * k / 62) + 0.08 * np.cos(4 * np.pi * k / 62))  # np.sinc(t) = sin(pi t) / (pi t)
    g[(c % 2 == 0) & (c != 0)] = 0.0
    return g / g.sum()


@functools.lru_cache(maxsize=None)
def taps():
    h = design64().astype(np.float32)
    h.setflags(write=False)
    return h


def response_db(h, freqs_hz):
    """|H(f)| in dB of taps h (any dtype, evaluated in float64) at the input rate of 16000"""
    k = np.arange(len(h), dtype=np.float64)
    w = 2 * np.pi * np.asarray(freqs_hz, np.float64)[:, None] / WAVE_RATE
    return 20 * np.log10(np.abs((np.asarray(h, np.float64)[None, :] * np.exp(-1j * w * k[None, :])).sum(axis=1)))


def fir(x):
    """x [..., 62 + 2000] float32, the block behind the 62 samples before it -> y [..., 1000] float32"""
    h = taps()
    acc = np.zeros(x.shape[:-1] + (WAVE_BATCH // 2,), np.float32)
    for k in range(TAPS):
        acc = acc + h[k] * x[..., HISTORY - k:HISTORY - k + WAVE_BATCH:2]
    assert acc.dtype == np.float32
    return acc


def quantise(y):
    v = np.asarray(y, np.float32) * np.float32(32767.0)
    assert v.dtype == np.float32
    return np.rint(np.clip(v, np.float32(-32767.0), np.float32(32767.0))).astype(np.int16)


def ima_index0(s0, s1):
    d = np.abs(s1.astype(np.int64) - s0.astype(np.int64))
    below = (7 * STEPS[None, :] < 4 * d[:, None]).sum(axis=1)  # the table ascends: the smallest i with 7 T[i] >= 4 d
    return np.minimum(below, 88)


def ima_encode(s, trace=False):
    """s [n][25] int16 -> [n][16] uint8; with trace also the predictor after every sample [n][25], the index before every step [n][24]
    and whether the predictor was clamped [n][24]"""
    s = np.asarray(s, np.int16).astype(np.int64)
    n = len(s)
    out = np.zeros((n, IMA_BYTES), np.uint8)
    index = ima_index0(s[:, 0], s[:, 1])
    out[:, 0], out[:, 1], out[:, 2] = s[:, 0] & 0xFF, (s[:, 0] >> 8) & 0xFF, index
    p = s[:, 0].copy()
    preds, indices, clamps = [p.copy()], [], []
    for j in range(1, IMA_SAMPLES):
        indices.append(index.copy())
        step = STEPS[index]
        diff = s[:, j] - p
        sign = np.where(diff < 0, 8, 0)
        diff = np.abs(diff)
        vp = step >> 3
        code = np.zeros(n, np.int64)
        for bit in (4, 2, 1):
            hit = diff >= step
            code |= np.where(hit, bit, 0)
            if bit != 1:
                diff = np.where(hit, diff - step, diff)
            vp = np.where(hit, vp + step, vp)
            step = step >> 1
        raw = np.where(sign != 0, p - vp, p + vp)
        p = np.clip(raw, -32768, 32767)
        clamps.append(raw != p)
        index = np.clip(index + INDEX_STEP[code], 0, 88)
        nibble = (code | sign).astype(np.uint8)
        out[:, 4 + (j - 1) // 2] |= nibble if (j - 1) % 2 == 0 else nibble << 4
        preds.append(p.copy())
    if trace:
        return out, np.stack(preds, axis=1), np.stack(indices, axis=1), np.stack(clamps, axis=1)
    return out


def ima_decode(blocks):
    """[n][16] uint8 -> [n][25] int64 samples.  From the format's description (WAV format 0x0011, mono): a block begins with the first
    sample as int16 LE, the step index and a zero byte; every following nibble, low nibble first, adds to the predictor
    (step >> 3) + (step if bit 2) + (step >> 1 if bit 1) + (step >> 2 if bit 0), subtracts it if bit 3 is set, saturates at int16, and
    moves the index by -1 for 0 .. 3 and by 2, 4, 6, 8 for 4 .. 7 of the low three bits, kept within 0 .. 88."""
    blocks = np.asarray(blocks, np.uint8)
    assert blocks.ndim == 2 and blocks.shape[1] == IMA_BYTES
    first = (blocks[:, 0].astype(np.int64) | (blocks[:, 1].astype(np.int64) << 8))
    first = np.where(first >= 32768, first - 65536, first)
    idx = blocks[:, 2].astype(np.int64)
    assert (idx <= 88).all() and (blocks[:, 3] == 0).all()
    out = [first]
    cur = first.copy()
    for i in range(2 * (IMA_BYTES - 4)):
        byte = blocks[:, 4 + i // 2].astype(np.int64)
        nib = (byte >> 4) if i % 2 else (byte & 15)
        step = STEPS[idx]
        delta = step >> 3
        delta = delta + np.where(nib & 4, step, 0) + np.where(nib & 2, step >> 1, 0) + np.where(nib & 1, step >> 2, 0)
        cur = cur + np.where(nib & 8, -delta, delta)
        cur = np.minimum(np.maximum(cur, -32768), 32767)
        idx = idx + np.where((nib & 7) < 4, -1, 2 * ((nib & 7) - 3))
        idx = np.minimum(np.maximum(idx, 0), 88)
        out.append(cur.copy())
    return np.stack(out, axis=1)


def fresh_state(rows):
    return np.zeros(rows, STATE)


def block_samples(wave, index, state, rate, nbatches):
    """int16 samples [k][S] of the index's blocks, and which entries are of this call (the others' samples are zero)"""
    wave = np.asarray(wave, np.float32)
    index = np.asarray(index, np.int64).reshape(-1, 2)
    rows = wave.shape[0]
    ok = (index[:, 0] < rows) & (index[:, 1] < nbatches)
    x = np.zeros((len(index), HISTORY + WAVE_BATCH), np.float32)
    for k, (row, batch) in enumerate(index):
        if not ok[k]:
            continue
        x[k, HISTORY:] = wave[row, batch * WAVE_BATCH:(batch + 1) * WAVE_BATCH]
        x[k, :HISTORY] = wave[row, batch * WAVE_BATCH - HISTORY:batch * WAVE_BATCH] if batch else state["x"][row]
    return quantise(fir(x) if rate == 8000 else x[:, HISTORY:]), ok


def pcm_model(wave, index, state=None, enabled=None, rate=8000, fmt=S16, nbatches=None):
    """One call: wave [rows][>= nbatches * 2000] float32, index [k][2] = (row, batch), state [rows] of STATE or None (fresh), enabled
    [rows] or None (all).  Returns (blocks [k][block_bytes] uint8, the state after the call)."""
    wave = np.asarray(wave, np.float32)
    rows = wave.shape[0]
    nb = wave.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    state = fresh_state(rows) if state is None else np.array(state, copy=True).view(STATE).reshape(rows)
    enabled = np.ones(rows, bool) if enabled is None else np.asarray(enabled).astype(bool)
    s, ok = block_samples(wave, index, state, rate, nb)
    if fmt == S16:
        blocks = s.astype("<i2").view(np.uint8).reshape(len(s), block_bytes(rate, fmt))
    else:
        blocks = ima_encode(s.reshape(-1, IMA_SAMPLES)).reshape(len(s), block_bytes(rate, fmt))
    blocks = np.where(ok[:, None], blocks, np.uint8(0))
    assert blocks.shape == (len(s), block_bytes(rate, fmt))
    after = state.copy()
    after["x"][enabled] = wave[enabled, nb * WAVE_BATCH - HISTORY:nb * WAVE_BATCH]
    return np.ascontiguousarray(blocks), after


def run_in_calls(wave, cuts, indices, rate, fmt, masks=None, state=None):
    """consecutive calls of the lengths `cuts` over one long wave: [(blocks, state after)] per call; indices[i] is call-relative"""
    out, done = [], 0
    for i, n in enumerate(cuts):
        blocks, state = pcm_model(wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH], indices[i], state, None if masks is None else masks[i], rate, fmt)
        out.append((blocks, state))
        done += n
    return out


# ---------------- indices ----------------

def full_index(rows, nb):
    """every (row, batch), rows ascending and batches ascending within a row: what MI_GATE_ALL packs"""
    return np.stack(np.meshgrid(np.arange(rows), np.arange(nb), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.uint32)


def drawn_index(rows, nb, seed, keep=0.7):
    """the gate's order with some blocks left out, batch 0 and the last batch of row 0 always in"""
    rng = np.random.default_rng(seed)
    idx = full_index(rows, nb)
    take = rng.random(len(idx)) < keep
    take[0] = take[nb - 1] = True
    return idx[take]


FOREIGN = 0xFFFFFFFF
FOREIGN_SHAPE = (3, 2, 8)  # rows, nbatches of the call, max_batches of the handle: a grid of 6 under a capacity of 24
FOREIGN_FILL = np.float32(0.5)  # what the input holds behind the call's batches


def foreign_index(rows=3, nbatches=2, max_batches=8, entries=20):
    """An index no gate writes, for a call of `nbatches` on a handle of `max_batches`: (index [entries][2], count [2] = (entries,
    entries), row_first [rows + 1]).  The stages launch min(rows * nbatches, max_blocks) workgroups, and workgroup g takes the
    entries g, g + grid, g + 2 grid, ...; at rows 3, nbatches 2 (a grid of 6) the columns below are one workgroup's trips.  V is an
    entry of the call, the others are not: A has row == rows, B batch == nbatches, C 0xFFFFFFFF in both fields, D a batch in
    nbatches + 1 .. max_batches - 1, which the input is laid out for (foreign_wave) and the call is not.

        g      0        1        2        3        4        5
        k=g    V(2,1)   C        V(0,1)   V(1,0)   B(2,.)   V(2,0)
        +6     A(.,0)   B(0,.)   V(2,0)   D(0,+1)  V(2,1)   C
        +12    V(0,0)   V(1,0)   D(2,+5)  A(.,1)   V(1,1)   V(0,1)
        +18    D(1,+3)  V(1,1)   V(2,1)   B(1,.)   D(0,+2)  V(1,0)     (entries 20 .. 23 only where asked for)

    The first 13 entries alone (a capacity of 13) still hold every kind and every order of neighbours.  row_first is not a gate's:
    row 0 has its start behind its end, row 1's slice runs past what is stored, row 2's begins behind that.  It is laid out for
    `entries` stored blocks; foreign_row_first gives it for another number."""
    r, n, m = rows, nbatches, max_batches
    assert r >= 3 and n >= 2 and m >= n + 6 and 13 <= entries <= 24
    f = FOREIGN
    index = np.array([[2, 1], [f, f], [0, 1], [1, 0], [2, n], [2, 0],
                      [r, 0], [0, n], [2, 0], [0, n + 1], [2, 1], [f, f],
                      [0, 0], [1, 0], [2, n + 5], [r, 1], [1, 1], [0, 1],
                      [1, n + 3], [1, 1], [2, 1], [1, n], [0, n + 2], [1, 0]], np.uint32)[:entries]
    return index, np.array([entries, entries], np.uint32), foreign_row_first(rows, entries)


def foreign_row_first(rows, stored):
    """row 0: first > last, no block.  Row 1: 2 .. stored + 1, cut by `stored`.  Row 2: begins at stored + 1, behind it.  (The largest
    value is stored + 2: a walk that did not clip would still stay within two guard blocks behind the capacity.)"""
    return np.array([5, 2] + [stored + 1] * (rows - 2) + [stored + 2], np.uint32)


def foreign_kinds(index, rows, nbatches, max_batches):
    """per entry one of V (of the call), A (row == rows), B (batch == nbatches), C (0xFFFFFFFF twice), D (a batch of the handle behind
    the call); anything else is a mistake in the builder"""
    kinds = []
    for row, batch in np.asarray(index, np.int64).reshape(-1, 2):
        if row < rows and batch < nbatches:
            kinds.append("V")
        elif row == rows and batch < nbatches:
            kinds.append("A")
        elif row < rows and batch == nbatches:
            kinds.append("B")
        elif row == FOREIGN and batch == FOREIGN:
            kinds.append("C")
        else:
            assert row < rows and nbatches < batch < max_batches, (row, batch)
            kinds.append("D")
    return "".join(kinds)


def assert_foreign_properties(index, row_first, rows, nbatches, max_batches, stored, grid=None):
    """What foreign_index is built for, stated on the index alone: over the first `stored` entries, walked as a grid of `grid`
    workgroups walks them."""
    grid = min(rows * nbatches, stored) if grid is None else grid
    index = np.asarray(index, np.int64).reshape(-1, 2)[:stored]
    kinds = foreign_kinds(index, rows, nbatches, max_batches)
    trips = [kinds[g::grid] for g in range(grid)]  # entries k, k + grid, k + 2 grid, ... go to one workgroup
    assert stored > grid and all(len(t) >= 2 for t in trips), "every workgroup makes a second trip"
    assert max(len(t) for t in trips) >= 3
    zero = lambda t: "Z" if t != "V" else "V"
    pairs = {zero(a) + zero(b) for t in trips for a, b in zip(t, t[1:])}
    assert pairs == {"VV", "VZ", "ZV", "ZZ"}, f"orders of neighbouring trips: {sorted(pairs)}"
    assert any(t[0] != "V" for t in trips) and any(t[-1] != "V" for t in trips), "a zero entry as a first and as a last trip"
    assert set(kinds) == set("VABCD"), f"kinds {sorted(set(kinds))}"
    valid = [k for k in range(stored) if kinds[k] == "V"]
    seen = {}
    for k in valid:
        seen.setdefault(tuple(index[k]), []).append(k)
    assert any(len({k % grid for k in ks}) >= 2 for ks in seen.values()), "one valid entry twice, in different workgroups"
    order = [tuple(index[k]) for k in valid]
    assert order != sorted(order), "valid entries are unsorted"
    assert any(k >= grid and index[k][1] == 0 for k in valid) and any(k >= grid and index[k][1] == 1 for k in valid), \
        "batch 0 (the carried state) and batch 1 (the previous batch) in a later trip"
    first = np.asarray(row_first, np.int64)
    assert len(first) == rows + 1
    assert first[0] > first[1], "a row with first > last"
    assert any(first[r] < stored < first[r + 1] for r in range(rows)), "a row slice cut by `stored`"
    assert any(stored < first[r] < first[r + 1] for r in range(rows)), "a row slice that begins behind `stored`"
    return kinds


def foreign_wave(wave, nbatches, max_batches):
    """the call's audio in a buffer laid out for all of the handle's batches, FOREIGN_FILL behind the call: a stage that read a batch
    behind the call would encode something, not fault"""
    wave = np.asarray(wave, np.float32)
    out = np.full((wave.shape[0], max_batches * WAVE_BATCH), FOREIGN_FILL)
    out[:, :nbatches * WAVE_BATCH] = wave[:, :nbatches * WAVE_BATCH]
    return out


def stored_blocks(count, max_blocks):
    """what the stages make of a count and a capacity: min(count[1], max_blocks)"""
    return min(int(count[1]), int(max_blocks))


FOREIGN_CASES = ("20 entries", "capacity 13", "count 40")


def foreign_case(name, rows=3, nbatches=2, max_batches=8):
    """(index, count, row_first, max_blocks, stored) of the three shapes the foreign index is run at.  "20 entries": 20 entries under
    the handle's full capacity of rows * max_batches.  "capacity 13": the same 20 under max_blocks 13, three trips for workgroup 0 and
    two for the others.  "count 40": a count written by hand above the capacity, over an index buffer of exactly rows * max_batches
    entries; min(count[1], max_blocks) of them are stored.  The properties hold over what is stored."""
    full = rows * max_batches
    if name == "20 entries":
        (index, count, _), cap = foreign_index(rows, nbatches, max_batches, 20), full
    elif name == "capacity 13":
        (index, count, _), cap = foreign_index(rows, nbatches, max_batches, 20), 13
    else:
        assert name == "count 40" and full == 24
        (index, _, _), count, cap = foreign_index(rows, nbatches, max_batches, full), np.array([40, 40], np.uint32), full
    stored = stored_blocks(count, cap)
    assert stored <= len(index)
    row_first = foreign_row_first(rows, stored)
    assert_foreign_properties(index, row_first, rows, nbatches, max_batches, stored)
    return index, count, row_first, cap, stored


# ---------------- audio ----------------

def voice_tones(rows, nb, seed=0):
    """a few tones in the voice band under a slow envelope, up to 0.9 of full scale"""
    rng = np.random.default_rng(1000 + seed)
    n = np.arange(nb * WAVE_BATCH, dtype=np.float64)
    out = np.zeros((rows, len(n)))
    for r in range(rows):
        f = rng.uniform(300.0, 3000.0, 3)
        a = rng.dirichlet(np.ones(3)) * 0.9
        env = 0.55 + 0.45 * np.sin(2 * np.pi * rng.uniform(1.0, 6.0) * n / WAVE_RATE + rng.uniform(0, 6.28))
        out[r] = env * sum(a[i] * np.sin(2 * np.pi * f[i] * n / WAVE_RATE + rng.uniform(0, 6.28)) for i in range(3))
    return out.astype(np.float32)


SQUARE_HALF_PERIODS = (25, 50, 7, 400, 100)


def square(rows, nb, seed=0):
    """Full-scale +-1 square waves whose edges fall between samples 25 j and 25 j + 1: at 16000 every sub-block of row 0 begins
    -32767, 32767 or the reverse (d = 65534, beyond 7 * 32767 / 4: the index0 fallback, 88), and the predictor overshoots the rails;
    at 8000 the filter's overshoot passes +-1 and the quantiser clamps.  Row r has half-period SQUARE_HALF_PERIODS[r % 5]."""
    n = np.arange(nb * WAVE_BATCH)
    out = np.empty((rows, len(n)), np.float32)
    for r in range(rows):
        half = SQUARE_HALF_PERIODS[r % len(SQUARE_HALF_PERIODS)]
        out[r] = np.where(((n - 1) // half) % 2 == 0, 1.0, -1.0)
    return out


def silence(rows, nb, seed=0):
    return np.zeros((rows, nb * WAVE_BATCH), np.float32)


def subnormal(rows, nb, seed=0):
    """values of subnormal size (below 2^-126) of both signs with a few of the smallest normal ones between them: every product with a
    tap is subnormal or zero, every sample quantises to 0, and the carried state must hold these bit patterns as they are"""
    rng = np.random.default_rng(2000 + seed)
    bits = rng.integers(1, 1 << 23, (rows, nb * WAVE_BATCH)).astype(np.uint32)  # exponent field 0
    bits[:, ::97] = 0x00800000  # 2^-126
    bits |= rng.integers(0, 2, bits.shape).astype(np.uint32) << 31
    out = bits.view(np.float32)
    assert (np.abs(out) <= np.float32(2.0 ** -126)).all() and (out != 0).all()
    return out


def ramp(rows, nb, seed=0):
    """-1 .. 1 over the call, row r beginning r / rows of the way along and wrapping"""
    n = nb * WAVE_BATCH
    t = (np.arange(n)[None, :] / n + np.arange(rows)[:, None] / rows) % 1.0
    return (2.0 * t - 1.0).astype(np.float32)


def noise(rows, nb, seed=0):
    return np.random.default_rng(3000 + seed).uniform(-1.0, 1.0, (rows, nb * WAVE_BATCH)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def tie_values():
    """float32 x with x * 32767.0f == n + 0.5 exactly in float32, found by search around (n + 0.5) / 32767: both signs, even and odd n"""
    found = {}
    scale = np.float32(32767.0)
    for n in range(0, 4096):
        x = np.float32((n + 0.5) / 32767.0)
        cands = [x]
        for _ in range(2):
            cands = [np.nextafter(cands[0], np.float32(-1)), *cands, np.nextafter(cands[-1], np.float32(2))]
        for c in cands:
            if np.float32(c) * scale == np.float32(n + 0.5):
                found[n] = np.float32(c)
                break
    ns = np.array(sorted(found))
    assert (ns % 2 == 0).sum() >= 8 and (ns % 2 == 1).sum() >= 8, f"the search found {len(ns)} ties"
    xs = np.array([found[n] for n in ns], np.float32)
    return ns, xs


def ties(rows, nb, seed=0):
    """(for rate 16000) every sample an exact tie of the quantiser, n + 0.5 with even and odd n and both signs: round-half-even gives
    n or n + 1 where round-half-away and truncation give something else"""
    ns, xs = tie_values()
    rng = np.random.default_rng(4000 + seed)
    pick = rng.integers(0, len(xs), (rows, nb * WAVE_BATCH))
    sign = np.where(rng.integers(0, 2, pick.shape) == 0, np.float32(1), np.float32(-1))
    out = (xs[pick] * sign).astype(np.float32)
    v = out * np.float32(32767.0)
    assert (np.abs(v) % 1 == 0.5).all()
    return out


BUILDERS = {"voice": voice_tones, "square": square, "silence": silence, "subnormal": subnormal, "ramp": ramp, "noise": noise, "ties": ties}
TONE_BUILDERS = ("voice",)


@functools.lru_cache(maxsize=None)
def audio(name, rows, nb, seed=0):
    a = BUILDERS[name](rows, nb, seed)
    assert a.dtype == np.float32 and a.shape == (rows, nb * WAVE_BATCH) and np.isfinite(a).all() and (np.abs(a) <= 1).all()
    a.setflags(write=False)
    return a


def snr_db(ref, got):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    return 10 * np.log10((ref ** 2).sum() / ((ref - got) ** 2).sum())
