"""Seeded families of adversarial stage-2 input planes (numpy only, deterministic).

The parity tests feed stage 2 what mi_iqgen_* generated and stage 1 channelised: a few gated carriers over Gaussian noise, 10^3 of
dynamic range, edges wherever gate_samples puts them.  The plane entries (mi_demod_process_planes on the GPU, ao_demod_run_planes in
the oracle) take every sample from the caller, so here each sample is chosen: edges on the boundaries the time-parallel path and
the multi-wave serial kernel cut the work at, levels that graze the squelch threshold, lone samples that break a block regime, a
noise floor that steps, 10^12 of dynamic range, digital silence.

A family is a function (seed, nsteps, L, **kw) -> plane[AGC_EXTRA + nsteps] of float32 for ONE row, every value finite and >= 0
(what the magnitude of a finite I/Q sample can be).  Entry AGC_EXTRA + i is the squelch's raw sample of step i (entry i the AM
audio sample of that step), so "step" positions below are plane index - AGC_EXTRA.  L is the segment length of the time-parallel
path the row is meant for (512 .. 4096).  "Noise" is a level times a log-normal jitter, not Gaussian I/Q.

raw_iq_row(kind, ...) builds the (mag, cplx) pair of a row that needs raw I/Q (NFM, CTCSS, notch, low-pass).
"""
import numpy as np

WAVE_RATE = 16000
WAVE_BATCH = 2000
AGC_EXTRA = 100
NSTEPS = 24 * WAVE_BATCH  # 3 000 blocks: past the default lead of 1 920; 93 segments of 512, 11.7 of 4096

BLOCK = 16                 # steps between noise-floor updates (squelch.cpp:212-214): the block of k_tp_core
GROUPS = (63 * 16, 64 * 16)            # 1008, 1024: a group of the noise-floor wave
PASSES = (4 * 63 * 16, 4 * 64 * 16)    # 4032, 4096: a pass of four groups
TP_W = 4096                # warm-up of a segment lane (kernels.hpp)
LEAD = 1920 * 16           # default MI_AIRBAND_CORE_LEAD, in steps
# burst and gap lengths: the state machine's own constants (squelch.cpp:36-82)
LOW_SIGNAL_ABORT, RING, DELAY, RECENT = 88, 102, 197, 1000
CRITICAL_LENGTHS = tuple(v + d for v in (LOW_SIGNAL_ABORT, RING, DELAY, RECENT) for d in (-1, 0, 1))


def _rng(family, seed):
    return np.random.default_rng([family, seed])


def _jitter(rng, n, sigma=0.1):
    return np.exp(rng.normal(0.0, sigma, size=n))


def _finish(x):
    x = np.asarray(x, dtype=np.float64)
    out = x.astype(np.float32)
    assert out.ndim == 1 and np.isfinite(out).all() and (out >= 0).all()
    return out


def critical_positions(nsteps, L):
    """Every step index in (0, nsteps) that is a boundary of something: group, pass, segment, warm-up start, batch, lead."""
    pos = set()
    for unit in GROUPS + PASSES + (L, WAVE_BATCH):
        pos.update(range(unit, nsteps, unit))
    pos.update(s * L - TP_W for s in range(nsteps // L + 1) if 0 < s * L - TP_W < nsteps)
    if LEAD < nsteps:
        pos.add(LEAD)
    return np.array(sorted(pos))


def _pick_edge(rng, crit, lo, hi):
    """A position in [lo, hi): b - 1, b or b + 1 of a critical boundary b where one is in reach, else of a block boundary."""
    c = crit[(crit >= lo + 1) & (crit < hi - 1)]
    if c.size and rng.random() < 0.75:
        b = int(rng.choice(c))
    else:
        b = int(rng.integers((lo + BLOCK) // BLOCK, max((lo + BLOCK) // BLOCK + 1, (hi - 1) // BLOCK))) * BLOCK
    return min(max(b + int(rng.integers(-1, 2)), lo), hi - 1)


# ---------------------------------------------------------------- 1
def edges_on_boundaries(seed, nsteps=NSTEPS, L=512, floor=1.0):
    """A quiet floor with bursts of 3x, 10x and 1000x the floor whose on and off edges sit at b - 1, b, b + 1 of block, group, pass,
    segment, warm-up, batch and lead boundaries; burst and gap lengths from the state machine's constants +-1."""
    rng = _rng(1, seed)
    crit = critical_positions(nsteps, L)
    x = floor * _jitter(rng, nsteps)
    t = int(rng.integers(200, 1200)) if seed % 2 else 2600 + int(rng.integers(0, 400))
    k = 0
    # one boundary of each kind is not left to chance
    must = sorted({LEAD, 2 * PASSES[0], 2 * PASSES[1], 5 * GROUPS[0], 7 * GROUPS[1], 9 * L if 9 * L < nsteps else L, 3 * WAVE_BATCH,
                   (TP_W // L + 3) * L - TP_W + (0 if L < TP_W else TP_W)})
    while t < nsteps - 50:
        due = [b for b in must if t + 2 <= b < t + 2500 and b < nsteps - 2]
        if due:
            must.remove(due[0])
            on = due[0] + int(rng.integers(-1, 2))
        else:
            on = _pick_edge(rng, crit, t, min(t + 700, nsteps))
        amp = (10.0, 1000.0, 3.0, 10.0)[(k + seed) % 4]
        if rng.random() < 0.5:
            off = on + int(rng.choice(CRITICAL_LENGTHS + (250,)))
        else:
            off = _pick_edge(rng, crit, on + 60, min(on + 1400, nsteps))
        off = min(off, nsteps)
        x[on:off] = floor * amp * _jitter(rng, off - on, 0.05)
        if k % 2 == 0:  # a dropout under the floor behind every other burst: LOW_SIGNAL_ABORT also where the threshold is the floor
            x[off:off + 100] *= 0.5
        t = off + int(rng.choice(CRITICAL_LENGTHS + (300,)))
        k += 1
    return _finish(np.concatenate([np.full(AGC_EXTRA, floor), x]))


# ---------------------------------------------------------------- 2
QUIET_STEPS = 6000  # the first quiet part of a threshold_grazers row: the noise floor has settled on it by then


def threshold_grazers(seed, nsteps=NSTEPS, L=512, floor=1.0, threshold_of=None):
    """After a quiet part the level ramps by 1e-4 (of the threshold) per step up through the squelch threshold and back down through
    it, cycle after cycle, so that `pre_capped >= squelch_level` flips on near-equal operands.  threshold_of(samples so far) -> the
    level the squelch compares against after them: the caller takes it from the oracle's own trace of that prefix, before every
    cycle -- normal_signal_ratio * noise floor, 0.9 of that once three openings within `recent_sample_size` steps have made the
    squelch flappy, or the manual level -- so every cycle swings through the threshold as it then is.  After every eight cycles a
    quiet part of 2 600 steps at a quarter of the one before: long and deep enough for a squelch of 0 dB, whose threshold follows
    the signal down, to close, stay closed for `recent_sample_size` steps and forget that it flapped."""
    assert threshold_of is not None, "threshold_grazers needs the squelch threshold before each cycle, from the oracle's trace"
    rng = _rng(2, seed)
    parts = [floor * _jitter(rng, min(nsteps, QUIET_STEPS), 0.02)]
    have, cycle, quiet_level = parts[0].size, 0, floor
    half = 350 + 25 * (seed % 4)  # steps up, and as many down: +-half/2 * 1e-4 around the threshold
    while have < nsteps:
        thr = float(threshold_of(_finish(np.concatenate(parts))))
        assert thr > 0
        w = np.concatenate([np.arange(-half / 2, half / 2), np.arange(half / 2, -half / 2, -1.0)])[:nsteps - have]
        parts.append(thr * (1.0 + 1e-4 * w) * _jitter(rng, w.size, 1e-3))
        have, cycle = have + w.size, cycle + 1
        if cycle % 8 == 0 and have < nsteps:
            quiet_level *= 0.25
            m = min(nsteps - have, 2600)
            parts.append(quiet_level * _jitter(rng, m, 0.02))
            have += m
    return _finish(np.concatenate([np.full(AGC_EXTRA, floor)] + parts))


# ---------------------------------------------------------------- 3
CALLS = (9, 1, 11, 3)  # the call pattern of the streaming tests: boundaries at steps 18 000, 20 000, 42 000


def flap_and_recover(seed, nsteps=NSTEPS, L=512, floor=1.0):
    """Groups of 4 - 5 bursts of 250 steps with 300-step gaps (recent_open_count reaches 3: the flappy ratio applies), then 999 / 1000
    / 1001 steps of quiet (recent_open_count reset, or not), a burst, and a long quiet.  Two of the groups are placed so that their
    quiet part lies across a call boundary of CALLS."""
    rng = _rng(3, seed)
    x = floor * _jitter(rng, nsteps)

    def group(t, quiet, amp):
        for i in range(4 + seed % 2):
            x[t:t + 250] = floor * amp * _jitter(rng, len(x[t:t + 250]), 0.05)
            if i % 2 == 0:  # a dropout under the floor: LOW_SIGNAL_ABORT also where the threshold is the floor itself
                x[t + 250:t + 350] *= 0.5
            t += 250 + 300
        t += quiet - 300
        x[t:t + 250] = floor * amp * _jitter(rng, len(x[t:t + 250]), 0.05)  # does this one still meet the flappy ratio?
        return t + 250

    # (from the end of a burst to CLOSED: <= 88 steps to LOW_SIGNAL_ABORT + 197 of its delay; the quiet is counted from there)
    quiets = [q + d for q in (RECENT, RECENT + LOW_SIGNAL_ABORT + DELAY, RECENT + DELAY) for d in (-1, 0, 1)]
    glen = (4 + seed % 2) * 550
    bounds = np.cumsum(CALLS)[:-1] * WAVE_BATCH
    starts = [2600 + 16 * (seed % 5), int(bounds[0]) - glen - 400 - 100 * (seed % 3), int(bounds[2]) - glen - 500 - 90 * (seed % 4)]
    k = seed
    t = starts[0]
    while t + glen + 1800 < nsteps:
        for s in starts:  # a group that has to straddle a call boundary goes first
            if t <= s < t + 3000:
                t = s
        t = group(t, quiets[k % len(quiets)], (10.0, 30.0, 6.0)[k % 3]) + 1700 + 16 * (k % 7)
        k += 1
    return _finish(np.concatenate([np.full(AGC_EXTRA, floor), x]))


# ---------------------------------------------------------------- 4
def regime_breakers(seed, nsteps=NSTEPS, L=512, floor=1.0):
    """Stretches where every sample is far above the cap (SATURATED) with single samples below it, and stretches of an exact constant
    (MERGED steady) with single spikes -- the lone sample at position 0, 1 or 15 of a block, in the first or the last block of a
    segment among others."""
    rng = _rng(4, seed)
    x = floor * _jitter(rng, nsteps)
    t = 3000 + 16 * (seed % 9)
    k = seed
    while t + 4500 < nsteps:
        length = (2048, 3072, 4096 + 512)[k % 3]
        lo, hi = t, t + length
        saturated = k % 2 == 0
        if saturated:
            x[lo:hi] = floor * 60.0 * _jitter(rng, length, 0.05)
            lone = (0.0, floor * 0.5, floor * 4.0)  # below any cap the stretch can have (cap = 1.5 * ratio * floor >= 1.5 * floor... and x >> it)
        else:
            x[lo:hi] = floor * (1.0, 2.5, 0.6)[k % 3]  # an exact constant: full_ meets its fixed point, capped_ == full_
            lone = (floor * 1000.0, floor * 2.0, floor * 30.0)
        segs = [s for s in range((lo + 600) // L + 1, hi // L)]
        places = []
        for j, s in enumerate(segs):
            base = s * L if j % 2 == 0 else s * L - BLOCK  # first / last block of a segment
            places.append(base + (0, 1, 15)[(j + k) % 3])
        blocks = rng.integers((lo + 600) // BLOCK, hi // BLOCK, size=6)
        places += [int(b) * BLOCK + (0, 1, 15)[(i + k) % 3] for i, b in enumerate(blocks)]
        for i, p in enumerate(places):
            if lo + 400 <= p < hi:
                x[p] = lone[(i + k) % 3]
        t = hi + 1500 + 16 * (k % 5) + k % 3
        k += 1
    return _finish(np.concatenate([np.full(AGC_EXTRA, floor), x]))


# ---------------------------------------------------------------- 5
def noise_staircase(seed, nsteps=NSTEPS, L=512):
    """The floor itself steps by x2, x30, x1/30, x1/2 and x1/30 again (every cycle leaves it a thirtieth lower) every 2 000 - 7 000 steps,
    with short bursts right after a step down: the operand of the noise-floor minimum, min(capped_, noise_floor_), changes sides, and
    capped_ decays from a cap that the falling noise floor takes along."""
    rng = _rng(5, seed)
    crit = critical_positions(nsteps, L)
    x = np.empty(nsteps)
    cycle = (1.0, 2.0, 60.0, 2.0, 1.0)  # relative to the base, which drops to a thirtieth behind the last one
    base, t, k, prev = 1.0, 0, seed % 3, None
    while t < nsteps:
        level = base * cycle[k % len(cycle)]
        raised = cycle[k % len(cycle)] > 2.0
        e = min(nsteps, t + int(rng.integers(2000, 3501 if raised else 7001)))  # (a raised floor keeps the squelch open: not for long)
        if e < nsteps:
            e = _pick_edge(rng, crit, max(t + 1500, e - 300), min(nsteps, e + 300))
        x[t:e] = level * _jitter(rng, e - t)
        if prev is not None and level < prev:
            b = t + int(rng.choice((1, 16, 40, 88, 197)))
            x[b:min(e, b + int(rng.choice((100, 197, 300))))] *= 12.0
        prev, t, k = level, e, k + 1
        if k % len(cycle) == 0 and base > 1e-4:
            base /= 30.0
    return _finish(np.concatenate([np.full(AGC_EXTRA, 1.0), x]))


# ---------------------------------------------------------------- 6
def dynamic_range(seed, nsteps=NSTEPS, L=512):
    """seed % 3 == 0: a floor of 1e-3 with one-sample and 100-sample spikes of 1e4, 1e6 and 1e9, early and late in each call of CALLS --
    10^12 of range, beyond what the warm-up of the full_ sandwich (TP_W1) closes; 1: the same scaled so that the floor is 1e-20;
    2: a row that is huge throughout (1e20) but for two dips.  The spikes of 1e4 come 300 samples wide as well: a spike has to
    outlast the opening delay for the squelch to open on it.  The scaled rows are for a manual threshold down there (the 1e-6 a
    block that the noise floor gains would bury them under any SNR threshold)."""
    rng = _rng(6, seed)
    kind = seed % 3
    if kind == 2:
        x = 1e20 * _jitter(rng, nsteps)
        # dips of 20 orders of magnitude, down to where the noise floor started (5): the row closes, and opens again behind them
        for at in (nsteps // 3 + 16 * (seed % 7), 2 * nsteps // 3 - seed % 16):
            x[at:at + 700] *= 1e-20
        return _finish(np.concatenate([np.full(AGC_EXTRA, 1e20), x]))
    scale = 1.0 if kind == 0 else 1e-17
    x = 1e-3 * _jitter(rng, nsteps)
    bounds = [0] + [int(b) * WAVE_BATCH for b in np.cumsum(CALLS) if b * WAVE_BATCH <= nsteps]
    spikes = (1e4, 1e6, 1e9)
    k = seed // 3
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        for at in (lo + 40 + 16 * (k % 4), lo + 700 + k % 16, hi - 900 - k % 16, hi - 130 + (k % 3)):
            if lo <= at and at + 300 <= hi:
                width = 1 if k % 2 == 0 else (300 if k % 3 == 0 else 100)
                x[at:at + width] = spikes[k % 3] * (1.0 if width == 1 else _jitter(rng, width, 0.05))
            k += 1
    return _finish(np.concatenate([np.full(AGC_EXTRA, 1e-3), x]) * scale)


# ---------------------------------------------------------------- 7
def silence(seed, nsteps=NSTEPS, L=512):
    """seed % 4 == 0: 12 000 and more steps of exact 0.0 (capped_ and full_ pass through the subnormals to 0), then noise and bursts with silence between them;
    1: 1e-40 throughout (subnormal); 2: exact 0.0 throughout (every call a silent one; seeds from 4 on: a stretch of noise near the end); 3: noise and bursts with the one-batch call of
    CALLS and the tail of the row exactly 0.0."""
    rng = _rng(7, seed)
    kind = seed % 4
    if kind == 1:
        return np.full(AGC_EXTRA + nsteps, 1e-40 * (1 + seed // 4), np.float32)
    if kind == 2:
        x = np.zeros(AGC_EXTRA + nsteps, np.float32)
        if seed // 4:  # (further seeds: noise at the very end, so that no two rows are the same)
            tail = WAVE_BATCH * (1 + seed // 4 % 3) - seed // 4
            x[-tail:-700] = _jitter(rng, tail - 700)  # (it opens the squelch; the silence behind it closes it again)
        return x
    x = 1.0 * _jitter(rng, nsteps)
    for t in range(2500 + 16 * (seed // 4), nsteps - 600, 2900):
        x[t:t + 420] *= 10.0
    head = np.full(AGC_EXTRA, 1.0)
    if kind == 0:
        z = 12000 + 16 * (seed // 4) + seed // 4
        x[:z] = 0.0
        head[:] = 0.0
        # The noise floor has followed the silence down and only creeps back (1e-6 a block), so noise of 1 is a strong signal from
        # here on: stretches of it open the squelch, and silence between them closes it again.
        for t in range(z + 3000, nsteps, 4400):
            x[t:t + 1500] = 0.0
        x[nsteps - 1200:] = 0.0
    else:
        x[18000:20000] = 0.0
        x[min(42000, nsteps - 6000):] = 0.0
    return _finish(np.concatenate([head, x]))


# ---------------------------------------------------------------- 8
def random_walk(seed, nsteps=NSTEPS, L=512):
    """Piecewise-constant log-uniform levels over 10^5 (under the jitter), piece lengths drawn from the critical lengths and the edges
    from the critical positions."""
    rng = _rng(8, seed)
    crit = critical_positions(nsteps, L)
    lengths = CRITICAL_LENGTHS + (16, 17, 250, 300, 1008, 1024, 2000, 2001, 4096)
    x = np.empty(nsteps)
    t = 0
    while t < nsteps:
        if rng.random() < 0.5:
            e = t + int(rng.choice(lengths))
        else:
            e = _pick_edge(rng, crit, t + 16, min(nsteps, t + 3000)) if t + 20 < nsteps else nsteps
        e = min(max(e, t + 1), nsteps)
        x[t:e] = 10.0 ** rng.uniform(-2.0, 3.0) * _jitter(rng, e - t, 0.08)
        t = e
    return _finish(np.concatenate([np.full(AGC_EXTRA, 1.0), x]))


FAMILIES = {"edges_on_boundaries": edges_on_boundaries, "threshold_grazers": threshold_grazers, "flap_and_recover": flap_and_recover,
            "regime_breakers": regime_breakers, "noise_staircase": noise_staircase, "dynamic_range": dynamic_range, "silence": silence,
            "random_walk": random_walk}


# ---------------------------------------------------------------- rows that need raw I/Q
RAW_IQ_KINDS = ("nfm", "ctcss", "notch", "lowpass_outside", "lowpass_inside")


def raw_iq_row(kind, seed, nsteps=NSTEPS, L=512, scale=1.0):
    """(mag[AGC_EXTRA + nsteps], cplx[AGC_EXTRA + nsteps][2]) of a row with needs_raw_iq.  The envelope is one of the families above
    times `scale` (at most 1e15, so that re^2 + im^2 stays finite); the phase carries what the row needs:
      nfm              a 1 kHz tone (2.5 kHz deviation)
      ctcss            the same plus 100 Hz FM switched on and off every 14 000 steps while the envelope keeps the squelch open for
                       long stretches: ctcss_count and no_ctcss_count both move
      notch            a 100 Hz component (in the envelope, and as FM: the notch filters the demodulated audio of either modulation)
      lowpass_outside  sections by turns: mag strong + energy at DC (inside the filter), mag strong + energy at +-7 kHz (outside a
                       bandwidth of 5 000: has_pre && !has_post, process_filtered closes the squelch), mag weak + strong in-band I/Q
                       (the reverse disagreement), both weak.  mag is NOT |cplx| here: that is the point
      lowpass_inside   the same sections in another order and with -7 kHz
    For the other kinds mag is sqrt(re^2 + im^2) in float32, as stage 1 would leave it."""
    assert kind in RAW_IQ_KINDS and scale <= 1e15
    rng = _rng(9 + RAW_IQ_KINDS.index(kind), seed)
    count = AGC_EXTRA + nsteps
    k = np.arange(count, dtype=np.float64)
    if kind in ("lowpass_outside", "lowpass_inside"):
        sign = 1.0 if kind == "lowpass_outside" else -1.0
        order = (0, 1, 3, 2, 0, 1) if kind == "lowpass_outside" else (1, 0, 2, 3, 1, 1)
        mag = np.empty(count)
        amp = np.empty(count)
        freq = np.zeros(count)
        t, j = 0, seed
        while t < count:
            e = min(count, t + 2300 + 16 * (j % 7) + (j % 3))
            sec = order[j % len(order)]
            mag[t:e] = (12.0, 12.0, 1.0, 1.0)[sec]
            amp[t:e] = (12.0, 12.0, 12.0, 1.0)[sec]
            freq[t:e] = (0.0, sign * 7000.0, 0.0, 0.0)[sec]
            t, j = e, j + 1
        mag *= _jitter(rng, count, 0.05) * scale
        amp *= _jitter(rng, count, 0.05) * scale
        phase = 2.0 * np.pi * np.cumsum(freq) / WAVE_RATE + 0.3
        cplx = np.stack([amp * np.cos(phase), amp * np.sin(phase)], axis=1).astype(np.float32)
        return _finish(mag), cplx
    if kind == "ctcss":
        env = np.full(count, 1.0) * _jitter(rng, count, 0.1)
        t, j = 3000, seed
        while t < count:  # long transmissions with short pauses
            e = min(count, t + 20000 + 1000 * (j % 3))
            env[t:e] *= 12.0
            t, j = e + 1500, j + 1
    else:
        env = FAMILIES["edges_on_boundaries" if kind == "nfm" else "flap_and_recover"](seed, nsteps, L).astype(np.float64)
    env = env * scale
    audio = 2500.0 * np.sin(2.0 * np.pi * 1000.0 * k / WAVE_RATE)  # instantaneous frequency in Hz
    if kind == "ctcss":
        on = ((k // 14000).astype(np.int64) + seed) % 2 == 0
        audio = audio + np.where(on, 600.0 * np.sin(2.0 * np.pi * 100.0 * k / WAVE_RATE), 0.0)
    if kind == "notch":
        audio = audio + 800.0 * np.sin(2.0 * np.pi * 100.0 * k / WAVE_RATE)
        env = env * (1.0 + 0.3 * np.sin(2.0 * np.pi * 100.0 * k / WAVE_RATE))
    phase = 2.0 * np.pi * np.cumsum(audio) / WAVE_RATE
    cplx = np.stack([env * np.cos(phase), env * np.sin(phase)], axis=1).astype(np.float32)
    assert np.isfinite(cplx).all()
    mag = np.sqrt(cplx[:, 0] * cplx[:, 0] + cplx[:, 1] * cplx[:, 1])  # float32 throughout, like rtl_airband.cpp:508
    return _finish(mag), cplx


def cplx_for(kind, seed, nsteps=NSTEPS, L=512, scale=1.0):
    """[AGC_EXTRA + nsteps][2]: the complex plane of raw_iq_row."""
    return raw_iq_row(kind, seed, nsteps, L, scale)[1]
