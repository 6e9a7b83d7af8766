"""Cases for AFC (rtl_airband.cpp:180-251), shared by tests/test_afc_model.py (oracle against the float64 model of
afc_model.py, no GPU) and tests/test_gpu_afc.py (HIP against the oracle bit for bit, and against the model).  Plain helpers,
no pytest hooks.

Captures are made by numpy: float64 tones plus a little seeded Gaussian noise, rounded to u8 (the wider formats are the same
values widened).  A tone is given in true FFT bins relative to the base bin of the channel it belongs to and is gated in
"batch positions": position p is window 2000 p + 100, so p = 1.5 is the middle of what the squelch sees in batch 1 and every
transition falls inside a batch.  A tone `d` bins off sits |d| + 0.2 bins from the base bin: exactly on the grid the spectrum
is symmetric about the peak and the walk's `value <= base_value` test across the peak (bin base + 2 d against the base bin)
would be a tie that only the noise decides.

Every channel states what its bin must do: +1 / -1 it must walk up / down at least once and return to its base inside the
run, 0 it must never move.
"""
import functools

import numpy as np

import signal_model as sm
from afc_model import AGC_EXTRA, WAVE_BATCH, last_window

CENTRE = 120000000
SFMT = {"u8": (sm.SFMT_U8, 127.5), "s8": (sm.SFMT_S8, 127.5), "s16": (sm.SFMT_S16, 32767.0), "f32": (sm.SFMT_F32, 1.0)}
NOISE_LSB = 0.3
OFF_GRID = 0.2
BURSTS = ((1.5, 4.5), (6.5, 8.5))  # the first burst gives the walk and the return every moving channel must show
SHORT = ((1.5, 3.5), (5.5, 7.5))   # the same in 8 batches

# Largest |sq_oracle - sq_model| / max(sq_model) over every batch's AFC spectrum of every case and stream, as printed by
# tests/test_afc_model.py::test_oracle_bins_flags_and_spectrum_equal_the_model: 3.55e-7 (`edges`; 2.0e-7 .. 3.4e-7 elsewhere).  The margin is 4 x that, the
# rule of stage1_plans.STAGE1_BOUND.  The smallest margin of any comparison in the cases is 3.5e-5 (`rows65`, stream 4).
SQ_MEASURED = 3.55e-7
MARGIN = 4 * SQ_MEASURED


class Chan:
    """bin: the base bin wanted; off: its tone in bins from the base (None: it shares the tone of an earlier channel at the same
    bin, or has none); amp: tone amplitude in LSB of u8; expect: +1 / -1 / 0; fm: (tone Hz, deviation Hz) of a frequency-modulated
    carrier (CTCSS channels open on nothing else); kw: further channel settings."""

    def __init__(self, bin, afc, off=None, amp=5.0, expect=None, fm=None, marker=(), more=(), **kw):
        self.bin, self.afc, self.off, self.amp, self.fm, self.kw = bin, afc, off, amp, fm, kw
        self.more = tuple(more)      # further tones of its own: (bins from the base, amplitude)
        self.marker = tuple(marker)  # batches whose LAST window alone holds a burst one bin below the base (see MARKER)
        self.expect = expect if expect is not None else (0 if afc == 0 or not off else (1 if off > 0 else -1))


class Tone:
    """pos: position in FFT bins (0 .. N, fractional); amp in LSB; spans in batch positions; fm as above."""

    def __init__(self, pos, amp, spans=BURSTS, fm=None, samples=None):
        self.pos, self.amp, self.spans, self.fm = pos, amp, spans, fm
        self.samples = samples  # [(first, end)] in input samples, instead of spans


class Case:
    def __init__(self, name, log2n, chans, rate=2560000, sfmt="u8", nbat=10, nstreams=1, spans=BURSTS, extra_tones=(), stream_off=None):
        self.name, self.log2n, self.chans, self.rate, self.sfmt, self.nbat, self.nstreams = name, log2n, chans, rate, sfmt, nbat, nstreams
        self.spans, self.extra_tones = spans, list(extra_tones)
        self.stream_off = stream_off  # (stream, channel index, off) -> off of that stream's capture; None: every stream alike
        self.n = 1 << log2n

    # ---- configuration, for either binding (libs.* / pkg.*)
    def device(self, mk):
        code, fullscale = SFMT[self.sfmt]
        return mk(sample_rate=self.rate, centerfreq=CENTRE, fft_size_log=self.log2n, sfmt=code, fullscale=fullscale)

    def freq(self, b):
        """One Hz above the true grid point of bin b (the upper half of the spectrum lies below the centre)."""
        return CENTRE + int(round((b if b < self.n // 2 else b - self.n) * self.rate / self.n)) + 1

    def channels(self, mk):
        return [mk(self.freq(c.bin), afc=c.afc, **c.kw) for c in self.chans]

    def base_bins(self):
        return [sm.bin_index(self.freq(c.bin), CENTRE, self.rate, self.n) for c in self.chans]

    def off(self, s, i):
        c = self.chans[i]
        if c.off is None or self.stream_off is None:
            return c.off
        return self.stream_off(s, i, c.off)

    def expect(self, s, i):
        c = self.chans[i]
        if c.off is None or self.stream_off is None:
            return c.expect
        o = self.off(s, i)
        return 0 if c.afc == 0 or not o else (1 if o > 0 else -1)

    def tones(self, s):
        base = self.base_bins()
        out = list(self.extra_tones)
        for i, c in enumerate(self.chans):
            o = self.off(s, i)
            if o is not None:
                pos = base[i] + o + (OFF_GRID if o > 0 else -OFF_GRID if o < 0 else 0.0)
                out.append(Tone(pos % self.n, c.amp, self.spans, c.fm))
            for o, amp in c.more:
                out.append(Tone((base[i] + o) % self.n, amp, self.spans))
            if c.marker:
                # one hop long, centred in the last window of the batch: the 7-term window is a narrow bell, so that window sees
                # the burst almost whole and the windows before and after it see next to nothing of it
                hop, mid = sm.hop_of(self.rate), self.n // 2
                at = [last_window(b) * hop + mid for b in c.marker]
                out.append(Tone((base[i] - 1) % self.n, MARKER, samples=[(a - hop // 2, a + hop // 2) for a in at]))
        return out

    def bytes_per_stream(self):
        hop = sm.hop_of(self.rate)
        return 2 * ((self.nbat * WAVE_BATCH + AGC_EXTRA) * hop + self.n)

    def capture(self, s):
        """The bytes of stream s: enough for nbat batches by the reference's availability rule (rtl_airband.cpp:417)."""
        return _capture(self, s)


@functools.lru_cache(maxsize=None)
def _capture(case, s):
    hop = sm.hop_of(case.rate)
    ns = case.bytes_per_stream() // 2
    rng = np.random.default_rng([77, s, case.log2n, case.rate])
    t = np.arange(ns, dtype=np.float64)
    x = rng.normal(0.0, NOISE_LSB, ns) + 1j * rng.normal(0.0, NOISE_LSB, ns)
    for tone in case.tones(s):
        ph = 2.0 * np.pi * (tone.pos / case.n * t + rng.uniform())
        if tone.fm:
            hz, dev = tone.fm
            ph = ph + (dev / hz) * np.sin(2.0 * np.pi * hz * t / case.rate)
        gate = np.zeros(ns)
        for s0, s1 in tone.samples or ():
            gate[s0:s1] = 1.0
        for p0, p1 in () if tone.samples else tone.spans:
            gate[max(0, int(round((WAVE_BATCH * p0 + AGC_EXTRA) * hop))):int(round((WAVE_BATCH * p1 + AGC_EXTRA) * hop))] = 1.0
        x += tone.amp * gate * np.exp(1j * ph)
    u8 = np.empty(2 * ns, np.uint8)
    u8[0::2] = np.clip(np.round(x.real + 127.5), 1, 255)
    u8[1::2] = np.clip(np.round(x.imag + 127.5), 1, 255)
    if case.sfmt != "u8":
        v = u8.astype(np.float32) - 127.5
        u8 = {"s8": lambda: np.round(v - 0.5).astype(np.int8), "s16": lambda: np.round(v * 200.0).astype(np.int16),
              "f32": lambda: (v / 128.0).astype(np.float32)}[case.sfmt]().view(np.uint8)
    u8.setflags(write=False)
    return u8


def batch_pos(hop_bytes, done):
    """Byte position of a stream after `done` batches (input_t.bufs, rtl_airband.cpp:691)."""
    return 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * hop_bytes


# ------------------------------------------------------------------ the cases

AM, NFM = sm.MOD_AM, sm.MOD_NFM
MARKER = 16.0   # amplitude of the one-window burst
STRONG = 16.0  # a tone three bins off reaches its channel's base bin through the skirt of the window


def _spread(n, k, count):
    """Base bin of the k-th of `count` channels: evenly over the spectrum, clear of bin 0, N / 2 and N - 1."""
    step = (n - 32) // count
    b = 16 + k * step
    return b + 8 if abs(b - n // 2) < 8 else b


def _walk_rules(n):
    offs = [(+1, 1), (-1, 2), (+2, 5), (-2, 255), (+3, 1), (-3, 2), (+1, 5), (-1, 255), (+2, 1), (-2, 2), (+3, 255), (-3, 5), (+2, 2), (-2, 1)]
    count = len(offs) + 4
    ch = [Chan(_spread(n, k, count), afc, off, amp=STRONG if abs(off) == 3 else 5.0) for k, (off, afc) in enumerate(offs)]
    ch.append(Chan(_spread(n, 14, count), 1, 0, expect=0))     # on frequency
    ch.append(Chan(ch[8].bin, 0))                              # afc = 0 on the frequency of the +2 / afc 1 channel: shares its tone
    # two channels three bins apart with one tone between them: both walks end on the tone's bin (SAME_END)
    b = _spread(n, 15, count)
    ch.append(Chan(b, 1, +1))
    ch.append(Chan(b + 3, 1, None, expect=-1))
    # its carrier is two bins up, but the last windows of the batches it opens in (1 and 6) hold a burst one bin down: the walk
    # goes down there, and up in the spectrum of the window before or after (MARKED)
    ch.append(Chan(_spread(n, 16, count), 1, +2, expect=-1, marker=(1, 6)))
    # between two carriers, the stronger one above: down is tried first and moves, so up is never tried
    ch.append(Chan(_spread(n, 17, count), 1, None, expect=-1, more=((-2.2, 5.0), (+2.2, 8.0))))
    return ch


def _sizes(n):
    """The same offsets in bins at another size, format or hop: +-1, +-2, +-3 with afc 1, 2, 5, 255, one channel on frequency
    and one with afc = 0."""
    offs = [(+1, 255), (-1, 1), (+2, 2), (-2, 5), (+3, 2), (-3, 1)]
    ch = [Chan(_spread(n, k, 7), afc, off, amp=STRONG if abs(off) == 3 else 5.0) for k, (off, afc) in enumerate(offs)]
    ch.append(Chan(_spread(n, 6, 7), 1, 0, expect=0))
    ch.append(Chan(ch[2].bin, 0))
    return ch


def _types(n):
    """Every channel type under AFC beside an afc = 0 twin of the same type on the same frequency."""
    kinds = [dict(has_iq_outputs=1), dict(bandwidth=8000), dict(modulation=NFM, has_iq_outputs=1),
             dict(modulation=NFM, notch=1000.0, notch_q=5.0, ctcss=100.0), dict(modulation=NFM, tau=0)]
    ch = []
    for k, kw in enumerate(kinds):
        off = +2 if k % 2 == 0 else -2
        fm = (100.0, 600.0) if kw.get("ctcss") else None
        ch.append(Chan(_spread(n, k, 5), 1 + k % 2, off, fm=fm, **kw))
        ch.append(Chan(ch[-1].bin, 0, **kw))
    return ch


def _edges(n):
    """One strong carrier on the centre frequency (bin 0).  Channels a few bins above bin 0 walk down to it and stop; channels a
    few bins below N - 1 walk up to N - 1 and stop there, although sq[0] beyond the edge is larger."""
    return [Chan(3, 1, expect=-1), Chan(2, 255, expect=-1), Chan(n - 4, 1, expect=+1), Chan(n - 3, 2, expect=+1), Chan(n // 3, 1, expect=0)]


def _rows65(n):
    afcs = [1, 2, 5, 255, 1, 0, 2, 5, 255, 1, 2, 0, 5]
    return [Chan(_spread(n, k, 13), a, +1, amp=7.0) for k, a in enumerate(afcs)]


def _rows65_off(s, i, off):
    """Stream s hears channel i's carrier (i + 2 s) mod 5 - 2 bins off: -2 .. +2, different from stream to stream."""
    return (i + 2 * s) % 5 - 2


CASES = {c.name: c for c in [
    Case("walk_rules", 9, _walk_rules(512)),
    # (a manual squelch level: the automatic one starts from a noise floor of 5.0 that only ever falls, squelch.cpp:36-82, and a
    # carrier that is there from the first sample keeps it up)
    Case("first_batch", 9, [Chan(100, 1, +2, squelch_threshold_dbfs=-30), Chan(200, 2, -1, squelch_threshold_dbfs=-30),
                            Chan(100, 0, squelch_threshold_dbfs=-30), Chan(300, 5, +3, amp=STRONG, squelch_threshold_dbfs=-30)],
         nbat=8, spans=((-1.0, 2.5), (4.5, 6.5))),
    # (two streams with the same tones: beyond sq[N - 1] of stream 0 lies sq[0] of stream 1, the carrier itself, so a walk that
    # did not stop at N - 1 would run on into it)
    Case("edges", 9, _edges(512), nstreams=2, extra_tones=[Tone(0.0, 60.0)]),
    Case("types", 9, _types(512), nbat=12, spans=((1.5, 6.5), (8.5, 11.5))),
    Case("fft256", 8, _sizes(256)),
    Case("fft2048", 11, _sizes(2048)),
    Case("fft4096", 12, _sizes(4096), nbat=8, spans=SHORT),
    Case("fft8192", 13, _sizes(8192), nbat=8, spans=SHORT),
    Case("s8", 9, _sizes(512), sfmt="s8"),
    Case("s16", 9, _sizes(512), sfmt="s16"),
    Case("f32", 9, _sizes(512), sfmt="f32"),
    Case("hop150", 9, _sizes(512), rate=2400000),
    # hop 151, 302 bytes: the later batches of a handle's first call start 8 bytes off a multiple of 16
    Case("hop151", 9, _sizes(512), rate=2416000),
    Case("rows65", 9, _rows65(512), nbat=8, nstreams=5, spans=SHORT, stream_off=_rows65_off),
]}
EDGE_END = {0: 0, 1: 0, 2: 511, 3: 511}  # `edges`: the bin each of the first four channels must end its walk on
MARKED = 18                              # `walk_rules`: the channel with the one-window burst
SAME_END = (16, 17)                      # `walk_rules`: the two channels whose walks end on one bin


# ------------------------------------------------------------------ the oracle, batch by batch

BYTES_PER_SAMPLE = {"u8": 1, "s8": 1, "s16": 2, "f32": 4}


@functools.lru_cache(maxsize=None)
def oracle(case, s):
    """The oracle over stream s, one batch per run so that the bin table and the spectrum can be read in between.  Computed once
    and shared; nothing changes it.  A dict: flags [nch][nbat], bins [nch][nbat] after each batch, base [nch], sq [nbat][N] the
    squared spectrum handed to the walk, audio [nch][nbat * 2000], iq [nch][nbat * 2000 * 2], counters [nch][5], levels [nch]."""
    import libs
    dev, chans = case.device(libs.device_cfg), case.channels(libs.channel_cfg)
    raw = case.capture(s)
    hop_bytes = 2 * BYTES_PER_SAMPLE[case.sfmt] * sm.hop_of(case.rate)
    od = libs.OracleDemod(dev, chans)
    flags, bins, sq, audio, iq = [], [], [], [], []
    for b in range(case.nbat):
        nb, wo, axc, iqo = od.run(raw[batch_pos(hop_bytes, b):], 1, want_iq=True)
        assert nb == 1
        flags.append(axc[:, 0].copy()), bins.append(od.bins()[0]), sq.append(od.afc_spectrum()), audio.append(wo), iq.append(iqo)
    out = dict(flags=np.stack(flags, axis=1), bins=np.stack(bins, axis=1), base=od.bins()[1], sq=np.stack(sq), audio=np.concatenate(audio, axis=1),
               iq=np.concatenate(iq, axis=1), counters=od.counters(), levels=od.squelch_levels())
    od.close()
    for v in out.values():
        v.setflags(write=False)
    return out
