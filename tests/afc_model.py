"""A float64 model of AFC (rtl_airband.cpp:180-251), written from the rule and signal theory in the manner of
signal_model.py.  numpy only; it calls neither the oracle nor the package nor plan.cpp.

What the reference does, once per batch and channel with afc > 0, after the batch's sample loop (:648-652):

  spectrum   fftout still holds the FFT of the last window pushed before the batch trigger (:514-516).  A batch is
             WAVE_BATCH = 2000 windows and the first one waits for AGC_EXTRA = 100 more, so batch b ends on window
             WAVE_BATCH + AGC_EXTRA - 1 + b * WAVE_BATCH, input samples [w * hop, w * hop + N).  square() is re^2 + im^2.
  finalize   prev = the indicator the previous batch left (NO_SIGNAL before the first), cur = this batch's.
             prev NO_SIGNAL and cur not: walk.  prev not NO_SIGNAL and cur NO_SIGNAL: bins[i] = base_bins[i].  Else nothing.
  walk       check<-1> from the base bin; only if that did not move, check<+1>.  bins[i] is stored, and the indicator becomes
             AFC_UP '<' (bin > base) or AFC_DOWN '>' (bin < base), only if the result differs from bins[i].
  check      from bin = base, step by step: stop at the edge (bin 0 going down, bin N - 1 going up: no wrap); stop when the next
             bin's value <= the BASE bin's value; on the first step set threshold = (value - base_value) / afc; on later steps
             stop when value - base_value < threshold, else threshold += threshold / 10.  The base bin's value is used
             throughout, never the current bin's.

The model has no squelch: it is fed the per-batch indicators of the backend under test and reads only "is NO_SIGNAL / is not"
from them ('<' and '>' count as not NO_SIGNAL).  Every float comparison it evaluates is recorded with its margin
|lhs - rhs| / max(spectrum), so that a test can assert that no decision is a near-tie a float32 spectrum may take differently.
"""
import numpy as np

import signal_model as sm

WAVE_BATCH = 2000
AGC_EXTRA = sm.AGC_EXTRA
NO_SIGNAL, SIGNAL, AFC_UP, AFC_DOWN = ord(" "), ord("*"), ord("<"), ord(">")
WALK, RETURN = "walk", "return"


def last_window(batch):
    """Index of the last window pushed before batch `batch` is processed."""
    return WAVE_BATCH + AGC_EXTRA - 1 + batch * WAVE_BATCH


def spectrum(x, sample_rate, n, w):
    """|FFT|^2 of window w of the complex samples x: sum_m x[w hop + m] win[m] e^{-2 pi j k m / N}, all N bins."""
    hop = sm.hop_of(sample_rate)
    if w < 0 or w * hop + n > x.size:
        raise ValueError("window outside the capture")
    X = np.fft.fft(np.asarray(x[w * hop:w * hop + n], dtype=np.complex128) * sm.window(n))
    return X.real ** 2 + X.imag ** 2


def walk(sq, step, base, afc, margins=None):
    """check<step> over the squared spectrum sq: the bin the walk ends on.  margins: a list that receives
    |lhs - rhs| / max(sq) of every float comparison evaluated."""
    n = len(sq)
    top = float(np.max(sq))
    base_value = float(sq[base])
    threshold = 0.0
    b = base
    while True:
        if step < 0:
            if b < 1:
                break
        elif b + 1 >= n:
            break
        value = float(sq[b + step])
        if margins is not None:
            margins.append(abs(value - base_value) / top)
        if value <= base_value:
            break
        if b == base:
            threshold = (value - base_value) / float(afc)
        else:
            if margins is not None:
                margins.append(abs((value - base_value) - threshold) / top)
            if value - base_value < threshold:
                break
            threshold = threshold + threshold / 10.0
        b += step
    return b


def finalize_walk(sq, base, afc, margins=None):
    """Down first, up only if down did not move."""
    b = walk(sq, -1, base, afc, margins)
    if b == base:
        b = walk(sq, +1, base, afc, margins)
    return b


class Result:
    """spectra [nbat][N]; base [nch]; bins [nch][nbat] after each batch; flags [nch][nbat] the batch must carry;
    action [nch][nbat] in {WALK, RETURN, None}; margins [(channel, batch, margin)]."""

    def __init__(self, spectra, base, bins, flags, action, margins):
        self.spectra, self.base, self.bins, self.flags, self.action, self.margins = spectra, base, bins, flags, action, margins

    def min_margin(self):
        return min((m for _, _, m in self.margins), default=np.inf)

    def moved(self, c):
        """Batches in which a walk changed channel c's bin, and batches in which it went back to its base from elsewhere."""
        walks = [b for b in range(self.bins.shape[1]) if self.action[c][b] == WALK and self.bins[c, b] != self.base[c]]
        returns = [b for b in range(1, self.bins.shape[1]) if self.action[c][b] == RETURN and self.bins[c, b - 1] != self.base[c]]
        return walks, returns


def run(raw, dev, chans, flags, shift=0):
    """raw: the IQ bytes of one stream.  dev / chans: objects with the fields of the device and channel configuration.
    flags: uint8 [nch][nbat], the backend's indicators.  shift: take the spectrum `shift` windows late (a test of the test)."""
    flags = np.asarray(flags, dtype=np.uint8)
    nch, nbat = flags.shape
    assert nch == len(chans)
    n = 1 << dev.fft_size_log
    x = sm.samples_from_bytes(raw, dev.sfmt, dev.fullscale)
    spectra = np.stack([spectrum(x, dev.sample_rate, n, last_window(b) + shift) for b in range(nbat)])
    base = np.array([sm.bin_index(c.freq, dev.centerfreq, dev.sample_rate, n) for c in chans], np.int64)
    bins = np.zeros((nch, nbat), np.int64)
    out = np.where(flags == NO_SIGNAL, NO_SIGNAL, SIGNAL).astype(np.uint8)
    action = [[None] * nbat for _ in range(nch)]
    margins = []
    for c, ch in enumerate(chans):
        cur, prev_open = int(base[c]), False
        for b in range(nbat):
            is_open = flags[c, b] != NO_SIGNAL
            if ch.afc != 0:
                if is_open and not prev_open:
                    action[c][b] = WALK
                    m = []
                    to = finalize_walk(spectra[b], int(base[c]), ch.afc, m)
                    margins += [(c, b, v) for v in m]
                    if to != cur:
                        cur = to
                        if to > base[c]:
                            out[c, b] = AFC_UP
                        elif to < base[c]:
                            out[c, b] = AFC_DOWN
                elif prev_open and not is_open:
                    action[c][b] = RETURN
                    cur = int(base[c])
            bins[c, b] = cur
            prev_open = is_open
    return Result(spectra, base, bins, out, action, margins)
