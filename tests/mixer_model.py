"""The yardstick of the mixer tests: mix_waveforms and mixer_thread's input loop (src/mixer.cpp:56-98, 133-140, 190-213) written out in
numpy, operation for operation, and the planes and input lists the oracle and the device are run over.  It does not call into the library.

What the reference does not read, the planes fill with NaN: the samples of a NO_SIGNAL batch (an input is copied only when it has a
signal), a row no input lists, and the padding behind the call.  One row carries +Inf in the batches where it signals: an input whose
multiplier is 0.0f is not added at all (mix_waveforms returns at once), so Inf must not reach that channel -- Inf * 0 is NaN."""
import numpy as np

from common import WAVE_BATCH

NO_SIGNAL, SIGNAL, AFC_UP, AFC_DOWN = ord(" "), ord("*"), ord("<"), ord(">")
ROWS = 8                 # rows 0 .. 6 are listed by some input, row 7 by none
INF_ROW, UNLISTED_ROW = 2, 7
SILENT_BATCH, LONE_BATCH = 1, 2  # nobody signals (nb >= 2); INF_ROW alone signals (nb >= 3)


def numpy_mixer(inputs, wave, axc, nb):
    stereo = any(b != 0.0 for _, _, b in inputs)
    left = np.zeros(nb * WAVE_BATCH, np.float32)
    right = np.zeros(nb * WAVE_BATCH, np.float32)
    out = np.full(nb, ord(" "), np.uint8)
    for b in range(nb):
        sl = slice(b * WAVE_BATCH, (b + 1) * WAVE_BATCH)
        for row, amp, bal in inputs:
            if axc[row, b] == ord(" "):
                continue
            ampl = np.float32(min(np.float32(1.0), np.float32(1.0) - np.float32(bal)))
            ampr = np.float32(min(np.float32(1.0), np.float32(1.0) + np.float32(bal)))
            ml, mr = np.float32(amp) * ampl, np.float32(amp) * ampr
            if ml != 0:
                left[sl] = left[sl] + wave[row, sl] * ml
            if stereo and mr != 0:
                right[sl] = right[sl] + wave[row, sl] * mr
            out[b] = ord("*")
    return left, (right if stereo else None), out


def case(seed, rows=6, nb=5):
    rng = np.random.default_rng(seed)
    wave = rng.uniform(-1, 1, (rows, nb * WAVE_BATCH + 100)).astype(np.float32)
    axc = np.where(rng.random((rows, nb)) < 0.6, ord("*"), ord(" ")).astype(np.uint8)
    axc[1, 2] = ord("<")  # AFC indicators count as signal (output.cpp:564)
    axc[:, 3] = ord(" ")  # a batch nobody talks in
    return wave, axc


def mixer_planes(rows, nb, pad, seed=0):
    """(wave float32 [rows][(nb + pad) * WAVE_BATCH], axc uint8 [rows][nb + pad]) for a call of nb batches.  Flags are drawn at 0.6 open;
    batch 0 has a '<' on row 1, a '>' on row 3 and a signal on INF_ROW; batch SILENT_BATCH is NO_SIGNAL on every listed row; in
    batch LONE_BATCH INF_ROW alone of them signals (as far as nb has these batches).  Samples are uniform in [-1, 1) where a listed row signals,
    +Inf on every 97th sample of INF_ROW's signalling batches, and NaN wherever the mixer must not look: NO_SIGNAL batches, the last
    row (which no input lists; its flags are all '*') and the `pad` batches behind the call (flags '*')."""
    assert rows > max(INF_ROW, 3) + 1 and nb >= 1
    rng = np.random.default_rng([seed, rows, nb, pad])
    axc = np.where(rng.random((rows, nb + pad)) < 0.6, SIGNAL, NO_SIGNAL).astype(np.uint8)
    axc[1, 0], axc[3, 0], axc[INF_ROW, 0] = AFC_UP, AFC_DOWN, SIGNAL
    if nb > SILENT_BATCH:
        axc[:, SILENT_BATCH] = NO_SIGNAL
    if nb > LONE_BATCH:
        axc[:, LONE_BATCH] = NO_SIGNAL
        axc[INF_ROW, LONE_BATCH] = SIGNAL
    axc[:, nb:] = SIGNAL
    axc[rows - 1] = SIGNAL
    wave = rng.uniform(-1, 1, (rows, (nb + pad) * WAVE_BATCH)).astype(np.float32)
    inf_at = np.arange(5, WAVE_BATCH, 97)
    for b in range(nb):
        if axc[INF_ROW, b] != NO_SIGNAL:
            wave[INF_ROW, b * WAVE_BATCH + inf_at] = np.inf
    per_sample = np.repeat(axc, WAVE_BATCH, axis=1)
    wave[per_sample == NO_SIGNAL] = np.nan
    wave[:, nb * WAVE_BATCH:] = np.nan
    wave[rows - 1] = np.nan
    return wave, axc


# (row, ampfactor, balance).  Rows 0 .. 6 of mixer_planes(ROWS, ...); INF_ROW's ampfactor is never negative (Inf - Inf is NaN too)
MONO_ONE = [(0, 1.0, 0.0)]
MONO_NINE = [(0, 1.0, 0.0), (3, 0.5, 0.0), (1, 2.0, 0.0), (INF_ROW, 0.0, 0.0), (4, 0.25, 0.0), (3, 0.75, 0.0), (5, -0.0, 0.0), (6, 1.5, 0.0),
             (1, -1.0, 0.0)]  # rows 1 and 3 twice, 0.0 on the row that signals alone in LONE_BATCH, -0.0
STEREO_INF_LEFT = [(INF_ROW, 1.0, -1.0), (0, 1.0, 1.0), (4, 0.7, 0.25), (1, 1.0, 0.0)]
STEREO_INF_RIGHT = [(INF_ROW, 1.0, 1.0), (0, 1.0, -1.0), (4, 0.7, 0.25), (1, 1.0, 0.0)]
LISTS = {"mono1": MONO_ONE, "mono9": MONO_NINE, "stereo_inf_left": STEREO_INF_LEFT, "stereo_inf_right": STEREO_INF_RIGHT}
assert all(r != UNLISTED_ROW for inputs in LISTS.values() for r, _, _ in inputs)


def assert_mix_conditions(name, axc, nb, left, right, out):
    """what the planes are for, on any mixer's output: no NaN, Inf only in the channel INF_ROW feeds, the lone 0.0 input"""
    assert not np.isnan(left).any() and (right is None or not np.isnan(right).any()), f"{name}: something unread was read, or Inf met a 0"
    assert (right is None) == name.startswith("mono")
    if name == "stereo_inf_left":
        assert np.isinf(left).any() and np.isfinite(right).all(), "mult == 0 on the right skipped the Inf input"
    elif name == "stereo_inf_right":
        assert np.isinf(right).any() and np.isfinite(left).all(), "mult == 0 on the left skipped the Inf input"
    else:
        assert np.isfinite(left).all()
    if nb > SILENT_BATCH:
        assert out[SILENT_BATCH] == NO_SIGNAL and not left[SILENT_BATCH * WAVE_BATCH:(SILENT_BATCH + 1) * WAVE_BATCH].any()
    if name == "mono9" and nb > LONE_BATCH:  # INF_ROW alone, at ampfactor 0.0: a signal, and nothing added
        assert out[LONE_BATCH] == SIGNAL and not left[LONE_BATCH * WAVE_BATCH:(LONE_BATCH + 1) * WAVE_BATCH].any()
    assert (out[:nb] == np.where((axc[[r for r, _, _ in LISTS[name]], :nb] != NO_SIGNAL).any(axis=0), SIGNAL, NO_SIGNAL)).all()
