"""The yardstick of the output-gate tests: the reference's own skip rules, restated in numpy from src/output.cpp, one row and one
batch at a time with an `active` flag per row as output_t::active.  It does not call into the library.

  rule 1 (udp_stream, pulse)   output.cpp:568-570   skip when axcindicate == NO_SIGNAL
  rule 2 (file, rawfile)       output.cpp:518-520   skip when axcindicate == NO_SIGNAL and not active; :560 active = (axcindicate != NO_SIGNAL)
  rule 3 (continuous)          the same lines with continuous == true: never skipped
  rule 0                       the row has no output in this call: nothing is looked at, `active` included
"""
import numpy as np

WAVE_BATCH = 2000
NO_SIGNAL = ord(" ")
SYMBOLS = np.frombuffer(b"*<>", np.uint8)  # SIGNAL, AFC_UP, AFC_DOWN: all of them "not NO_SIGNAL"
SHAPES = [(1, 1), (1, 130), (3, 64), (3, 65), (65, 3), (1025, 3)]  # rows x batches
OPEN_PROBABILITIES = [0.0, 0.05, 0.5, 1.0]


def gate_model(rule, axc, active=None):
    """(index [k][2] of (row, batch) in travelling order, row_first [rows + 1], active after the call) for flags axc [rows][nbatches]"""
    rows, nbatches = axc.shape
    active = np.zeros(rows, bool) if active is None else np.array(active, dtype=bool)
    index, row_first = [], np.zeros(rows + 1, np.uint32)
    for r in range(rows):
        row_first[r] = len(index)
        if rule[r] == 0:
            continue
        for b in range(nbatches):
            signal = axc[r, b] != NO_SIGNAL
            if rule[r] == 1 and not signal:  # :568
                active[r] = signal
                continue
            if rule[r] == 2 and not signal and not active[r]:  # :518
                continue
            index.append((r, b))
            active[r] = signal  # :560
    row_first[rows] = len(index)
    return np.array(index, np.uint32).reshape(-1, 2), row_first, active.astype(np.uint8)


def draw_flags(rng, rows, nbatches, p_open):
    """axc [rows][nbatches]: a batch is open with probability p_open, an open one carries '*', '<' or '>'"""
    is_open = rng.random((rows, nbatches)) < p_open
    return np.where(is_open, SYMBOLS[rng.integers(0, 3, (rows, nbatches))], np.uint8(NO_SIGNAL)).astype(np.uint8)


def draw_rules(rng, rows, kind):
    """kind 0..3: that rule on every row; "mixed": every rule somewhere (as far as there are rows)"""
    if kind != "mixed":
        return np.full(rows, kind, np.uint8)
    rule = rng.integers(0, 4, rows).astype(np.uint8)
    rule[:min(rows, 4)] = np.array([2, 1, 3, 0], np.uint8)[:min(rows, 4)]
    return rule


def bits(a):
    """float32 data compared as bit patterns (the gate only copies; NaN patterns included)"""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a
