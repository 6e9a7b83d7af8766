"""The output gate's rule, pinned without a GPU: mi_gate_plan_host against the numpy restatement of src/output.cpp in gate_model.py
(index, row_first, counts and carried flags, bit for bit), the argument errors, the exported symbols, and the model itself against
what rawfile_put (host/output_adapters.cpp) writes batch by batch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gate_model import NO_SIGNAL, OPEN_PROBABILITIES, SHAPES, WAVE_BATCH, bits, draw_flags, draw_rules, gate_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"mi_outgate_create", "mi_outgate_destroy", "mi_outgate_set_rules", "mi_outgate_process_device", "mi_outgate_download",
               "mi_outgate_state_size", "mi_outgate_get_state", "mi_outgate_set_state", "mi_outgate_set_timing", "mi_outgate_last_launch_ms",
               "mi_gate_plan_host"}
RULE_KINDS = [0, 1, 2, 3, "mixed"]


def assert_plan_equals_model(pkg, rule, axc, carried, what):
    index, row_first, count, after = pkg.gate_plan_host(rule, axc, carried)
    want_index, want_first, want_after = gate_model(rule, axc, carried)
    assert np.array_equal(index, want_index), f"{what}: index"
    assert np.array_equal(row_first, want_first), f"{what}: row_first"
    assert count[0] == len(want_index) and count[1] == len(want_index), f"{what}: counts {count} vs {len(want_index)}"
    assert np.array_equal(after, want_after), f"{what}: carried flags"
    return index, after


@pytest.mark.parametrize("p_open", OPEN_PROBABILITIES)
@pytest.mark.parametrize("rows,nbatches", SHAPES)
def test_plan_host_equals_the_model(pkg, rows, nbatches, p_open):
    rng = np.random.default_rng([rows, nbatches, int(p_open * 100)])
    axc = draw_flags(rng, rows, nbatches, p_open)
    if 0 < p_open < 1 and rows * nbatches >= 64:
        assert (axc == NO_SIGNAL).any() and (axc != NO_SIGNAL).any()
    for kind in RULE_KINDS:
        rule = draw_rules(rng, rows, kind)
        for carried in (np.zeros(rows, np.uint8), rng.integers(0, 2, rows).astype(np.uint8)):
            assert_plan_equals_model(pkg, rule, axc, carried, f"{rows} x {nbatches}, p {p_open}, rule {kind}, carried {carried[:4]}")


def test_flags_of_every_kind_are_drawn():
    axc = draw_flags(np.random.default_rng(1), 3, 130, 0.5)
    assert set(np.unique(axc)) == {ord(" "), ord("*"), ord("<"), ord(">")}
    assert (draw_flags(np.random.default_rng(1), 3, 65, 0.0) == NO_SIGNAL).all()
    assert (draw_flags(np.random.default_rng(1), 3, 65, 1.0) != NO_SIGNAL).all()


@pytest.mark.parametrize("p_open", OPEN_PROBABILITIES)
@pytest.mark.parametrize("cuts", [(1, 64, 65), (65, 1, 64), (130,), (3, 127)])
def test_calls_of_unequal_length_concatenate_to_the_uncut_run(pkg, cuts, p_open):
    rows, total = 5, 130
    assert sum(cuts) == total
    rng = np.random.default_rng([7, int(p_open * 100)])
    axc = draw_flags(rng, rows, total, p_open)
    rule = draw_rules(rng, rows, "mixed")
    uncut, _, uncut_after = gate_model(rule, axc)
    carried, done, per_row = np.zeros(rows, np.uint8), 0, [[] for _ in range(rows)]
    for n in cuts:
        index, carried = assert_plan_equals_model(pkg, rule, np.ascontiguousarray(axc[:, done:done + n]), carried, f"cuts {cuts}, call at {done}")
        for r, b in index:
            per_row[r].append(int(b) + done)
        done += n
    for r in range(rows):
        assert per_row[r] == [int(b) for rr, b in uncut if rr == r], f"cuts {cuts}: row {r}"
    assert np.array_equal(carried, uncut_after)


def test_a_row_under_rule_0_keeps_its_carried_flag(pkg):
    """Two rows under the file rule; row 0 sits the second call out (rule 0).  Its last batch before was open and its first batch after
    is closed: that batch is the trailing one and still travels."""
    star, off = ord("*"), NO_SIGNAL
    first = np.array([[off, star], [off, star]], np.uint8)
    second = np.array([[star, star], [off, off]], np.uint8)  # (row 0's flags here belong to nobody: they must not be looked at)
    third = np.array([[off, off], [off, off]], np.uint8)
    _, _, _, carried = pkg.gate_plan_host([2, 2], first)
    assert list(carried) == [1, 1]
    index, row_first, count, carried = pkg.gate_plan_host([0, 2], second, carried)
    assert [tuple(x) for x in index] == [(1, 0)] and list(row_first) == [0, 0, 1] and count[0] == 1
    assert list(carried) == [1, 0], "rule 0 leaves the flag as it was"
    index, _, _, carried = pkg.gate_plan_host([2, 2], third, carried)
    assert [tuple(x) for x in index] == [(0, 0)], "the closed batch after the pause is row 0's trailing batch"
    assert list(carried) == [0, 0]
    want, _, want_after = gate_model([2, 2], third, [1, 0])
    assert np.array_equal(index, want) and np.array_equal(carried, want_after)


def test_argument_errors(pkg):
    f = pkg.lib().mi_gate_plan_host
    rows, nb = 2, 3
    axc = np.full((rows, nb), ord("*"), np.uint8)
    carried = np.zeros(rows, np.uint8)
    index = np.zeros((rows * nb, 2), np.uint32)
    row_first = np.zeros(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(rule, nbatches=nb, drop=None):
        args = [p(np.array(rule, np.uint8)), rows, p(axc), nb, nbatches, p(carried), p(index), p(row_first), p(count)]
        if drop is not None:
            args[drop] = None
        return f(*args)

    assert call([1, 2]) == pkg.MI_OK
    assert call([1, 4]) == pkg.MI_ERR_INVALID
    assert b"rule" in pkg.lib().mi_last_error()
    assert call([255, 0]) == pkg.MI_ERR_INVALID
    assert call([1, 2], nbatches=0) == pkg.MI_ERR_INVALID
    assert call([1, 2], nbatches=-1) == pkg.MI_ERR_INVALID
    assert call([1, 2], nbatches=nb + 1) == pkg.MI_ERR_INVALID, "a call longer than the flag stride"
    for drop in (0, 2, 5, 6, 7, 8):
        assert call([1, 2], drop=drop) == pkg.MI_ERR_INVALID, f"NULL argument {drop}"
    with pytest.raises(pkg.MiError):
        pkg.gate_plan_host([1, 7], axc)


def test_library_exports_the_gate_s_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    gate = {s for s in declared if s.startswith("mi_outgate_") or s.startswith("mi_gate_")}
    assert gate == NEW_SYMBOLS
    lib = pkg.lib()
    missing = [s for s in sorted(gate) if not hasattr(lib, s)]
    assert not missing, f"declared in include/mi_airband.h but not exported: {missing}"
    assert gate <= set(pkg.ABI_SYMBOLS)
    assert C.sizeof(pkg.GateBlock) == 8
    assert (pkg.GATE_NONE, pkg.GATE_OPEN, pkg.GATE_OPEN_TRAIL, pkg.GATE_ALL) == (0, 1, 2, 3)
    for name, value in (("MI_GATE_NONE", 0), ("MI_GATE_OPEN", 1), ("MI_GATE_OPEN_TRAIL", 2), ("MI_GATE_ALL", 3)):
        assert re.search(rf"\b{name} = {value}\b", header)


@pytest.mark.parametrize("p_open", [0.05, 0.5])
def test_model_under_the_file_rule_equals_rawfile_put(tmp_path, p_open):
    """What the model lets travel under rule 2, block after block, is the byte stream a non-continuous rawfile output gets from
    rawfile_put called batch by batch (a stand-alone program over host/output_adapters.cpp; nothing of the library is linked)."""
    host = os.path.join(ROOT, "boondock-airband_amd", "host")
    exe = tmp_path / "outgate_rawfile"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-I", host, "-o", str(exe), os.path.join(ROOT, "tests", "outgate_rawfile_main.cpp"),
                    os.path.join(host, "output_adapters.cpp")], check=True, capture_output=True, text=True)
    rows, nb = 3, 65
    rng = np.random.default_rng([11, int(p_open * 100)])
    axc = draw_flags(rng, rows, nb, p_open)
    axc[0, :3] = [ord("*"), NO_SIGNAL, NO_SIGNAL]  # a trailing batch, then a skipped one, whatever was drawn
    iq = rng.integers(0, 2**32, (rows, nb, 2 * WAVE_BATCH), dtype=np.uint32).view(np.float32)
    axc.tofile(tmp_path / "axc.bin")
    iq.tofile(tmp_path / "iq.bin")
    r = subprocess.run([str(exe), str(rows), str(nb), str(tmp_path / "axc.bin"), str(tmp_path / "iq.bin"), str(tmp_path)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stderr
    index, row_first, _ = gate_model(np.full(rows, 2, np.uint8), axc)
    assert (0, 1) in {tuple(x) for x in index} and (0, 2) not in {tuple(x) for x in index}
    for row in range(rows):
        mine = index[row_first[row]:row_first[row + 1]]
        assert (mine[:, 0] == row).all()
        want = np.concatenate([iq[row, b] for b in mine[:, 1]]) if len(mine) else np.zeros(0, np.float32)
        got = np.fromfile(tmp_path / f"row_{row}.cf32", np.float32)
        assert got.size == want.size, f"row {row}: {got.size // (2 * WAVE_BATCH)} batches written, the model lets {len(mine)} travel"
        assert np.array_equal(bits(got), bits(want)), f"row {row}: byte stream"
