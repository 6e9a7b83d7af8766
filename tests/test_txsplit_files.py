"""txfile_put and tx_file_suffix (host/output_adapters.cpp) without a GPU: a stand-alone program feeds txfile_put one batch at a
time; the files it leaves equal, byte for byte, the slices the model's records (tx_model.py) cut from the model's travelling blocks,
and what it reports as opened, closed and written is what the model says.  Nothing of the library is linked."""
import calendar
import os
import subprocess
import time

import numpy as np
import pytest

from tx_model import DEFAULT_CFG, NONE, SMALL_CFG, draw_family, tx_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITTEN, OPENED, CLOSED = 1, 2, 4
PAYLOAD = 48  # bytes a batch: the adapter does not look into them


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    host = os.path.join(ROOT, "boondock-airband_amd", "host")
    path = tmp_path_factory.mktemp("txsplit") / "txsplit_files"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Wextra", "-I", host, "-o", str(path),
                    os.path.join(ROOT, "tests", "txsplit_files_main.cpp"), os.path.join(host, "output_adapters.cpp")], check=True, capture_output=True, text=True)
    return str(path)


@pytest.mark.parametrize("family,cfg", [("bursts", DEFAULT_CFG), ("bursts", SMALL_CFG), ("p05", DEFAULT_CFG), ("p50", SMALL_CFG), ("p100", SMALL_CFG),
                                        ("p0", DEFAULT_CFG)])
def test_files_on_disk_are_the_model_s_slices(exe, tmp_path, family, cfg):
    rows, nb = 4, 130
    rng = np.random.default_rng([21, cfg[0], len(family)])
    axc = draw_family(family, rng, rows, nb)
    payload = rng.integers(0, 256, (rows, nb, PAYLOAD), dtype=np.uint8)
    axc.tofile(tmp_path / "axc.bin")
    payload.tofile(tmp_path / "payload.bin")
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, "run", str(rows), str(nb), *[str(x) for x in cfg], str(PAYLOAD), str(tmp_path / "axc.bin"), str(tmp_path / "payload.bin"), str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    records, row_first, state, file_of, closes = tx_model(axc, cfg=cfg)
    want_files = {}
    for row in range(rows):
        travelling = payload[row][file_of[row] > 0]  # the row's travelling blocks, what an MI_GATE_OPEN_TRAIL gate packs
        for rec in records[row_first[row]:row_first[row + 1]]:
            assert rec["row"] == row and rec["nblocks"] > 0, "one call from a fresh state: every file has blocks"
            want_files[f"row_{row}_tx_{rec['seq']}"] = travelling[rec["first_block"]:rec["first_block"] + rec["nblocks"]].tobytes()
    assert sorted(os.listdir(out)) == sorted(want_files)
    for name, want in want_files.items():
        assert (out / name).read_bytes() == want, name
    events = {(int(a), int(b)): int(m) for k, a, b, m in (l.split() for l in r.stdout.splitlines() if l.startswith("event"))}
    per_row = {int(a): [int(x) for x in rest] for k, a, *rest in (l.split() for l in r.stdout.splitlines() if l.startswith("row"))}
    want_events = {}
    for row, b in zip(*np.nonzero(file_of)):
        want_events[(int(row), int(b))] = WRITTEN
    for rec in records:
        want_events[(int(rec["row"]), int(rec["first_batch"]))] |= OPENED
    for row, b, _ in closes:
        want_events[(row, b)] = want_events.get((row, b), 0) | CLOSED
    assert events == want_events
    for row in range(rows):
        mine = records[row_first[row]:row_first[row + 1]]
        still_open = int(state[row]["open"])
        assert per_row[row] == [len(mine), int((mine["close_batch"] != NONE).sum()) + still_open, int((file_of[row] > 0).sum()), still_open]
    if family == "bursts":
        assert len(closes) > rows, "bursts close files"
    if family == "p100":
        assert any(m == WRITTEN | OPENED | CLOSED for m in events.values()), "a split at max closes one file and opens the next in one batch"
    if family == "p0":
        assert not want_files and not events


def test_suffix_is_gmtime_of_the_batch_s_own_second(exe):
    def suffix(epoch_us, batch, include_freq=0, freq=0):
        r = subprocess.run([exe, "suffix", str(epoch_us), str(batch), str(include_freq), str(freq)], capture_output=True, text=True, check=True)
        text, n = r.stdout.split()
        assert len(text) == int(n)
        return text

    def want(sec):
        return time.strftime("_%Y%m%d_%H%M%S", time.gmtime(sec))

    leap = calendar.timegm((2024, 2, 29, 23, 59, 59))
    for epoch in (0, 1, 951782399, leap, calendar.timegm((2026, 12, 31, 23, 59, 58)), 2**31 + 5):
        assert suffix(epoch * 10**6, 0) == want(epoch)
        assert suffix(epoch * 10**6, 7) == want(epoch), "7 batches are 0.875 s"
        assert suffix(epoch * 10**6, 8) == want(epoch + 1), "8 batches are one second"
        assert suffix(epoch * 10**6 + 125000, 7) == want(epoch + 1), "0.125 s + 7 batches reach the next second exactly"
        assert suffix(epoch * 10**6 + 124999, 7) == want(epoch)
        assert suffix(epoch * 10**6 + 999999, 28800 * 3) == want(epoch + 3 * 3600)
    assert suffix(leap * 10**6, 8) == "_20240301_000000"
    assert suffix(leap * 10**6, 8, 1, 118525000) == "_20240301_000000_118525000"
    assert suffix(0, 0, 1, 0) == "_19700101_000000_0"
