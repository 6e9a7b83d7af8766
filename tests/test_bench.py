"""bench.py's contract: --steps timed steps, ms_per_step in the line, a plain run without the --full extras, and
--dump-outputs writing the last timed step's outputs (float32, <= 64 MB, the same from run to run)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dumped(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_keeps_small_outputs_whole(tmp_path):
    bench = load_bench()
    audio = np.arange(2 * 3 * 4000, dtype=np.float32).reshape(2, 3, 4000)
    flags = np.full((2, 3, 2), 42, np.float32)
    bench.dump_outputs(str(tmp_path), {"audio": audio, "flags": flags})
    out = dumped(tmp_path)
    assert sorted(out) == ["audio", "flags"]
    assert np.array_equal(out["audio"], audio) and out["audio"].dtype == np.float32
    assert np.array_equal(out["flags"], flags)


def test_dump_samples_large_outputs_under_the_limit(tmp_path):
    bench = load_bench()
    rows, n = 80, 250000  # 80 MB of audio
    audio = np.broadcast_to(np.arange(rows, dtype=np.float32)[:, None], (rows, n)).reshape(8, 10, n)
    flags = np.zeros((8, 10, 125), np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"audio": audio, "flags": flags})
    a, b = dumped(tmp_path / "a"), dumped(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_LIMIT
    assert {k: v.dtype for k, v in a.items()} == {"audio": np.float32, "audio_rows": np.float64, "flags": np.float32}
    keep = a["audio_rows"].astype(np.int64)
    assert 0 < keep.size < rows and np.all(np.diff(keep) > 0)
    assert np.array_equal(a["audio"][:, 0], keep.astype(np.float32))  # row r holds the value r: the indices name the rows kept
    assert all(np.array_equal(a[k], b[k]) for k in a)                  # a fixed sample


def _bench(tmp_path, name, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--seconds", "2",
                        "--dump-outputs", str(tmp_path / name), *extra], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), dumped(tmp_path / name)


@pytest.mark.gpu
def test_bench_line_and_outputs_repeat(tmp_path):
    line, out = _bench(tmp_path, "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert {"metric", "value", "unit", "higher_is_better", "dtype"} <= set(line) and line["unit"] == "MS/s"
    assert "cpu_baseline" not in line and "config5" not in line  # --full only
    assert sorted(out) == ["audio", "flags"]
    assert out["audio"].dtype == np.float32 and out["audio"].shape == (1, 8, 16 * 2000)
    assert out["flags"].dtype == np.float32 and out["flags"].shape == (1, 8, 16)
    assert np.isfinite(out["audio"]).all() and (out["flags"] == ord("*")).any()
    _, again = _bench(tmp_path, "b")
    for k in out:
        assert np.array_equal(out[k].view(np.uint32), again[k].view(np.uint32)), k
