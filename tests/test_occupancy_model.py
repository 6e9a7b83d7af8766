"""The channel finder without a GPU: mi_occupancy_plan_host against the numpy model of tests/occupancy_model.py as bytes, the model
against a brute-force statement of the definition, the capacity, the refusals, the exported symbols and the record sizes, and the
round trip candidate -> mi_survey_bin_range -> mi_plan_create."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import occupancy_model as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE = 120000000
NCELLS = [1, 2, 3, 5, 67, 257, 1000]
PERMILLES = [1, 250, 500, 1000, 0]  # 0 = the default
SENT = 0xA5


def dev_for(pkg, log2n, rate=2560000):
    return pkg.device_cfg(sample_rate=rate, centerfreq=CENTRE, fft_size_log=log2n)


def twin_equals_model(pkg, name, log2n, ncells, ns, permille, disabled):
    """the host twin into sentinel-filled, over-allocated outputs against the model: records as bytes, and the bytes nobody may write"""
    n = 1 << log2n
    mean, peak, cfg, cap = om.planes(name, n, ncells, ns)
    want_bins, want_cands, want_first, want_count = om.expected(name, n, ncells, ns, permille, disabled)
    enabled = None if disabled is None else [s != disabled for s in range(ns)]
    slots = (min(cap, ns * n // 2) if cap else ns * n // 2) + 3
    bins = np.frombuffer(bytearray([SENT]) * (om.BIN_DTYPE.itemsize * (ns * n + 2)), pkg.OCC_BIN_DTYPE)
    cands = np.frombuffer(bytearray([SENT]) * (om.CAND_DTYPE.itemsize * slots), pkg.OCC_CAND_DTYPE)
    _, _, first, count = pkg.occupancy_plan_host(dev_for(pkg, log2n), mean, peak, om.with_permille(cfg, permille), enabled, cap, bins, cands)
    what = f"builder {name}, fft {n}, {ncells} cells, {ns} streams, permille {permille}, disabled {disabled}"
    assert np.array_equal(count, want_count) and np.array_equal(first, want_first), f"{what}: counts {count} {first} vs {want_count} {want_first}"
    stored = int(want_count[1])
    assert cands[:stored].tobytes() == want_cands[:stored].tobytes(), f"{what}: candidates differ"
    assert (cands[stored:].view(np.uint8) == SENT).all(), f"{what}: written beyond the last stored candidate"
    for s in range(ns):
        got = bins[s * n:(s + 1) * n]
        if s == disabled:
            assert (got.view(np.uint8) == SENT).all(), f"{what}: a disabled stream's bin region was written"
        else:
            bad = np.flatnonzero(got.view(np.uint8).reshape(n, -1) != want_bins[s].view(np.uint8).reshape(n, -1))
            assert bad.size == 0, f"{what}: stream {s}: bin records differ, first at bin {bad[0] // 32}: {got[bad[0] // 32]} vs {want_bins[s][bad[0] // 32]}"
    assert (bins[ns * n:].view(np.uint8) == SENT).all(), f"{what}: written behind the last bin record"
    return want_count


@pytest.mark.parametrize("name", sorted(om.BUILDERS))
def test_host_twin_fft256(pkg, name):
    """every ncells x every floor_permille on three streams with stream 1 disabled; one stream with the permilles taken in turn"""
    for ncells in NCELLS:
        for permille in PERMILLES:
            twin_equals_model(pkg, name, 8, ncells, 3, permille, 1)
    for i, ncells in enumerate(NCELLS):
        twin_equals_model(pkg, name, 8, ncells, 1, PERMILLES[i % len(PERMILLES)], None)


@pytest.mark.parametrize("name", sorted(om.BUILDERS))
def test_host_twin_fft8192(pkg, name):
    """one stream at every ncells, the permilles taken in turn (each occurs); three streams with stream 0 disabled at 3 and 67 cells"""
    for i, ncells in enumerate(NCELLS):
        twin_equals_model(pkg, name, 13, ncells, 1, PERMILLES[(i + ord(name)) % len(PERMILLES)], None)
    twin_equals_model(pkg, name, 13, 3, 3, 250, 0)
    twin_equals_model(pkg, name, 13, 67, 3, 500, 0)


def test_builders_do_what_they_are_for():
    """the planes give the shapes of result their tests rely on (checked on the model alone, fft 256, 67 cells, defaults)"""
    n, ncells = 256, 67
    res = {name: om.expected(name, n, ncells, 1, 0) for name in om.BUILDERS}
    assert res["a"][3][0] >= 3
    assert res["b"][3][0] == 0 and np.array_equal(res["b"][0]["floor"][0], om.planes("b", n, ncells, 1)[0][0, 0])
    c_bins = res["c"][0][0]
    assert (c_bins["floor"].view(np.uint32) >> 8 == om.planes("c", n, ncells, 1)[0][0, 0].view(np.uint32) >> 8).all()
    assert (c_bins["active_cells"] > 0).all() and (c_bins["active_cells"] < ncells).all()
    d_bins = om.expected("d", n, 5, 1, 1)[0][0]
    assert (d_bins["floor"] == 0).any() and (d_bins["floor"] > 0).any() and (d_bins["threshold"] == 0).any()
    sub = om.planes("d", n, 1000, 1)[0]
    assert ((sub > 0) & (sub < np.finfo(np.float32).tiny)).any(), "no subnormal among the planes of (d)"
    e = res["e"]
    assert e[3][0] == 1 and e[1][0]["nbins"] == n and e[1][0]["lo_bin"] == n // 2 and e[1][0]["hi_bin"] == n // 2 - 1
    assert res["f"][3][0] == 0
    g = res["g"]
    assert g[3][0] == n // 2 and g[3][1] < g[3][0] and (g[1]["nbins"] == 1).all()
    h = res["h"][1]
    assert [(int(c["lo_bin"]), int(c["hi_bin"]), int(c["best_bin"])) for c in h] == \
        [(n // 2, n // 2 + 4, n // 2 + 2), (n - 2, 1, n - 2), (n // 2 - 3, n // 2 - 1, n // 2 - 2)]
    i_bins = res["i"][0][0]
    assert (i_bins[10]["first_cell"], i_bins[10]["last_cell"], i_bins[10]["runs"]) == (0, 0, 1)
    assert (i_bins[20]["first_cell"], i_bins[20]["last_cell"], i_bins[20]["runs"]) == (ncells - 1, ncells - 1, 1)
    assert (i_bins[30]["first_cell"], i_bins[30]["last_cell"], i_bins[30]["runs"]) == (1, ncells - 2, ncells // 2)
    assert (i_bins[40]["first_cell"], i_bins[40]["last_cell"], i_bins[40]["runs"]) == (0, ncells - 1, (ncells + 1) // 2)
    j = res["j"]
    m = ncells // 3
    assert j[0][0][100]["active_cells"] == m and j[0][0][102]["active_cells"] == m - 1
    assert [int(c["best_bin"]) for c in j[1]] == [100]


def brute_force(mean, peak, permille, ratio, min_cells):
    """the definition with Python lists and loops only: (per bin tuples, candidate tuples) of one stream"""
    ncells, n = mean.shape
    k = (ncells - 1) * permille // 1000
    bins = []
    for b in range(n):
        col = [mean[c, b] for c in range(ncells)]
        floor = sorted(col)[k]
        thr = np.float32(floor) * np.float32(ratio)
        act = [c for c in range(ncells) if col[c] > thr]
        runs = sum(1 for c in act if c - 1 not in act)
        bins.append((floor, thr, len(act), act[0] if act else om.NONE, act[-1] if act else om.NONE, runs,
                     max([col[c] for c in act], default=np.float32(0)), max([peak[c, b] for c in act], default=np.float32(0))))
    cands, p = [], 0
    occ = [bins[(q + n // 2) % n][2] >= min_cells for q in range(n)]
    while p < n:
        if not occ[p]:
            p += 1
            continue
        q = p
        while q < n and occ[q]:
            q += 1
        run = [(r + n // 2) % n for r in range(p, q)]
        best = max(run, key=lambda b: bins[b][6])  # max() keeps the first of equals: the lowest position
        cands.append((best, run[0], run[-1], len(run)) + bins[best][2:5] + bins[best][6:8])
        p = q
    return bins, cands


@pytest.mark.parametrize("name,ncells,permille", [("a", 67, 250), ("c", 257, 500), ("d", 5, 1), ("d", 67, 1000), ("h", 3, 250), ("i", 2, 0),
                                                  ("g", 1, 250), ("j", 67, 250), ("e", 2, 1000)])
def test_model_against_brute_force(name, ncells, permille):
    n = 256
    mean, peak, cfg, cap = om.planes(name, n, ncells, 1)
    bins, cands, first, count = om.finder(mean, peak, om.with_permille(cfg, permille), None, 0)
    pm, ratio, min_cells = om.settings(om.with_permille(cfg, permille))
    want_bins, want_cands = brute_force(mean[0], peak[0], pm, ratio, min_cells)
    for b in range(n):
        assert tuple(bins[0][b]) == want_bins[b], (b, bins[0][b], want_bins[b])
    got = [tuple(c)[1:] for c in cands]
    assert got == want_cands
    assert count[0] == len(want_cands) == first[1] and first[0] == 0


def test_one_cell_has_no_activity_above_ratio_one():
    """ncells = 1: the floor is the cell itself, so with a ratio above 1 nothing is active -- positive values; a zero is not above 0"""
    for name in ("a", "d", "i"):
        mean, peak, _, _ = om.planes(name, 256, 1, 1)
        bins, cands, _, count = om.finder(mean, peak, (0, 1.5, 0))
        assert np.array_equal(bins[0]["floor"], mean[0, 0]) and (bins[0]["active_cells"] == 0).all() and count[0] == 0 and cands.size == 0
        assert (bins[0]["first_cell"] == om.NONE).all() and (bins[0]["runs"] == 0).all() and (bins[0]["max_mean"] == 0).all()


def test_capacity(pkg):
    """builder (g) has N / 2 candidates a stream: with a smaller buffer count[0] > count[1] and nothing lies beyond count[1]; with
    max_candidates = 0 the buffer of nstreams * N / 2 holds them all"""
    want = twin_equals_model(pkg, "g", 8, 5, 3, 250, None)
    assert want[0] == 3 * 128 and want[1] == 3 * 64 - 3
    mean, peak, cfg, _ = om.planes("g", 256, 5, 3)
    _, cands, first, count = pkg.occupancy_plan_host(dev_for(pkg, 8), mean, peak, cfg)
    assert count[0] == count[1] == 3 * 128 == cands.size and list(first) == [0, 128, 256, 384]
    assert cands.tobytes() == om.finder(mean, peak, cfg)[1].tobytes()
    _, cands, _, count = pkg.occupancy_plan_host(dev_for(pkg, 8), mean, peak, cfg, max_candidates=1)
    assert list(count) == [384, 1] and cands.size == 1 and cands[0]["best_bin"] == 129


def test_record_sizes_and_symbols(pkg):
    assert C.sizeof(pkg.OccBin) == 32 == pkg.OCC_BIN_DTYPE.itemsize and C.sizeof(pkg.OccCandidate) == 40 == pkg.OCC_CAND_DTYPE.itemsize
    assert C.sizeof(pkg.OccCfg) == 12
    assert pkg.OCC_BIN_DTYPE == om.BIN_DTYPE and pkg.OCC_CAND_DTYPE == om.CAND_DTYPE
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_occupancy_")}
    assert declared == {"mi_occupancy_create", "mi_occupancy_destroy", "mi_occupancy_set_streams", "mi_occupancy_process_device",
                        "mi_occupancy_download", "mi_occupancy_set_timing", "mi_occupancy_last_launch_ms", "mi_occupancy_plan_host"}
    assert declared <= set(pkg.ABI_SYMBOLS)
    for s in declared:
        assert hasattr(pkg.lib(), s), s


def test_refusals(pkg):
    mean, peak, _, _ = om.planes("a", 256, 3, 1)
    dev = dev_for(pkg, 8)

    def refused(text, fn, code=None):
        with pytest.raises(pkg.MiError) as e:
            fn()
        assert e.value.code == (code or pkg.MI_ERR_INVALID) and text in str(e.value), str(e.value)

    refused("floor_permille", lambda: pkg.occupancy_plan_host(dev, mean, peak, (1001, 0.0, 0)))
    for ratio in (-1.0, float("inf"), float("nan")):
        refused("ratio", lambda: pkg.occupancy_plan_host(dev, mean, peak, (0, ratio, 0)))
    refused("no stream enabled", lambda: pkg.occupancy_plan_host(dev, mean, peak, enabled=[0]))
    for log2n in (7, 14):
        refused("fft_size", lambda: pkg.occupancy_plan_host(dev_for(pkg, log2n), mean, peak))
    refused("sample_rate", lambda: pkg.occupancy_plan_host(dev_for(pkg, 8, rate=16000), mean, peak))
    # create: bad arguments are refused before the device is looked for
    for kw in (dict(nstreams=0), dict(max_cells=0), dict(cfg=(1001, 0.0, 0)), dict(cfg=(0, -0.5, 0)), dict(cfg=(0, float("nan"), 0)),
               dict(max_cells=4, cfg=(0, 0.0, 5))):
        refused("", lambda: pkg.Occupancy(dev, **kw))
    refused("min_cells", lambda: pkg.Occupancy(dev, max_cells=4, cfg=(0, 0.0, 5)))
    refused("fft_size", lambda: pkg.Occupancy(dev_for(pkg, 14)))
    if pkg.device_count() < 1:
        refused("no HIP device: the channel finder runs on the GPU only", lambda: pkg.Occupancy(dev), pkg.MI_ERR_NO_DEVICE)
    else:
        pkg.Occupancy(dev, max_cells=4, cfg=(0, 0.0, 4)).close()
    L = pkg.lib()
    some = np.zeros(64, np.uint8).ctypes.data
    for rc in (L.mi_occupancy_set_streams(None, None), L.mi_occupancy_process_device(None, some, some, 1, some, some, some, some, None),
               L.mi_occupancy_download(None, None, some, some, some, some), L.mi_occupancy_set_timing(None, 1),
               L.mi_occupancy_last_launch_ms(None, some),
               L.mi_occupancy_plan_host(None, None, None, 1, some, some, 1, some, some, 0, some, some)):
        assert rc == pkg.MI_ERR_INVALID and L.mi_last_error() == b"NULL argument"
    L.mi_occupancy_destroy(None)


@pytest.mark.parametrize("rate", [2560000, 2500000])
@pytest.mark.parametrize("log2n", [8, 13])
def test_candidates_round_trip_into_a_plan(pkg, log2n, rate):
    """every candidate of builder (a): the lo_hz mi_survey_bin_range gives its best_bin, handed to mi_plan_create, comes back as that bin"""
    n = 1 << log2n
    dev = dev_for(pkg, log2n, rate)
    mean, peak, cfg, _ = om.planes("a", n, 67, 1)
    _, cands, _, count = pkg.occupancy_plan_host(dev, mean, peak, cfg)
    assert count[0] == count[1] >= 3
    freqs = [pkg.survey_bin_range(dev, int(b))[0] for b in cands["best_bin"]]
    p = pkg.Plan(dev, [pkg.channel_cfg(f) for f in freqs])
    assert [p.channel(i).bin for i in range(len(freqs))] == [int(b) for b in cands["best_bin"]]
    p.close()


def test_end_to_end_capture_on_the_models(pkg):
    """the capture tests/test_gpu_occupancy.py surveys on the device, through the two models alone: survey_model's planes (its float64
    mean rounded to float32) into the finder's model give exactly one candidate per carrier at the carrier's bin"""
    import survey_model as sv
    dev, u8, wpc, ncells = om.e2e_capture(pkg)
    mean, peak = sv.survey_model(dev, u8, wpc, ncells)
    bins, cands, first, count = om.finder(mean.astype(np.float32)[None], peak[None])
    print("candidates:", [(int(c["best_bin"]), int(c["lo_bin"]), int(c["hi_bin"]), int(c["active_cells"]), int(c["first_cell"])) for c in cands])
    om.e2e_check(cands, 1 << dev.fft_size_log, dev.sample_rate)
    twin = pkg.occupancy_plan_host(dev, mean.astype(np.float32)[None], peak[None])
    assert twin[1].tobytes() == cands.tobytes() and twin[0].tobytes() == bins.tobytes()
