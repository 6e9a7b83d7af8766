"""Reference model of the channel finder (mi_occupancy_*, csrc/occupancy.hip; definition in include/mi_airband.h "channel finder") and the
planes its tests share.  Plain numpy, written from the definition and not from the code under test:
  floor      np.sort(mean over the cells)[k], k = (ncells - 1) * floor_permille // 1000
  threshold  floor * ratio in float32
  active     mean > threshold, float comparisons
  runs, first, last, the maxima over the active cells; then, per stream, the maximal runs of occupied positions p = (bin + N / 2) % N.
The device and the host twin must equal what `finder` returns byte for byte.  The records are numpy structured arrays with the ABI's
layouts (32 and 40 bytes), spelled out here on their own.

The plane builders are seeded, float32 and non-negative; each exists to break one part of a kernel (see `BUILDERS`)."""
import functools

import numpy as np

BIN_DTYPE = np.dtype([("floor", "<f4"), ("threshold", "<f4"), ("active_cells", "<u4"), ("first_cell", "<u4"), ("last_cell", "<u4"), ("runs", "<u4"),
                      ("max_mean", "<f4"), ("max_peak", "<f4")])
CAND_DTYPE = np.dtype([("stream", "<u4"), ("best_bin", "<u4"), ("lo_bin", "<u4"), ("hi_bin", "<u4"), ("nbins", "<u4"), ("active_cells", "<u4"),
                       ("first_cell", "<u4"), ("last_cell", "<u4"), ("max_mean", "<f4"), ("max_peak", "<f4")])
assert BIN_DTYPE.itemsize == 32 and CAND_DTYPE.itemsize == 40
NONE = 0xFFFFFFFF
DEFAULTS = (250, 3.0, 1)  # floor_permille, ratio, min_cells: what a 0 field means


def settings(cfg):
    """(floor_permille, ratio float32, min_cells) with the defaults filled in; cfg: None or a triple whose zeros mean the default"""
    cfg = cfg or (0, 0.0, 0)
    return int(cfg[0]) or DEFAULTS[0], np.float32(cfg[1] if cfg[1] else DEFAULTS[1]), int(cfg[2]) or DEFAULTS[2]


def bin_records(mean, peak, permille, ratio):
    """BIN_DTYPE [N] of one stream: mean, peak float32 [ncells][N]"""
    assert mean.dtype == np.float32 and peak.dtype == np.float32 and mean.shape == peak.shape
    ncells, n = mean.shape
    k = (ncells - 1) * permille // 1000
    out = np.zeros(n, BIN_DTYPE)
    out["floor"] = np.sort(mean, axis=0)[k]
    out["threshold"] = out["floor"] * np.float32(ratio)
    assert out["threshold"].dtype == np.float32
    active = mean > out["threshold"][None, :]
    out["active_cells"] = active.sum(axis=0)
    some = active.any(axis=0)
    out["first_cell"] = np.where(some, active.argmax(axis=0), NONE)
    out["last_cell"] = np.where(some, ncells - 1 - active[::-1].argmax(axis=0), NONE)
    before = np.vstack([np.zeros((1, n), bool), active[:-1]])
    out["runs"] = (active & ~before).sum(axis=0)
    out["max_mean"] = np.where(active, mean, np.float32(0)).max(axis=0)
    out["max_peak"] = np.where(active, peak, np.float32(0)).max(axis=0)
    return out


def candidates(stream, bins, min_cells):
    """the CAND_DTYPE records of one stream, positions ascending: a Python walk over the positions"""
    n = bins.size
    cells, top = bins["active_cells"].tolist(), bins["max_mean"]
    out = []
    p = 0
    while p < n:
        if cells[(p + n // 2) % n] < min_cells:
            p += 1
            continue
        q = p
        best = (p + n // 2) % n
        while q < n and cells[(q + n // 2) % n] >= min_cells:
            b = (q + n // 2) % n
            if top[b] > top[best]:  # ties stay with the lowest position
                best = b
            q += 1
        r = bins[best]
        out.append((stream, best, (p + n // 2) % n, (q - 1 + n // 2) % n, q - p, r["active_cells"], r["first_cell"], r["last_cell"], r["max_mean"],
                    r["max_peak"]))
        p = q
    return np.array(out, CAND_DTYPE)


def finder(mean, peak, cfg=None, enabled=None, max_candidates=0):
    """mean, peak float32 [nstreams][ncells][N] -> (bins [nstreams][N] -- zeros for a disabled stream, whose region nobody writes --,
    all candidates found, stream_first [nstreams + 1], count [2]).  The stored candidates are the first count[1] of those found."""
    permille, ratio, min_cells = settings(cfg)
    ns, _, n = mean.shape
    bins = np.zeros((ns, n), BIN_DTYPE)
    found, first = [], np.zeros(ns + 1, np.uint32)
    total = 0
    for s in range(ns):
        first[s] = total
        if enabled is not None and not enabled[s]:
            continue
        bins[s] = bin_records(mean[s], peak[s], permille, ratio)
        c = candidates(s, bins[s], min_cells)
        found.append(c)
        total += c.size
    first[ns] = total
    cap = min(max_candidates, ns * n // 2) if max_candidates else ns * n // 2
    cands = np.concatenate(found) if found else np.zeros(0, CAND_DTYPE)
    return bins, cands, first, np.array([total, min(total, cap)], np.uint32)


# ------------------------------------------------------------------ planes

def _noise(rng, ns, ncells, n):
    """mean around 1 within 10 %, peak 1.5 .. 3 times the mean"""
    mean = rng.uniform(0.9, 1.1, (ns, ncells, n)).astype(np.float32)
    peak = (mean * rng.uniform(1.5, 3.0, mean.shape).astype(np.float32)).astype(np.float32)
    return mean, peak


def _late(ncells):
    """the cells a builder raises: the last third, at least one -- above any floor up to the median"""
    return slice(ncells - max(1, ncells // 3), ncells)


def build_a(rng, ns, ncells, n):
    """(a) noise-like columns with a few raised stretches of bins x cells"""
    mean, peak = _noise(rng, ns, ncells, n)
    for s in range(ns):
        for _ in range(6):
            b0, width = int(rng.integers(0, n)), int(rng.integers(1, 14))
            c0 = int(rng.integers(0, ncells))
            c1 = min(ncells, c0 + 1 + int(rng.integers(0, max(1, ncells // 4))))
            gain = np.float32(rng.uniform(5, 40))
            for b in range(b0, b0 + width):
                mean[s, c0:c1, b % n] *= gain
                peak[s, c0:c1, b % n] *= gain
    return mean, peak, None, 0


def build_b(rng, ns, ncells, n):
    """(b) all cells of a bin equal: the selection runs among ties, and nothing is above floor x 3"""
    col = rng.uniform(0.5, 2.0, (ns, 1, n)).astype(np.float32)
    mean = np.repeat(col, ncells, axis=1)
    return mean, (mean * np.float32(2)).astype(np.float32), None, 0


def build_c(rng, ns, ncells, n):
    """(c) a column's values differ in the low 8 mantissa bits only, so the last radix round decides; ratio 1.0 makes every cell above
    the exact floor active, so a floor that is off by one value changes the counts"""
    base = np.uint32(0x3FC00000) + (rng.integers(0, 1 << 15, (ns, 1, n)).astype(np.uint32) << np.uint32(8))
    bits = base + rng.integers(0, 256, (ns, ncells, n)).astype(np.uint32)
    mean = bits.view(np.float32)
    return np.ascontiguousarray(mean), (mean * np.float32(1.5)).astype(np.float32), (0, 1.0, 0), 0


def build_d(rng, ns, ncells, n):
    """(d) bit patterns spread evenly from 0.0 and the subnormals up to 1e6, zeros in up to half of a column's cells: floor and threshold
    can be 0, and every radix round sees every digit"""
    top = int(np.float32(1e6).view(np.uint32))
    bits = rng.integers(0, top + 1, (ns, ncells, n)).astype(np.uint32)
    zero = rng.random((ns, ncells, n)) < rng.uniform(0, 0.5, (ns, 1, n))
    bits[zero] = 0
    mean = bits.view(np.float32)
    peak = np.maximum(mean, rng.integers(0, top + 1, mean.shape).astype(np.uint32).view(np.float32))
    return np.ascontiguousarray(mean), np.ascontiguousarray(peak), None, 0


def build_e(rng, ns, ncells, n):
    """(e) every bin occupied (ratio 0.5 under positive noise): one candidate of N bins per stream"""
    mean, peak = _noise(rng, ns, ncells, n)
    return mean, peak, (0, 0.5, 0), 0


def build_f(rng, ns, ncells, n):
    """(f) no bin occupied: noise within 10 % under ratio 3"""
    mean, peak = _noise(rng, ns, ncells, n)
    return mean, peak, None, 0


def build_g(rng, ns, ncells, n):
    """(g) occupied positions alternating -- all-zero columns at the even positions, ratio 0.5 -- which gives N / 2 candidates a stream,
    the maximum; max_candidates is set to under half of that, below the count even where one of three streams sits out"""
    mean, peak = _noise(rng, ns, ncells, n)
    even = (np.arange(n) + n // 2) % n % 2 == 0  # by bin: the position is even
    mean[:, :, even] = 0
    return mean, peak, (0, 0.5, 0), ns * n // 4 - 3


def build_h(rng, ns, ncells, n):
    """(h) a run from position 0, a run ending at position N - 1, a run across bins N - 1 | 0; two bins of a run with equal max_mean"""
    mean = np.ones((ns, ncells, n), np.float32)
    late = _late(ncells)

    def raise_at(s, p, v):
        mean[s, late, (p + n // 2) % n] = v

    for s in range(ns):
        for p, v in zip(range(0, 5), (5, 6, 7 + s, 6, 5)):
            raise_at(s, p, v)
        for p, v in zip(range(n - 3, n), (5, 9, 9)):  # the tie: position N - 2 is the best bin
            raise_at(s, p, v)
        for p, v in zip(range(n // 2 - 2, n // 2 + 2), (8, 8, 4, 4)):  # bins N - 2, N - 1, 0, 1; the tie: bin N - 2
            raise_at(s, p, v)
    return mean, (mean * np.float32(2)).astype(np.float32), None, 0


def build_i(rng, ns, ncells, n):
    """(i) activity on the first cell only, on the last only, and on alternating cells (the odd ones, or the even ones where that ends
    on the last cell too): runs is exercised and first / last sit at the ends"""
    mean, peak = _noise(rng, ns, ncells, n)
    for s in range(ns):
        mean[s, 0, 10 + s] = 50
        mean[s, ncells - 1, 20 + s] = 60
        mean[s, 1::2, 30 + s] = 70
        mean[s, (ncells - 1) % 2::2, 40 + s] = 80  # ends on the last cell
        peak[s] = np.maximum(peak[s], mean[s] * np.float32(1.25))
    return mean, peak, None, 0


def build_j(rng, ns, ncells, n):
    """(j) min_cells = m: one bin with exactly m active cells (occupied), its neighbour but one with m - 1 (not)"""
    mean, peak = _noise(rng, ns, ncells, n)
    m = max(1, ncells // 3)
    for s in range(ns):
        mean[s, ncells - m:, 100 + s] = 30
        mean[s, ncells - m + 1:, 102 + s] = 30
    return mean, peak, (0, 0.0, m), 0


BUILDERS = dict(a=build_a, b=build_b, c=build_c, d=build_d, e=build_e, f=build_f, g=build_g, h=build_h, i=build_i, j=build_j)


@functools.lru_cache(maxsize=6)
def planes(name, n, ncells, ns, seed=0):
    """(mean, peak, cfg, max_candidates) of builder `name`, read-only: shared between the tests that need them"""
    rng = np.random.default_rng([ord(name), n, ncells, ns, seed])
    mean, peak, cfg, cap = BUILDERS[name](rng, ns, ncells, n)
    assert mean.dtype == np.float32 and peak.dtype == np.float32 and mean.shape == (ns, ncells, n) == peak.shape
    assert np.isfinite(mean).all() and np.isfinite(peak).all() and not np.signbit(mean).any() and not np.signbit(peak).any()
    mean.setflags(write=False)
    peak.setflags(write=False)
    return mean, peak, cfg, cap


def with_permille(cfg, permille):
    cfg = cfg or (0, 0.0, 0)
    return (permille, cfg[1], cfg[2])


@functools.lru_cache(maxsize=512)
def expected(name, n, ncells, ns, permille, disabled=None):
    """the model's answer for builder `name` with floor_permille set (0 = the default) and stream `disabled` sitting out"""
    mean, peak, cfg, cap = planes(name, n, ncells, ns)
    enabled = None if disabled is None else [s != disabled for s in range(ns)]
    return finder(mean, peak, with_permille(cfg, permille), enabled, cap)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the end-to-end capture

E2E_RATE, E2E_LOG2N, E2E_WPC, E2E_CELLS = 2560000, 9, 200, 16
# (offset from the centre in Hz, gate phase): bins of 5000 Hz, so -140.0, -90.2, 5.0 and 180.2 bins -- each at least 0.2 bin from a
# half-bin boundary and at least 20 bins from the next.  The gate turns every four cells: phase 0 is on in cells 4 .. 7 and 12 .. 15,
# phase 1 in cells 0 .. 3 and 8 .. 11, so every carrier's bins are quiet in half of the cells and the floor is the noise's.
E2E_CARRIERS = [(-700000, 0), (-451000, 1), (25000, 1), (901000, 0)]


def e2e_capture(pkg):
    """(dev, u8 capture exactly as long as the survey reads, windows per cell, cells): sigma = 2 LSB noise and four 12 LSB carriers"""
    import survey_model as sv
    dev = pkg.device_cfg(sample_rate=E2E_RATE, centerfreq=sv.CENTRE, fft_size_log=E2E_LOG2N)
    hop = sv.hop_samples(E2E_RATE)
    u8 = sv.noise_and_carriers(pkg, E2E_RATE, sv.samples_needed(dev, E2E_WPC * E2E_CELLS), E2E_CARRIERS, gate_samples=4 * E2E_WPC * hop)
    return dev, u8, E2E_WPC, E2E_CELLS


def e2e_check(cands, n, rate):
    """one candidate per carrier, in frequency order, each best_bin within one position of round(offset / (rate / N)); a carrier is seen
    in the cells its gate is on, give or take the cells a gate edge cuts"""
    assert len(cands) == len(E2E_CARRIERS), f"{len(cands)} candidates for {len(E2E_CARRIERS)} carriers"
    for c, (off, phase) in zip(cands, sorted(E2E_CARRIERS)):
        want = (round(off / (rate / n)) + n // 2) % n  # as a position
        got = (int(c["best_bin"]) + n // 2) % n
        assert abs(got - want) <= 1, f"carrier at {off} Hz: best_bin at position {got}, expected {want}"
        assert 7 <= c["active_cells"] <= 9 and c["first_cell"] in ((0,) if phase else (3, 4))
