"""The audio spectrum stage without a GPU: the window and the band, the host twin mi_aspec_plan_host against the numpy restatement in
aspec_model.py byte for byte, that restatement's spectrum against a float64 FFT, and the vote mi_aspec_notch_host at its thresholds
and on the builders."""
import math

import numpy as np
import pytest

import aspec_model as am
import pcm_model as pm
from aspec_model import BINS, HZ_PER_BIN, NONE, WAVE_BATCH, aspec_model, audio, notch_model

SENT = np.float32(-7.25)
NOTCH_FIELDS = ("found", "bin", "freq_hz", "peak", "floor", "votes", "blocks")


def same(a, b, what):
    for name, x, y in zip(("records", "power", "mean", "row counts"), a, b):
        assert (x is None) == (y is None) and (x is None or x.tobytes() == y.tobytes()), f"{what}: {name}"


def vote_pair(pkg, mean, blocks, records=None, **kw):
    """the library's vote as a tuple, checked against the model's"""
    v = pkg.aspec_notch_host(mean, blocks, records, **kw)
    got = tuple(getattr(v, f) for f in NOTCH_FIELDS)
    want = notch_model(mean, blocks, () if records is None else records, **kw)
    assert got == tuple(want[f] for f in NOTCH_FIELDS), (got, want)
    return v


def test_window(pkg):
    w = pkg.aspec_window()
    assert w.dtype == np.float32 and w.shape == (WAVE_BATCH,)
    assert w.tobytes() == w[::-1].tobytes(), "the window is symmetric bit for bit"
    assert w.tobytes() == am.window().tobytes()
    exact = am.window64()
    assert (np.abs(w.astype(np.float64) - exact) <= np.spacing(np.maximum(exact, 2.0 ** -126).astype(np.float32))).all(), "within one float32 step of the formula"
    assert w[0] == 0.0 and w[999] == w[1000] and 0.99999 < w[999] < 1.0 and (np.diff(w[:1000]) > 0).all()


def test_band_defaults(pkg):
    assert pkg.aspec_band() == am.band() == (8, 486) and pkg.aspec_band(60, 3800) == (8, 486)
    for lo_hz, hi_hz in ((300, 3000), (1, 8), (60, 7999), (63, 0), (0, 63), (3796, 3800)):
        assert pkg.aspec_band(lo_hz, hi_hz) == am.band(lo_hz, hi_hz), (lo_hz, hi_hz)
    for lo_hz, hi_hz in ((3797, 3800), (60, 8000), (0, 62), (4000, 0)):
        assert am.band(lo_hz, hi_hz) is None
        with pytest.raises(pkg.MiError) as e:
            pkg.aspec_band(lo_hz, hi_hz)
        assert e.value.code == pkg.MI_ERR_INVALID


@pytest.mark.parametrize("rows,nb", [(1, 1), (1, 4), (5, 1), (5, 4)])
def test_twin_equals_model_on_every_builder(pkg, rows, nb):
    """records, power rows, row means and row counts as bytes, over the index MI_GATE_ALL would pack"""
    index, first = am.full_index(rows, nb)
    for name in am.BUILDERS:
        wave = audio(name, rows, nb)
        want = aspec_model(wave, index, first)
        same(pkg.aspec_plan_host(rows, wave, index, first), want, f"{name}, {rows} x {nb}")
        assert (want[3] == nb).all() and (want[0]["peak_bin"] >= 8).all() and (want[0]["peak_bin"] <= 486).all()
        assert (want[0]["line_power"] <= want[0]["band_power"] * (1 + 1e-12)).all() and (want[0]["peak_power"] <= want[0]["line_power"]).all()


def test_what_the_builders_are_for():
    rows, nb = 2, 2
    index, first = am.full_index(rows, nb)
    rec = {name: aspec_model(audio(name, rows, nb), index, first) for name in am.BUILDERS}
    for name in ("silence", "subnormal"):
        assert not rec[name][1].any() and (rec[name][0]["peak_bin"] == 8).all() and not rec[name][0]["band_power"].any(), name
    p = rec["constant"][1]
    assert (p[:, :3].sum(axis=1) > 1e6 * p[:, 8:].sum(axis=1)).all(), "a constant's energy lies below the band"
    assert (rec["tone_on_bin"][0]["peak_bin"] == 128).all() and np.isin(rec["tone_between"][0]["peak_bin"], (128, 129)).all()
    for name, b in (("tone_lo", 8), ("tone_lo1", 9), ("tone_hi", 486)):
        r, p = rec[name][0], rec[name][1].astype(np.float64)
        assert (r["peak_bin"] == b).all(), name
        lo, hi = max(8, b - 2), min(486, b + 2)
        assert hi - lo < 4, "the line sum is clipped"
        want = np.zeros(len(r))
        for j in range(lo, hi + 1):
            want = want + p[:, j]
        assert (r["line_power"] == want).all(), name
    r, p = rec["outside_strong"][0], rec["outside_strong"][1]
    assert (r["peak_bin"] == am.INSIDE_BIN).all() and (p[:, am.OUTSIDE_BIN] > 1000 * r["peak_power"]).all(), "the weak tone inside the band is chosen"
    assert (rec["square"][0]["peak_power"] > rec["tone_on_bin"][0]["peak_power"]).all()  # full scale against 0.5


def test_unsorted_repeated_and_out_of_range_entries_into_sentinel_filled_outputs(pkg):
    """the twin takes the index in any order with repeats, cuts the rows by row_first alone, writes every record and every row and
    nothing else; entries that are not of the call give the empty record and a zero row, and nothing out of range is read"""
    import ctypes as C
    rows, nb = 5, 4
    wave = audio("noise", rows, nb)
    idx = np.array([[4, 3], [0, 0], [4, 3], [rows, 0], [2, 1], [1, nb], [0, 3], [0xFFFFFFFF, 0], [3, 2], [0, 0]], np.uint32)
    first = np.array([0, 3, 3, 4, 20, 10], np.uint32)  # row 1 has no block; row 3 runs past the end; row 4's start lies behind its end
    want = aspec_model(wave, idx, first)
    assert (want[0]["peak_bin"][[3, 5, 7]] == NONE).all() and not want[1][[3, 5, 7]].any() and want[0][0] == want[0][2] and want[0][1] == want[0][9]
    assert want[3].tolist() == [3, 0, 1, 6, 0] and not want[2][1].any() and not want[2][4].any()
    k = len(idx)
    rec = np.full(k + 1, SENT, np.float32).repeat(8).view(pkg.ASPEC_RECORD_DTYPE)
    power, mean, blocks = np.full((k + 1, BINS), SENT), np.full((rows + 1, BINS), SENT), np.full(rows + 1, 0xA5A5A5A5, np.uint32)
    sent_rec = rec[k:].tobytes()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # the audio lies in a buffer with nothing around it but the padding of the stride, filled with NaN: reading it would show
    padded = np.full((rows, nb * WAVE_BATCH + 8), np.nan, np.float32)
    padded[:, :nb * WAVE_BATCH] = wave
    assert pkg.lib().mi_aspec_plan_host(None, rows, nb, ptr(padded), padded.shape[1], ptr(idx), k, ptr(first), ptr(rec), ptr(power), ptr(mean), ptr(blocks)) == 0
    same((rec[:k], power[:k], mean[:rows], blocks[:rows]), want, "sentinel-filled outputs")
    assert rec[k:].tobytes() == sent_rec and (power[k] == SENT).all() and (mean[rows] == SENT).all() and blocks[rows] == 0xA5A5A5A5
    assert np.isfinite(power[:k]).all()
    # without the power rows and the row mean the records are the same
    rec2, none, mean2, blocks2 = pkg.aspec_plan_host(rows, wave, idx, None, want_power=False)
    assert rec2.tobytes() == want[0].tobytes() and none is None and mean2 is None and blocks2 is None


@pytest.mark.parametrize("lo_hz,hi_hz", [(0, 0), (300, 3000)])
@pytest.mark.parametrize("case", pm.FOREIGN_CASES)
def test_twin_equals_model_on_the_foreign_index(pkg, case, lo_hz, hi_hz):
    """pcm_model.foreign_index -- 20 or 24 entries for a call whose grid is 6, zero entries of every kind before, between and behind
    valid ones, a row_first that is not a gate's -- over the thirteen builders, three rows at a time, the input laid out for the
    handle's 8 batches: the twin through the C entry point into sentinel-filled outputs with a guard behind the capacity writes
    exactly min(count[1], max_blocks) records and power rows, and the row means over the slices as `stored` cuts them."""
    import ctypes as C
    rows, nb, mb = pm.FOREIGN_SHAPE
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    cfg = pkg.AspecCfg(lo_hz, hi_hz)
    guard = 2
    for group in range(am.FOREIGN_GROUPS):
        wave, index, count, row_first, cap, stored, want = am.foreign_reference(case, group, lo_hz, hi_hz)
        kinds = pm.foreign_kinds(index[:stored], rows, nb, mb)
        what = f"{case}, group {group}, band {lo_hz} .. {hi_hz}"
        # what the model says about the index, before anything is compared with it
        assert [int(b) == NONE for b in want[0]["peak_bin"]] == [k != "V" for k in kinds], what
        assert not want[1][[k != "V" for k in kinds]].any() and want[3].tolist() == [0, stored - 2, 0], what
        assert want[0]["row"].tolist() == index[:stored, 0].tolist() and want[0]["batch"].tolist() == index[:stored, 1].tolist()
        twice = [k for k in range(stored) if tuple(index[k]) == (2, 1)]
        assert len(twice) >= 2 and all(want[0][k] == want[0][twice[0]] and want[1][k].tobytes() == want[1][twice[0]].tobytes() for k in twice)
        as_handle = aspec_model(wave, index[[k for k in range(stored) if kinds[k] in "BD"]], None, lo_hz, hi_hz, nbatches=mb)
        assert (as_handle[0]["peak_bin"] != NONE).all() and as_handle[1].any(axis=1).all(), "a batch behind the call holds audio: reading it would show"
        rec = np.full(cap + guard, SENT, np.float32).repeat(8).view(pkg.ASPEC_RECORD_DTYPE)
        power, mean, blocks = np.full((cap + guard, BINS), SENT), np.full((rows + 1, BINS), SENT), np.full(rows + 1, 0xA5A5A5A5, np.uint32)
        sent_rec = rec[stored:].tobytes()
        n = pm.stored_blocks(count, cap)
        assert pkg.lib().mi_aspec_plan_host(C.byref(cfg), rows, nb, ptr(wave), wave.shape[1], ptr(index), n, ptr(row_first), ptr(rec), ptr(power), ptr(mean),
                                            ptr(blocks)) == 0
        same((rec[:stored], power[:stored], mean[:rows], blocks[:rows]), want, what)
        assert rec[stored:].tobytes() == sent_rec and (power[stored:] == SENT).all() and (mean[rows] == SENT).all() and blocks[rows] == 0xA5A5A5A5, what
        # without the power rows the records are the same; a row mean needs them
        rec2, none, _, _ = pkg.aspec_plan_host(rows, wave, index[:stored], None, lo_hz, hi_hz, nbatches=nb, want_power=False)
        assert rec2.tobytes() == want[0].tobytes() and none is None


# The largest |P - P64| / max P64 of a block over every builder at 3 rows x 2 batches, P64 from numpy.fft in float64 over the same
# float32 windowed input, measured on the CPU: 2.53e-7 (the tone between two bins; noise and the voice-like signals give 2.5e-7 too, the
# other tones and the square wave 1.1e-7 to 2.3e-7, the constant 0.26e-7), about two float32 steps of the largest bin.  The bound is 4 x
# that, the margin test_oracle_stage1_plans.py took, for the same reason: room for other seeds without hiding a wrong butterfly, which
# moves a bin by a part in ten or more.
MEASURED_P_ERROR = 2.53e-7


def test_model_spectrum_against_a_float64_fft():
    worst = {}
    for name in am.BUILDERS:
        x = audio(name, 3, 2).reshape(-1, WAVE_BATCH)
        p = am.powers(x).astype(np.float64)
        z = np.fft.fft(am.windowed(x).astype(np.float64), axis=1)[:, :BINS]
        p64 = z.real ** 2 + z.imag ** 2
        top = p64.max(axis=1)
        live = top > 1e-60  # (silence and subnormal audio: every float32 product underflows, P must be exactly 0)
        assert not p[~live].any()
        worst[name] = float((np.abs(p - p64)[live].max(axis=1) / top[live]).max()) if live.any() else 0.0
    print("largest |P - P64| / max P64 per builder:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 4 * MEASURED_P_ERROR, worst


def flat(level=1.0):
    return np.full(BINS, level, np.float32)


def test_vote_thresholds(pkg):
    # equality on both sides of ratio: the floor is 1, the peak is 16 or its float32 neighbours
    for peak, found in ((np.float32(16.0), 0), (np.nextafter(np.float32(16.0), np.float32(17.0)), 1), (np.nextafter(np.float32(16.0), np.float32(0.0)), 0)):
        mean = flat()
        mean[200] = peak
        v = vote_pair(pkg, mean, 8)
        assert (v.found, v.bin, v.floor, v.peak) == (found, 200, 1.0, float(peak)), peak
    # the product is one float32 multiply: ratio 3 x floor 1/3 (as float32) is exactly 1.0f, though 3 x that floor exceeds 1 in float64
    third = np.float32(1.0) / np.float32(3.0)
    assert np.float32(3.0) * third == np.float32(1.0) and 3.0 * float(third) > 1.0
    mean = flat(third)
    mean[300] = np.nextafter(np.float32(1.0), np.float32(2.0))
    assert vote_pair(pkg, mean, 8, ratio=3.0).found == 1
    mean[300] = 1.0
    assert vote_pair(pkg, mean, 8, ratio=3.0).found == 0
    # min_blocks, default 8 and given
    mean = flat()
    mean[200] = 100.0
    for blocks, min_blocks, found in ((7, 0, 0), (8, 0, 1), (0, 0, 0), (1, 1, 1), (99, 100, 0), (100, 100, 1)):
        assert vote_pair(pkg, mean, blocks, min_blocks=min_blocks).found == found, (blocks, min_blocks)
    # ties go to the lowest bin, also between the band's ends
    mean = flat()
    mean[[486, 100, 300]] = 50.0
    assert vote_pair(pkg, mean, 8).bin == 100
    mean = flat()
    mean[[7, 487]] = 1e6  # outside the band: not looked at
    v = vote_pair(pkg, mean, 8)
    assert (v.found, v.bin, v.freq_hz) == (0, 8, 8.5 * HZ_PER_BIN)  # bins 8 .. 9 of a flat row: (8 + 9) / 2; bin 7 is clipped away
    # the floor is the median of bins 3 .. 34 away, the element (m - 1) / 2 of m: a peak at the band's low end has only the upper side
    mean = flat()
    mean[8] = 1000.0
    mean[11:43] = np.arange(1, 33, dtype=np.float32)  # m = 32 values 1 .. 32: index 15 is 16
    assert vote_pair(pkg, mean, 8).floor == 16.0
    mean = flat()
    mean[200] = 1000.0
    mean[166:198] = np.arange(1, 33, dtype=np.float32)
    mean[203:235] = np.arange(33, 65, dtype=np.float32)  # m = 64 values 1 .. 64: index 31 is 32
    v = vote_pair(pkg, mean, 8)
    assert v.floor == 32.0 and v.found == 1
    mean[[165, 198, 199, 201, 202, 235]] = 1e-3  # 1, 2 and 35 bins away: not part of the floor
    assert vote_pair(pkg, mean, 8).floor == 32.0
    # m = 0: a band narrower than the three bins the floor keeps away gives floor 0, and any positive peak is found
    mean = flat()
    assert pkg.aspec_band(1, 24) == (1, 3)
    v = vote_pair(pkg, mean, 8, lo_hz=1, hi_hz=24)
    assert (v.found, v.bin, v.floor) == (1, 1, 0.0)
    # an all-zero row
    v = vote_pair(pkg, np.zeros(BINS, np.float32), 100)
    assert (v.found, v.bin, v.freq_hz, v.peak, v.floor, v.votes) == (0, 8, 8 * HZ_PER_BIN, 0.0, 0.0, 0)
    # votes: records within one bin of p, the empty record never
    rec = np.zeros(6, pkg.ASPEC_RECORD_DTYPE)
    rec["peak_bin"] = [199, 200, 201, 202, 198, NONE]
    mean = flat()
    mean[200] = 100.0
    assert vote_pair(pkg, mean, 8, rec).votes == 3
    # the centroid over p - 1 .. p + 1
    mean = flat(0.0)
    mean[199:202] = [1.0, 2.0, 1.0]
    assert vote_pair(pkg, mean, 8).freq_hz == 200 * HZ_PER_BIN
    mean[199:202] = [0.0, 3.0, 1.0]
    assert vote_pair(pkg, mean, 8).freq_hz == HZ_PER_BIN * (200 * 3.0 + 201 * 1.0) / 4.0


def test_vote_on_the_builders(pkg):
    """8 blocks of one row under the default rule.  A tone exactly on bin 128 must come out within one bin's width of 1000 Hz.  Noise:
    the largest of 479 means of 8 blocks each stays within a few times their median, far below 16.  A whistle as strong as the voice
    puts (A N / 4)^2 = 2 p_v 250000 into its bin, where the voice, spread over some 380 bins, leaves about 2000 p_v a bin: 250 times
    the floor."""
    nb = 8
    index, first = am.full_index(1, nb)

    def vote(wave):
        records, _, mean, blocks = aspec_model(wave, index, first)
        twin = pkg.aspec_plan_host(1, wave, index, first)
        assert twin[2].tobytes() == mean.tobytes()
        v = vote_pair(pkg, mean[0], int(blocks[0]), records)
        print(f"found {v.found} bin {v.bin} freq {v.freq_hz:.3f} peak / floor {v.peak / v.floor if v.floor else math.inf:.3g} votes {v.votes} of {v.blocks}")
        return v

    v = vote(audio("tone_on_bin", 1, nb))
    assert v.found == 1 and v.bin == 128 and abs(v.freq_hz - 1000.0) < HZ_PER_BIN and v.votes == nb
    v = vote(audio("tone_between", 1, nb))
    assert v.found == 1 and abs(v.freq_hz - 128.5 * HZ_PER_BIN) < HZ_PER_BIN
    v = vote(audio("outside_strong", 1, nb))
    assert v.found == 1 and v.bin == am.INSIDE_BIN
    for name in ("silence", "subnormal", "noise"):
        assert vote(audio(name, 1, nb)).found == 0, name
    v = vote(am.voice(1, nb, whistle_db=0.0) * np.float32(0.7))
    assert v.found == 1 and abs(v.freq_hz - am.WHISTLE_HZ) < HZ_PER_BIN and v.votes >= nb // 2
    vote(audio("voice", 1, nb))  # (printed: tools/aspec_classes.py has the table)
    vote(audio("voice_whistle", 1, nb))
