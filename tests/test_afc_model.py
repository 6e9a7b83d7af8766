"""AFC (rtl_airband.cpp:180-251) in the oracle against the float64 model of tests/afc_model.py, without a GPU.

For every case of tests/afc_cases.py the oracle is run batch by batch and the model is fed the oracle's own indicators: the
bin table after every batch, the base bins and the '<' / '>' indicators must be the model's exactly, and the squared spectrum
the oracle hands to its walk must be the model's spectrum of the batch's last window.  float32 and float64 may take a
comparison that is nearly a tie differently, so every comparison the model evaluates has to clear MARGIN; the cases are
built so that all of them do, and nothing is ever skipped.  The walk rule itself is run against ao_afc_check on seeded
random spectra whose values float32 holds exactly."""
import numpy as np
import pytest

import afc_cases as ac
import afc_model as am
import libs
import signal_model as sm

SQ_MEASURED = ac.SQ_MEASURED  # 3.55e-7 of the spectrum's maximum, measured (test_recorded_spectrum_error_is_the_measured_one)
MARGIN = ac.MARGIN            # 4 x that: 1.42e-6


def model_of(case, s, flags, shift=0):
    return am.run(case.capture(s), case.device(libs.device_cfg), case.channels(libs.channel_cfg), flags, shift=shift)


def assert_not_vacuous(case, s, r):
    """Every channel meant to move walks in its direction and returns to base inside the run; the others never move."""
    for c in range(len(case.chans)):
        want = case.expect(s, c)
        delta = r.bins[c] - r.base[c]
        if want == 0:
            assert (delta == 0).all(), f"{case.name}, stream {s}, channel {c}: must not move, bins - base {delta.tolist()}"
            continue
        walks, returns = r.moved(c)
        assert walks and returns, f"{case.name}, stream {s}, channel {c}: walks {walks}, returns {returns}"
        assert all(np.sign(delta[b]) == want for b in walks), f"{case.name}, stream {s}, channel {c}: bins - base {delta.tolist()}, meant {want:+d}"
        assert all(r.flags[c, b] == (am.AFC_UP if want > 0 else am.AFC_DOWN) for b in walks)


def check_case_specifics(case, r):
    n = case.n
    if case.name == "edges":
        # on-grid frequencies land one bin down: these are one Hz above the grid
        assert list(r.base[:4]) == [3, 2, n - 4, n - 3]
        assert [sm.bin_index(ac.CENTRE, ac.CENTRE, case.rate, n), sm.bin_index(ac.CENTRE + 1, ac.CENTRE, case.rate, n)] == [n - 1, 0]
        assert r.spectra[2].argmax() == 0, "the carrier sits in bin 0, beyond the upper edge"
        for c, end in ac.EDGE_END.items():
            walks, _ = r.moved(c)
            assert {int(r.bins[c, b]) for b in walks} == {end}, f"edges, channel {c}: walks end on {[int(r.bins[c, b]) for b in walks]}"
        # what the second stream is for: on the device its spectrum follows stream 0's, so sq[N] of stream 0 is the carrier again
        # and a walk without the stop at N - 1 runs on into it (and ends inside the second spectrum: no read beyond the two)
        both = np.concatenate([ac.oracle(case, 0)["sq"][1], ac.oracle(case, 1)["sq"][1]]).astype(np.float64)
        for c in (2, 3):
            assert n <= am.walk(both, +1, int(r.base[c]), case.chans[c].afc) < 2 * n - 1
    if case.name in ("hop150", "hop151"):
        # a call's batches start 2100 and then 2000 more windows into its IQ (the handle's first call), or 2000 k (later ones)
        hop_bytes = 2 * sm.hop_of(case.rate)
        starts = [(w * hop_bytes) % 16 for w in (2000, 2100, 4100)]
        assert (hop_bytes, starts) == {"hop150": (300, [0, 0, 0]), "hop151": (302, [0, 8, 8])}[case.name]
    if case.name == "first_batch":
        for c, ch in enumerate(case.chans):
            if ch.afc:
                assert r.action[c][0] == am.WALK and r.bins[c, 0] != r.base[c], f"first_batch, channel {c}: no walk in batch 0"
    if case.name == "walk_rules":
        a, b = ac.SAME_END
        assert r.base[a] != r.base[b] and r.bins[a, 1] == r.bins[b, 1] != r.base[a]


@pytest.mark.parametrize("name", list(ac.CASES))
def test_oracle_bins_flags_and_spectrum_equal_the_model(name):
    case = ac.CASES[name]
    assert 8 <= case.nbat <= 12 and case.nstreams * len(case.chans) <= 65
    for s in range(case.nstreams):
        o = ac.oracle(case, s)
        r = model_of(case, s, o["flags"])
        err = max(float(np.max(np.abs(o["sq"][b].astype(np.float64) - r.spectra[b])) / r.spectra[b].max()) for b in range(case.nbat))
        print(f"AFC, oracle vs float64 model: {name}, stream {s}: spectrum {err:.3e} of its maximum, smallest margin {r.min_margin():.3e}")
        assert list(o["base"]) == list(r.base) == case.base_bins()
        assert err <= MARGIN, f"{name}, stream {s}: squared spectrum off by {err:.3e}"
        assert r.min_margin() > MARGIN, f"{name}, stream {s}: a comparison lies {r.min_margin():.3e} from a tie"
        assert np.array_equal(o["bins"], r.bins), f"{name}, stream {s}: bins\n{o['bins'] - r.base[:, None]}\nmodel\n{r.bins - r.base[:, None]}"
        assert np.array_equal(o["flags"], r.flags), f"{name}, stream {s}: flags {[bytes(f) for f in o['flags']]}, model {[bytes(f) for f in r.flags]}"
        assert_not_vacuous(case, s, r)
        check_case_specifics(case, r)
    if case.stream_off:  # the bins of one channel differ from stream to stream
        after = np.stack([ac.oracle(case, s)["bins"][:, 2] for s in range(case.nstreams)])
        assert all(len(set(after[:, c])) >= 3 for c, ch in enumerate(case.chans) if ch.afc)


def spectrum_error(case, s):
    o = ac.oracle(case, s)
    r = model_of(case, s, o["flags"])
    return max(float(np.max(np.abs(o["sq"][b].astype(np.float64) - r.spectra[b])) / r.spectra[b].max()) for b in range(case.nbat))


def test_recorded_spectrum_error_is_the_measured_one():
    """SQ_MEASURED, from which MARGIN is taken, is the largest error over every case and stream as it is measured now: the
    figure in afc_cases.py and DESIGN.md section 5a cannot go stale unnoticed."""
    worst = max(spectrum_error(case, s) for case in ac.CASES.values() for s in range(case.nstreams))
    print(f"AFC, largest spectrum error over all cases: {worst:.4e}; recorded {ac.SQ_MEASURED:.3e}, margin {MARGIN:.3e}")
    assert 0.97 * ac.SQ_MEASURED <= worst <= ac.SQ_MEASURED


def test_model_depends_on_which_window_it_takes():
    """One window earlier or later and the model's bins of `walk_rules` are different ones: the channel with the one-window burst
    walks down on the batch's last window and up on its neighbours."""
    case = ac.CASES["walk_rules"]
    o = ac.oracle(case, 0)
    c = ac.MARKED
    assert (o["bins"][c, [1, 6]] < o["base"][c]).all()
    for shift in (-1, +1):
        r = model_of(case, 0, o["flags"], shift=shift)
        assert not np.array_equal(r.bins, o["bins"])
        assert (r.bins[c, [1, 6]] > r.base[c]).all(), f"shift {shift:+d}: {r.bins[c] - r.base[c]}"


def test_last_window_index():
    """Batch 0 waits for WAVE_BATCH + AGC_EXTRA windows, every later one for WAVE_BATCH more (rtl_airband.cpp:514-516, :677)."""
    assert [am.last_window(b) for b in range(3)] == [2099, 4099, 6099]


def random_spectrum(rng, n):
    """Integer re, im: re^2 + im^2 is exact in float32.  A peak with a jittered slope on either side, so that walks run for
    several bins, over a floor of small values."""
    peak, height, slope = int(rng.integers(0, n)), int(rng.integers(8, 60)), int(rng.integers(1, 6))
    k = np.arange(n)
    re = np.maximum(0, height - slope * np.abs(k - peak)) + rng.integers(0, 4, n)
    im = rng.integers(0, 4, n)
    return re.astype(np.int64), im.astype(np.int64)


def test_walk_equals_ao_afc_check_on_random_spectra():
    lib = libs.oracle_lib()
    rng = np.random.default_rng(20240611)
    seen = {(step, kind): 0 for step in (-1, 1) for kind in ("moved", "edge", "stayed")}
    per_afc = {1: 0, 2: 0, 5: 0, 255: 0}
    ends = []
    for i in range(600):
        n = int(rng.integers(8, 65))
        re, im = random_spectrum(rng, n)
        sq = (re * re + im * im).astype(np.float64)
        fft = np.zeros(2 * n, np.float32)
        fft[0::2], fft[1::2] = re, im
        base = [0, n - 1, int(rng.integers(0, n)), int(rng.integers(0, n))][i % 4]
        afc = [1, 2, 5, 255][(i // 4) % 4]
        for step in (-1, 1):
            want = am.walk(sq, step, base, afc)
            got = lib.ao_afc_check(fft, n, step, base, float(sq[base]), afc)
            assert got == want, f"spectrum {i}: n {n}, base {base}, afc {afc}, step {step:+d}: oracle {got}, model {want}\n{sq.tolist()}"
            assert 0 <= want < n
            seen[(step, "moved" if want != base else "stayed")] += 1
            seen[(step, "edge")] += want != base and want in (0, n - 1)
            per_afc[afc] += want != base
            ends.append(abs(want - base))
    assert all(v >= 10 for v in seen.values()), seen
    assert all(v >= 20 for v in per_afc.values()), per_afc
    assert max(ends) >= 5
