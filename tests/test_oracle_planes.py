"""The oracle's plane entry (ao_demod_run_planes) and the adversarial planes of plane_cases.py, on the CPU alone.

  - ao_demod_run_planes over stage 1's own output is ao_demod_run, bit for bit: the plane entry adds an input, not a second
    restatement of the sample loop.
  - On every plain AM family the oracle's whole loop and the Squelch component driver (squelch_run: the oracle's restatement, and
    the reference's own squelch.cpp where it has been compiled) take the same decisions at every step and end on the same counts and
    levels: the new inputs are tied to squelch.cpp itself, not only to its restatement.
  - Coverage conditions: each family does what it is there for (opens and closes, aborts on low signal, flaps and resets, grazes
    the threshold, disagrees with its filter, hears and misses its CTCSS tone, underflows to zero).  A generator that stops doing
    its job fails here, not silently on the GPU."""
import numpy as np
import pytest

import libs
import plane_cases as pc
import plane_plans as pp
from common import AGC_EXTRA, WAVE_BATCH, assert_same, bytes_for_batches, to_oracle_cfg
from conftest import load_package

NB = 24
PLANS = ["am16", "dynamic_range", "silence", "am96"]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _stats_tuple(s):
    return tuple(bits([getattr(s, f)])[0] for f in libs.STATS_LEVELS) + tuple(int(getattr(s, f)) for f in libs.STATS_COUNTS)


# ---------------------------------------------------------------- the plane entry is the IQ entry
def _iq_plan(which):
    pkg = load_package()
    if which == "config3":
        centre, chans = pkg.config3_channels()
        chans[3].has_iq_outputs = 1
        chans[4].has_iq_outputs = 1
        dev = pkg.device_cfg(centerfreq=centre, fft_size_log=11)
        kw = dict(gate_div=2, active=lambda k: k % 4 != 2, amp_q8=1024)
    else:  # the plan of test_manual_squelch_and_options
        centre = 120000000
        chans = [pkg.channel_cfg(centre + 250000, squelch_threshold_dbfs=-40),
                 pkg.channel_cfg(centre - 250000, squelch_snr_db=0.0, ampfactor=2.5),
                 pkg.channel_cfg(centre + 500000, modulation=pkg.MOD_NFM, tau=0, notch=1000.0, notch_q=5.0),
                 pkg.channel_cfg(centre - 500000, bandwidth=8000, has_iq_outputs=1),
                 pkg.channel_cfg(centre + 750000, modulation=pkg.MOD_NFM, ctcss=100.0, bandwidth=12500)]
        dev = pkg.device_cfg(centerfreq=centre, tau=75)
        kw = dict(gate_div=2, active=lambda k: True)
    n = bytes_for_batches(dev, 12) // 2
    carriers = pkg.carriers_for(centre, chans, amp_q8=kw.get("amp_q8", 3072), active=kw["active"])
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate // kw["gate_div"], carriers=carriers)
    return dev, chans, pkg.iqgen_host(cfg, 0, 0, n)


@pytest.mark.parametrize("which", ["config3", "manual_squelch_and_options"])
def test_run_planes_over_stage1_output_is_run(which):
    dev, chans, iq = _iq_plan(which)
    odev, ochans = to_oracle_cfg(dev, chans)
    nb = 12
    a = libs.OracleDemod(odev, ochans)
    a.trace_start(nb * WAVE_BATCH)
    n, wo, axc, iqo = a.run(iq, nb, want_iq=True)
    assert n == nb
    want_stats, want_look, want_trace = a.channel_stats(), a.lookahead(), a.trace()
    mag, z = a.stage1(iq, nb * WAVE_BATCH + AGC_EXTRA)  # (stage 1 touches no channel state; these plans have no AFC)
    a.close()
    raw = [i for i, c in enumerate(chans) if c.modulation == 1 or c.bandwidth != 0 or c.has_iq_outputs]
    assert raw, "the plan should have rows with raw I/Q"
    cplx = np.ascontiguousarray(z[raw])
    b = libs.OracleDemod(odev, ochans)
    b.trace_start(nb * WAVE_BATCH)
    got_wo, got_axc, got_iq, at, done = [], [], [], 0, 0
    for k in (1, 4, 7):
        count = k * WAVE_BATCH + (AGC_EXTRA if at == 0 else 0)
        n, w, x, q = b.run_planes(mag[:, at:at + count], k, cplx=cplx[:, at:at + count], want_iq=True)
        assert n == k
        got_wo.append(w), got_axc.append(x), got_iq.append(q.reshape(len(chans), k * WAVE_BATCH, 2))
        at, done = at + count, done + k
    assert_same(bits(np.concatenate(got_wo, axis=1)), bits(wo), "audio")
    assert_same(np.concatenate(got_axc, axis=1), axc, "flags")
    assert_same(bits(np.concatenate(got_iq, axis=1).reshape(len(chans), -1)), bits(iqo), "raw I/Q")
    assert_same(bits(b.lookahead()), bits(want_look), "lookahead")
    assert_same(b.trace(), want_trace, "per-step trace")
    assert [_stats_tuple(s) for s in b.channel_stats()] == [_stats_tuple(s) for s in want_stats], "counters and levels"
    assert (axc == ord("*")).any() and (axc == ord(" ")).any()
    b.close()


def test_run_planes_refuses_afc():
    od = libs.OracleDemod(libs.device_cfg(), [libs.channel_cfg(120250000, afc=2)])
    assert od.lib.ao_demod_run_planes(od.h, np.zeros(2100, np.float32), None, 2100, 1, np.zeros(2000, np.float32), None, None) == -1
    od.close()


# ---------------------------------------------------------------- the planes themselves
@pytest.mark.parametrize("name", PLANS)
def test_planes_are_finite_nonnegative_and_deterministic(name):
    nb = 16 if name == "am96" else NB
    L = 1024 if name == "am96" else 512
    rows, mag = pp.am_planes(name, nb, L)
    assert mag.dtype == np.float32 and mag.shape == (len(rows), AGC_EXTRA + nb * WAVE_BATCH)
    assert np.isfinite(mag).all() and (mag >= 0).all()
    # (the constant rows of `silence` differ in their squelch settings only)
    assert len({(m.tobytes(), st) for m, (_, _, st) in zip(mag, rows)}) == len(rows), "every row is a different plane"
    f, s, st = rows[0]
    pp.am_row.cache_clear()
    again = pp.am_row(f, s, st, nb * WAVE_BATCH, L)
    assert_same(bits(again), bits(mag[0]), "the same seed gives the same plane")


def test_edges_sit_on_the_boundaries_they_name():
    for L in (512, 4096):
        x = pc.edges_on_boundaries(0, pc.NSTEPS, L)[AGC_EXTRA:]
        hi = x > 2.0
        edges = np.flatnonzero(hi[1:] != hi[:-1]) + 1
        crit = pc.critical_positions(pc.NSTEPS, L)
        near = np.abs(edges[:, None] - crit[None, :]).min(axis=1) <= 1
        assert near.sum() >= 20 and len(edges) >= 60
        for unit in (1008, 1024, 4032, 4096, L, WAVE_BATCH, pc.LEAD):
            assert ((edges[:, None] - np.arange(-1, 2)[None, :]) % unit == 0).any(), f"no edge at a multiple of {unit} +-1"


# ---------------------------------------------------------------- tied to the reference's Squelch, and the coverage conditions
@pytest.fixture(scope="module")
def am_runs():
    out = {}
    for name in PLANS:
        nb = 16 if name == "am96" else NB
        rows, mag = pp.am_planes(name, nb, 1024 if name == "am96" else 512)
        res, trace = pp.oracle_calls(libs.device_cfg(), pp.am_chans(libs.channel_cfg, rows), mag, None, (nb,), trace=True)
        out[name] = (rows, mag, res[0], trace)
    return out


def _components():
    apis = [("the oracle's Squelch", libs.oracle())]
    if libs.ref_available():
        apis.append(("the compiled reference's Squelch", libs.ref()))
    return apis


@pytest.mark.parametrize("name", PLANS)
def test_whole_loop_equals_the_squelch_component_on_every_plain_am_family(am_runs, name):
    rows, mag, res, trace = am_runs[name]
    for what, api in _components():
        for r, (family, seed, setting) in enumerate(rows):
            # (ampfactor scales the audio behind the squelch: no part of the component)
            sq = api.squelch_run(mag[r, AGC_EXTRA:], **pp.squelch_kw(setting))
            tag = f"{what}, row {r} ({family} seed {seed}, {setting})"
            assert_same((sq["flags"] & 1).astype(bool), (trace[r] & libs.TRACE_OPEN).astype(bool), f"{tag}: per-step open mask")
            fin, st = sq["final"], res.stats[r]
            assert (fin.open_count, fin.flappy_count) == (st.open_count, st.flappy_count), tag
            assert_same(bits([fin.noise_level, fin.signal_level, fin.squelch_level]),
                        bits([st.noise_level, st.signal_level, st.squelch_level]), f"{tag}: final levels")


@pytest.mark.parametrize("name", ["am16", "dynamic_range", "silence"])
def test_cache_neutral_views_equal_the_getters(am_runs, name):
    """channel_stats() and the trace read squelch_level / should_filter / signal_outside_filter through views that leave the lazy cache
    alone; the statistics the GPU is compared with come from them.  Along every row -- once raw samples only, once with a filtered
    magnitude that disagrees with the raw one -- they answer what the getters answer on a copy of the state."""
    import ctypes as C
    rows, mag, _, _ = am_runs[name]
    lib = libs.oracle_lib()
    for r, (family, seed, setting) in enumerate(rows):
        kw = pp.squelch_kw(setting)
        cfg = libs.SquelchCfg(kw.get("manual_level", 0.0), 1 if "snr_db" in kw else 0, kw.get("snr_db", 0.0), 0.0, 16000.0)
        raw = np.ascontiguousarray(mag[r, AGC_EXTRA:])
        filt = np.ascontiguousarray(np.roll(raw, 700) * np.float32(0.8))
        assert lib.ao_squelch_peek_mismatches(C.byref(cfg), raw, None, raw.size) == 0, (family, seed, setting)
        assert lib.ao_squelch_peek_mismatches(C.byref(cfg), raw, filt.ctypes.data_as(C.c_void_p), raw.size) == 0, (family, seed, setting, "filtered")


MEANT_TO_OPEN = ("edges_on_boundaries", "threshold_grazers", "flap_and_recover", "regime_breakers", "noise_staircase", "random_walk")


@pytest.mark.parametrize("name", PLANS)
def test_every_family_does_its_job(am_runs, name):
    rows, mag, res, trace = am_runs[name]
    state = pp.state_of(trace)
    for r, (family, seed, setting) in enumerate(rows):
        tag = f"row {r} ({family} seed {seed}, {setting})"
        opened = (trace[r] & libs.TRACE_OPEN) != 0
        st = res.stats[r]
        # (of the two families of their own every row that carries spikes, bursts or noise: all but the constant 0.0 / 1e-40 rows)
        if family in MEANT_TO_OPEN or family == "dynamic_range" or (family == "silence" and not (seed % 4 == 1 or seed == 2)):
            assert opened.any() and not opened.all() and st.open_count >= 1, f"{tag}: meant to open and close"
            assert (np.diff(opened.astype(np.int8)) == -1).any(), f"{tag}: never closes again"
        if family in ("edges_on_boundaries", "flap_and_recover"):
            assert (state[r] == libs.SQ_LOW_SIGNAL_ABORT).any(), f"{tag}: LOW_SIGNAL_ABORT not reached"
        if family == "flap_and_recover":
            assert st.flappy_count > 0, f"{tag}: the flappy ratio never applied"
            assert (trace[r] & libs.TRACE_RESET).any(), f"{tag}: recent_open_count was never reset"
        if family == "threshold_grazers":
            assert pp.decisions(trace[r]) >= 20, f"{tag}: {pp.decisions(trace[r])} open / close decisions"
        if family == "silence" and seed % 4 in (0, 2):
            # Round to nearest never takes x * 0.99f to 0: below 50 units of the smallest subnormal the product rounds back to x
            # (49 * 0.99 = 48.51 -> 49), so over digital silence capped_ and full_ fall through the subnormals and stall there.
            # `pre_capped == 0.0` is therefore no state the recurrence has; what the row must reach is that stall.
            core = libs.oracle_core_trace(mag[r, AGC_EXTRA:], 16, **pp.squelch_kw(setting))
            tiny, ulp = np.finfo(np.float32).tiny, np.float32(1e-45)
            for col, what in ((2, "pre_capped"), (3, "pre_full")):
                v = core[:, col]
                assert (v > 0).all() and v.min() < tiny, f"{tag}: {what} never becomes subnormal"
                assert v.min() <= 50 * ulp and (v == v.min()).sum() > 16, f"{tag}: {what} does not fall to where x * 0.99f == x"
        if family == "silence" and seed % 4 == 1:
            assert 0 < mag[r, 0] < np.finfo(np.float32).tiny, "a subnormal row"
        if family == "dynamic_range" and seed % 3 == 0:
            assert mag[r].max() / mag[r].min() > 1e11
    if name == "am16":
        assert {s for _, _, s in rows} == set(pp.BASIC_SETTINGS), "every squelch setting on some row"


@pytest.fixture(scope="module")
def mixed_run():
    nb = 64
    mag, cplx = pp.mixed_planes(nb)
    chans = pp.mixed_chans(libs.channel_cfg)
    res, trace = pp.oracle_calls(libs.device_cfg(centerfreq=pp.CENTRE, tau=75), chans, mag, cplx, (nb,), want_iq=True, trace=True)
    return mag, cplx, res[0], trace


def test_mixed_plan_rows_do_their_job(mixed_run):
    mag, cplx, res, trace = mixed_run
    assert np.isfinite(mag).all() and (mag >= 0).all() and np.isfinite(cplx).all()
    z = cplx.astype(np.float64)
    assert np.isfinite((z[..., 0] ** 2 + z[..., 1] ** 2).astype(np.float32)).all(), "re^2 + im^2 stays finite in float32"
    for ch in range(len(pp.MIXED_ROWS)):
        opened = (trace[ch] & libs.TRACE_OPEN) != 0
        assert opened.any() and not opened.all(), f"channel {ch} {pp.MIXED_ROWS[ch]}: meant to open and close"
    for ch in pp.MIXED_LOWPASS:
        assert (trace[ch] & libs.TRACE_OUTSIDE_FILTER).any(), f"channel {ch}: signal_outside_filter at no step"
        filtering = (trace[ch] & libs.TRACE_FILTER) != 0
        assert filtering.any() and not filtering.all(), f"channel {ch}: the low-pass is meant to run in stretches"
        assert filtering[(trace[ch] & libs.TRACE_OUTSIDE_FILTER) != 0].all(), "signal_outside_filter only where the sample was filtered"
    for ch in pp.MIXED_CTCSS:
        st = res.stats[ch]
        assert st.ctcss_count > 0 and st.no_ctcss_count > 0, f"channel {ch}: ctcss {st.ctcss_count}, no ctcss {st.no_ctcss_count}"
    assert (res.iqo[3] != 0).any() and (res.iqo[5] != 0).any() and (res.iqo[6] != 0).any(), "rows with raw I/Q outputs emit some"
