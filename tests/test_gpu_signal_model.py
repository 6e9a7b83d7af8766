"""The HIP library against the float64 signal model: comparisons (b) and (c) of tests/test_signal_model.py with the same code and
bounds, on pkg.Demod, at the kernels and geometries the project ships.  Every test asserts the path that ran (last_path(),
last_stage1()) and, on the library's own flags and samples, that the compared span is open throughout -- nothing passes on zeros.
The model needs no oracle here: it starts from the IQ bytes."""
import functools

import numpy as np
import pytest

import signal_cases as sc
import signal_model as sm
from test_signal_model import (FILTERED_ROWS, ROWS, assert_raw_iq_phase, check_lag_of_the_raw_iq_rows, check_notch_rows, check_row, check_tone_peaks,
                               check_tone_through_the_lowpass)

pytestmark = pytest.mark.gpu

AM_ROWS = [sc.AM_ON_GRID, sc.AM_OFF_GRID, sc.AM_LOUD]
STAGE1_EXCHANGE_FULL, STAGE1_LANE_PLAN = 0, 3


def _plan(pkg, case, rows=ROWS, row_set="plain"):
    make, all_names = sc.ROW_SETS[row_set]
    dev = pkg.device_cfg(centerfreq=sc.CENTRE, **sc.CASES[case])
    chans = [c for r, c in enumerate(make(pkg.channel_cfg)) if r in rows]
    return dev, chans, [all_names[r] for r in rows], sc.capture(pkg, dev)


def _run(pkg, name, dev, chans, names, raw, options=()):
    """One host-entry call of all 16 batches."""
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=sc.NBATCHES)
    for opt, val in options:
        d.set_option(opt, val)
    want_iq = any(c.has_iq_outputs for c in chans)
    wo, axc, iqo, stats = d.process([raw], sc.NBATCHES, want_iq=want_iq)
    path, stage1, timeouts = d.last_path(), d.last_stage1(), d.pre_wave_timeouts()
    d.close()
    n = sc.NBATCHES * sc.WAVE_BATCH
    be = sc.Backend(name, wo[0, :, :n], axc[0], iqo[0] if want_iq else None, [s.squelch_level for s in stats], names)
    print(f"{name}: last_path {path}, last_stage1 {stage1}, pre_wave_timeouts {timeouts}")
    assert timeouts == 0
    return be, path, stage1


def _check_all(be, model, clamp_row=None):
    worst_audio, worst_iq = 0.0, 0.0
    for row in range(len(model.chans)):
        a, q = check_row(be, model, row, clamp_must_engage=(row == clamp_row))
        worst_audio, worst_iq = max(worst_audio, a), max(worst_iq, q or 0.0)
    print(f"{be.name}: worst audio residual {worst_audio:.3e} RMS, worst raw I/Q residual {worst_iq:.3e}")


@pytest.mark.parametrize("tp", ["time-parallel", "serial"])
def test_am_plan_at_fft_512(pkg, monkeypatch, tp):
    """The three plain AM rows (on the grid, off it, ampfactor 3 into the clamp) in one 16-batch call: by default the
    time-parallel path, with MI_AIRBAND_TP=0 the serial kernel."""
    if tp == "serial":
        monkeypatch.setenv("MI_AIRBAND_TP", "0")
    else:
        monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw = _plan(pkg, "fft512", AM_ROWS)
    be, path, stage1 = _run(pkg, f"hip fft512 AM plan, {tp}", dev, chans, names, raw)
    assert path == ((1, 0) if tp == "time-parallel" else (0, 0))
    assert stage1 == STAGE1_LANE_PLAN
    model = sc.Model(dev, chans, raw)
    _check_all(be, model, clamp_row=2)
    check_tone_peaks(be, chans, model.span, range(len(chans)))


def test_mixed_set_at_fft_2048_on_the_lane_kernel_with_the_split(pkg, monkeypatch):
    """All nine rows at fft 2048, the mixed split forced (MI_OPT_TIME_PARALLEL = 1): the plain AM rows time-parallel, the others
    through the serial kernel, stage 1 on the plan-compiled lane kernel."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    dev, chans, names, raw = _plan(pkg, "fft2048")
    be, path, stage1 = _run(pkg, "hip fft2048 mixed split", dev, chans, names, raw, options=[(pkg.OPT_TIME_PARALLEL, 1)])
    assert path == (1, 0) and stage1 == STAGE1_LANE_PLAN
    model = sc.Model(dev, chans, raw)
    _check_all(be, model)
    check_tone_peaks(be, chans, model.span, ROWS)
    check_notch_rows(be, chans, model.span, _atan_bound())


def _atan_bound():
    from test_signal_model import atan_bound
    return atan_bound()


def test_fft_4096_on_the_exchange_kernel(pkg, monkeypatch):
    """fft 4096 has no lane kernel.  The 625 Hz bins cut the 2.5 kHz deviation to pieces (the NFM audio is a tenth of what it is
    at fft 512), which the model follows like anything else; the tone check is for the AM rows."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw = _plan(pkg, "fft4096")
    be, path, stage1 = _run(pkg, "hip fft4096", dev, chans, names, raw)
    assert path == (0, 0) and stage1 == STAGE1_EXCHANGE_FULL
    model = sc.Model(dev, chans, raw)
    _check_all(be, model)
    check_tone_peaks(be, chans, model.span, AM_ROWS)


def test_s16_input(pkg, monkeypatch):
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw = _plan(pkg, "fft512_s16")
    be, path, stage1 = _run(pkg, "hip fft512 s16", dev, chans, names, raw)
    assert path == (0, 0) and stage1 == STAGE1_LANE_PLAN
    model = sc.Model(dev, chans, raw)
    _check_all(be, model, clamp_row=sc.AM_LOUD)
    check_tone_peaks(be, chans, model.span, ROWS)


def test_fm_quadri_and_the_physics_at_fft_512(pkg, monkeypatch):
    """fm_quadri = 1 on the serial kernel; the raw I/Q (which the discriminator does not touch) carries the modulation and no
    slope, and the notch row has lost the carrier's 100 Hz tone."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw = _plan(pkg, "fft512_quadri")
    be, path, stage1 = _run(pkg, "hip fft512 quadri", dev, chans, names, raw)
    assert path == (0, 0) and stage1 == STAGE1_LANE_PLAN
    model = sc.Model(dev, chans, raw)
    _check_all(be, model, clamp_row=sc.AM_LOUD)
    check_tone_peaks(be, chans, model.span, ROWS)
    assert_raw_iq_phase(be, chans, model.span)
    check_notch_rows(be, chans, model.span, _atan_bound())


def test_2500_ksps_at_fft_1024(pkg, monkeypatch):
    """Hop 156 of 156.25: the one geometry where the correction term of dm_dphi is not zero.  The lane kernel is built for hops
    160 and 128, so stage 1 is the exchange kernel."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw = _plan(pkg, "fft1024_2500k")
    be, path, stage1 = _run(pkg, "hip fft1024 2.5 MS/s", dev, chans, names, raw)
    assert path == (0, 0) and stage1 == STAGE1_EXCHANGE_FULL
    model = sc.Model(dev, chans, raw)
    _check_all(be, model)
    check_tone_peaks(be, chans, model.span, ROWS)


@pytest.mark.parametrize("plan", ["am", "mixed"])
def test_two_calls_with_early_input_across_the_span(pkg, monkeypatch, plan):
    """14 + 2 batches as two device calls in flight with MI_OPT_EARLY_INPUT: the boundary (audio sample 28 000) lies inside the
    compared span 27 900 .. 31 900, so the carried audio lookahead, plane heads, accumulator and filter state are all in it.
    The AM plan is forced time-parallel in both calls, the mixed set runs the serial kernel."""
    import torch
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    dev, chans, names, raw = _plan(pkg, "fft512", AM_ROWS if plan == "am" else ROWS)
    calls = [14, 2]
    assert calls[0] * sc.WAVE_BATCH in range(*sc.SPAN)
    nch = len(chans)
    pad = (raw.size + 255) // 256 * 256
    d_iq = torch.zeros(pad, dtype=torch.uint8, device="cuda")
    d_iq[:raw.size] = torch.from_numpy(raw).cuda()
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    d.set_option(pkg.OPT_EARLY_INPUT, 1)
    if plan == "am":
        d.set_option(pkg.OPT_TIME_PARALLEL, 1)
    want_iq = plan != "am"
    outs = [(torch.empty((1, nch, k * sc.WAVE_BATCH), dtype=torch.float32, device="cuda"), torch.empty((1, nch, k), dtype=torch.uint8, device="cuda"),
             torch.zeros((1, nch, k * sc.WAVE_BATCH, 2), dtype=torch.float32, device="cuda")) for k in calls]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    done = 0
    for k, (wo, ax, zo) in zip(calls, outs):
        pos = 0 if done == 0 else (done * sc.WAVE_BATCH + sm.AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, pad - pos, k, wo.data_ptr(), ax.data_ptr(), d_iq_out_ptr=zo.data_ptr() if want_iq else None, hip_stream=side.cuda_stream)
        done += k
    kernels = [[t[0] for t in d.kernel_times(age=age)] for age in (1, 0)]
    path, stage1 = d.last_path(), d.last_stage1()
    torch.cuda.synchronize()
    levels = [s.squelch_level for s in d.stats()]
    timeouts = d.pre_wave_timeouts()
    d.close()
    name = f"hip fft512 {plan} plan, calls {calls} in flight"
    print(f"{name}: last_path {path}, last_stage1 {stage1}, kernels {kernels}")
    assert timeouts == 0 and stage1 == STAGE1_LANE_PLAN
    if plan == "am":
        assert path == (1, 0) and all("k_tp_core" in " ".join(k) for k in kernels), "both calls time-parallel"
    else:
        assert path == (0, 0) and all("k_demod" in " ".join(k) for k in kernels), "both calls on the serial kernel"
    be = sc.Backend(name, torch.cat([o[0][0] for o in outs], dim=1).cpu().numpy(), torch.cat([o[1][0] for o in outs], dim=1).cpu().numpy(),
                    torch.cat([o[2][0] for o in outs], dim=1).cpu().numpy(), levels, names)
    model = sc.Model(dev, chans, raw)
    _check_all(be, model, clamp_row=2 if plan == "am" else sc.AM_LOUD)
    check_tone_peaks(be, chans, model.span, range(nch))


# ------------------------------------------------------------------ AM on the raw-I/Q path and the low-pass (sc.filtered_channels)

@functools.lru_cache(maxsize=None)
def _filtered_case(case):
    """(dev, chans, names, capture, model) of the second channel set, built once per case: the model starts from the bytes and
    its rows are cached, so the tests below share one."""
    from conftest import load_package
    dev, chans, names, raw = _plan(load_package(), case, FILTERED_ROWS, "filtered")
    return dev, chans, names, raw, sc.Model(dev, chans, raw)


BOUNDARY = 14 * sc.WAVE_BATCH  # where the split runs below cut the span


def _check_filtered(be, model, physics=False, boundary=False):
    _check_all(be, model, clamp_row=sc.F_AM_BW15000_LOUD if model.dev.fft_size_log == 9 else None)
    check_tone_peaks(be, model.chans, model.span, FILTERED_ROWS)
    check_lag_of_the_raw_iq_rows(be, model.chans, model.span)
    if physics:
        check_tone_through_the_lowpass(be, model.chans, model.span)
    if boundary:
        # The 100 magnitudes a call leaves behind must be the overwritten ones: carried as stage 1 wrote them, an AM row on the
        # raw-I/Q path is wrong by its whole audio for the 100 samples after the boundary (and its average for longer).
        for row in FILTERED_ROWS:
            m = model.row(row, sc.mode_for(model.chans[row]), be)
            k = BOUNDARY - model.span[0]
            worst = float(np.max(np.abs(be.waveout[row, BOUNDARY:BOUNDARY + 200] - m["audio"][k:k + 200])))
            print(f"{be.name} row {be.names[row]}: largest audio error over samples {BOUNDARY} .. {BOUNDARY + 200}: {worst:.3e} (bound {10 * sc.AUDIO_BOUND:.0e})")
            assert worst <= 10 * sc.AUDIO_BOUND


@pytest.mark.parametrize("pre_wave,audio_wave,steady", [(0, 0, 1), (1, 1, 1), (1, 0, 1), (2, 1, 1), (1, 1, 0)])
def test_filtered_rows_on_the_serial_kernel_at_fft_512(pkg, monkeypatch, pre_wave, audio_wave, steady):
    """The lagged overwrite lives in the channel's own wave, the pre-filter wave, the audio wave and the steady blocks, each with
    code of its own: every combination against the model."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw, model = _filtered_case("fft512")
    be, path, stage1 = _run(pkg, f"hip fft512 filtered rows, pre_wave {pre_wave} audio_wave {audio_wave} steady {steady}", dev, chans, names, raw,
                            options=[(pkg.OPT_PRE_WAVE, pre_wave), (pkg.OPT_AUDIO_WAVE, audio_wave), (pkg.OPT_STEADY_BLOCKS, steady)])
    assert path == (0, 0) and stage1 == STAGE1_LANE_PLAN
    _check_filtered(be, model, physics=True)


def test_filtered_rows_on_the_lane_packed_kernel(pkg, monkeypatch):
    """MI_OPT_UNI_ROWS = 1: eight rows are more than one, so k_demod packs them one lane per row."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw, model = _filtered_case("fft512")
    be, path, stage1 = _run(pkg, "hip fft512 filtered rows, lane-packed", dev, chans, names, raw, options=[(pkg.OPT_UNI_ROWS, 1)])
    assert path == (0, 0) and stage1 == STAGE1_LANE_PLAN
    _check_filtered(be, model, physics=True)


def test_filtered_rows_with_the_mixed_split(pkg, monkeypatch):
    """MI_OPT_TIME_PARALLEL = 1: the plain row goes time-parallel, the seven others through the serial kernel in the same call."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    dev, chans, names, raw, model = _filtered_case("fft512")
    be, path, stage1 = _run(pkg, "hip fft512 filtered rows, mixed split", dev, chans, names, raw, options=[(pkg.OPT_TIME_PARALLEL, 1)])
    assert path == (1, 0) and stage1 == STAGE1_LANE_PLAN
    _check_filtered(be, model, physics=True)


@pytest.mark.parametrize("case,kind", [("fft2048_quadri", STAGE1_LANE_PLAN), ("fft1024_2500k", STAGE1_EXCHANGE_FULL)])
def test_filtered_rows_at_other_geometries(pkg, monkeypatch, case, kind):
    """fft 2048 with fm_quadri: the lane kernel, the quadrature discriminator behind the low-pass.  fft 1024 at 2.5 MS/s: the
    exchange kernel and a dm_dphi whose correction term is not zero -- a wrong increment leaves the carrier off DC for the
    low-pass to eat."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw, model = _filtered_case(case)
    be, path, stage1 = _run(pkg, f"hip {case} filtered rows", dev, chans, names, raw)
    assert path == (0, 0) and stage1 == kind
    _check_filtered(be, model)


def test_filtered_rows_in_16_calls_of_one_batch(pkg, monkeypatch):
    """Every batch a call of its own: the overwritten head of wavein, the low-pass state and the accumulator cross 15 boundaries."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw, model = _filtered_case("fft512")
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=1)
    wos, axs, iqs = [], [], []
    for k in range(sc.NBATCHES):
        pos = 0 if k == 0 else (k * sc.WAVE_BATCH + sm.AGC_EXTRA) * d.hop_bytes
        wo, axc, iqo, stats = d.process([raw[pos:]], 1, want_iq=True)
        assert d.last_path() == (0, 0) and d.last_stage1() == STAGE1_LANE_PLAN
        wos.append(wo[0, :, :sc.WAVE_BATCH]), axs.append(axc[0]), iqs.append(iqo[0])
    timeouts = d.pre_wave_timeouts()
    d.close()
    assert timeouts == 0
    be = sc.Backend("hip fft512 filtered rows, 16 calls of one batch", np.concatenate(wos, axis=1), np.concatenate(axs, axis=1), np.concatenate(iqs, axis=1),
                    [s.squelch_level for s in stats], names)
    _check_filtered(be, model, boundary=True)


def test_filtered_rows_across_a_checkpoint(pkg, monkeypatch):
    """get_state() after 14 batches, set_state() into a fresh handle, 2 more batches there: the boundary at sample 28 000 lies in
    the span, and the state blob has to hold the overwritten magnitudes."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, names, raw, model = _filtered_case("fft512")
    calls = [14, 2]
    a = pkg.Demod(dev, chans, nstreams=1, max_batches=14)
    wo1, ax1, iq1, _ = a.process([raw], calls[0], want_iq=True)
    path1, timeouts = a.last_path(), a.pre_wave_timeouts()
    blob = a.get_state()
    a.close()
    b = pkg.Demod(dev, chans, nstreams=1, max_batches=14)
    b.set_state(blob)
    pos = (calls[0] * sc.WAVE_BATCH + sm.AGC_EXTRA) * b.hop_bytes
    wo2, ax2, iq2, stats = b.process([raw[pos:]], calls[1], want_iq=True)
    path2, stage1 = b.last_path(), b.last_stage1()
    timeouts += b.pre_wave_timeouts()
    b.close()
    assert path1 == (0, 0) and path2 == (0, 0) and stage1 == STAGE1_LANE_PLAN and timeouts == 0
    be = sc.Backend("hip fft512 filtered rows, checkpoint after 14 batches", np.concatenate([wo1[0, :, :calls[0] * sc.WAVE_BATCH], wo2[0, :, :calls[1] * sc.WAVE_BATCH]], axis=1),
                    np.concatenate([ax1[0], ax2[0]], axis=1), np.concatenate([iq1[0], iq2[0]], axis=1), [s.squelch_level for s in stats], names)
    _check_filtered(be, model, boundary=True)


def test_filtered_rows_in_two_calls_with_early_input(pkg, monkeypatch):
    """14 + 2 batches as two device calls in flight with MI_OPT_EARLY_INPUT, as test_two_calls_with_early_input_across_the_span
    does for the first channel set: stage 1 of the second call runs under k_demod of the first, which is still overwriting the
    magnitudes the second call's head is carried from."""
    import torch
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    dev, chans, names, raw, model = _filtered_case("fft512")
    calls = [14, 2]
    assert calls[0] * sc.WAVE_BATCH == BOUNDARY and BOUNDARY in range(*sc.SPAN)
    nch = len(chans)
    pad = (raw.size + 255) // 256 * 256
    d_iq = torch.zeros(pad, dtype=torch.uint8, device="cuda")
    d_iq[:raw.size] = torch.from_numpy(raw).cuda()
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    d.set_option(pkg.OPT_EARLY_INPUT, 1)
    outs = [(torch.empty((1, nch, k * sc.WAVE_BATCH), dtype=torch.float32, device="cuda"), torch.empty((1, nch, k), dtype=torch.uint8, device="cuda"),
             torch.zeros((1, nch, k * sc.WAVE_BATCH, 2), dtype=torch.float32, device="cuda")) for k in calls]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    done = 0
    for k, (wo, ax, zo) in zip(calls, outs):
        pos = 0 if done == 0 else (done * sc.WAVE_BATCH + sm.AGC_EXTRA) * d.hop_bytes
        d.process_device(d_iq.data_ptr() + pos, pad - pos, k, wo.data_ptr(), ax.data_ptr(), d_iq_out_ptr=zo.data_ptr(), hip_stream=side.cuda_stream)
        done += k
    kernels = [[t[0] for t in d.kernel_times(age=age)] for age in (1, 0)]
    path, stage1 = d.last_path(), d.last_stage1()
    torch.cuda.synchronize()
    levels = [s.squelch_level for s in d.stats()]
    timeouts = d.pre_wave_timeouts()
    d.close()
    name = f"hip fft512 filtered rows, calls {calls} in flight"
    print(f"{name}: last_path {path}, last_stage1 {stage1}, kernels {kernels}")
    assert timeouts == 0 and stage1 == STAGE1_LANE_PLAN
    assert path == (0, 0) and all("k_demod" in " ".join(k) for k in kernels), "both calls on the serial kernel"
    be = sc.Backend(name, torch.cat([o[0][0] for o in outs], dim=1).cpu().numpy(), torch.cat([o[1][0] for o in outs], dim=1).cpu().numpy(),
                    torch.cat([o[2][0] for o in outs], dim=1).cpu().numpy(), levels, names)
    _check_filtered(be, model, boundary=True)


# ------------------------------------------------------------------ dBFS

def test_manual_threshold_brackets_a_steady_carrier(pkg, monkeypatch):
    """As test_oracle_manual_threshold_brackets_a_steady_carrier: the channel whose threshold lies 3 dB under the carrier's
    measured level is open for the whole of its second half, the one 3 dB over never opens."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev = pkg.device_cfg(centerfreq=sc.CENTRE, fft_size_log=9)
    raw = sc.dbfs_capture(dev)
    chans, db, (under, over) = sc.dbfs_bracket(pkg.channel_cfg, dev, raw)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=sc.DBFS_BATCHES)
    wo, axc, _, stats = d.process([raw], sc.DBFS_BATCHES)
    path, stage1, timeouts = d.last_path(), d.last_stage1(), d.pre_wave_timeouts()
    d.close()
    print(f"carrier at {db:.2f} dBFS, thresholds {under} and {over}; last_path {path}, last_stage1 {stage1}")
    assert path[1] == 0 and stage1 == STAGE1_LANE_PLAN and timeouts == 0
    levels = [s.squelch_level for s in stats]
    assert np.allclose(levels, [sc.dbfs_to_level(under, 512), sc.dbfs_to_level(over, 512)], rtol=2e-6, atol=0)
    sc.assert_dbfs_bracket(sc.Backend("hip dBFS bracket", wo[0, :, :sc.DBFS_BATCHES * sc.WAVE_BATCH], axc[0], None, levels, ["under", "over"]))
