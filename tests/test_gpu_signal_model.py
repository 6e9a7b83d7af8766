"""The HIP library against the float64 signal model: comparisons (b) and (c) of tests/test_signal_model.py with the same code and
bounds, on pkg.Demod, at the kernels and geometries the project ships.  Every test asserts the path that ran (last_path(),
last_stage1()) and, on the library's own flags and samples, that the compared span is open throughout -- nothing passes on zeros.
The model needs no oracle here: it starts from the IQ bytes."""
import pytest

import signal_cases as sc
import signal_model as sm
from test_signal_model import ROWS, assert_raw_iq_phase, check_notch_rows, check_row, check_tone_peaks

pytestmark = pytest.mark.gpu

AM_ROWS = [sc.AM_ON_GRID, sc.AM_OFF_GRID, sc.AM_LOUD]
STAGE1_EXCHANGE_FULL, STAGE1_LANE_PLAN = 0, 3


def _plan(pkg, case, rows=ROWS):
    dev = pkg.device_cfg(centerfreq=sc.CENTRE, **sc.CASES[case])
    chans = [c for r, c in enumerate(sc.channels(pkg.channel_cfg)) if r in rows]
    return dev, chans, [sc.ROW_NAMES[r] for r in rows], sc.capture(pkg, dev)


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
