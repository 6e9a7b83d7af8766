"""The squelch core chain of the time-parallel path with and without the round-4 run paths and restarts of k_tp_core2
(MI_AIRBAND_CORE_LEAN=1, the default / 0, the round-3 ones): the core state at every 512-step boundary is the oracle's serial
trace, bit for bit, on the inputs that exercise what the lean paths change -- the bench's gated signal (passes of four groups cut at
the group a burst starts or ends in, restarts of the noise-floor wave), short gate periods (many decays), a manual threshold, no
decay waves, and short / long leads of the noise-floor wave (many / few restarts).  And two overlapped 64-batch calls at the
headline plan: audio, flags and channel statistics."""
import ctypes as C

import numpy as np
import pytest

from common import AGC_EXTRA, WAVE_BATCH, assert_same, gen_iq, oracle_run, to_oracle_cfg

pytestmark = pytest.mark.gpu

CASES = {
    # name: (batches, gate_div, manual threshold on channel 1, extra environment)
    "bench-gated": (128, 1, False, {}),
    "short-gates": (96, 8, False, {}),
    "manual-threshold": (96, 2, True, {}),
    "no-decay-waves": (128, 1, False, {"MI_AIRBAND_CORE_DECAY": "0"}),
    "lead-128": (128, 1, False, {"MI_AIRBAND_CORE_LEAD": "128"}),
    "lead-1920": (128, 1, False, {"MI_AIRBAND_CORE_LEAD": "1920"}),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("lean", ["1", "0"], ids=["lean", "round3"])
def test_core_chain_matches_the_serial_trace(pkg, monkeypatch, lean, case):
    import libs
    nbat, gate_div, manual, env = CASES[case]
    monkeypatch.setenv("MI_AIRBAND_TP", "1")
    monkeypatch.setenv("MI_AIRBAND_CORE_LEAN", lean)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    centre, chans = pkg.config2_channels()
    if manual:
        chans[1] = pkg.channel_cfg(chans[1].freq, squelch_threshold_dbfs=-30)  # constant cap (the plan then takes the one-wave chain)
    dev = pkg.device_cfg(centerfreq=centre)
    iq, _ = gen_iq(pkg, dev, centre, chans, nbat, gate_div=gate_div)
    odev, ochans = to_oracle_cfg(dev, chans)
    od = libs.OracleDemod(odev, ochans)
    omag, _ = od.stage1(iq, nbat * WAVE_BATCH + AGC_EXTRA, want_iq=False)
    od.close()
    lib = libs.oracle_lib()
    lib.ao_squelch_core_trace.argtypes = [C.POINTER(libs.SquelchCfg), libs.f32p, C.c_size_t, C.c_size_t, libs.f32p]
    lib.ao_squelch_core_trace.restype = None
    lib.ao_dbfs_to_level.restype = C.c_float
    d = pkg.Demod(dev, chans, max_batches=nbat)
    d.process([iq], nbat)
    assert d.last_path() == (1, 0)
    n = nbat * WAVE_BATCH
    for c, ch in enumerate(chans):
        core, diag = d.tp_debug(c)
        ref = np.zeros(((n + 511) // 512 + 1, 4), np.float32)
        level = lib.ao_dbfs_to_level(C.c_float(ch.squelch_threshold_dbfs), 512) if ch.squelch_threshold_dbfs < 0 else 0.0
        cfg = libs.SquelchCfg(level, ch.has_snr_threshold, ch.squelch_snr_db, 0.0, 16000.0)
        lib.ao_squelch_core_trace(C.byref(cfg), np.ascontiguousarray(omag[c, AGC_EXTRA:]), n, 512, ref.reshape(-1))
        assert_same(core, ref, f"core chain ch{c} ({case}, lean={lean})")
        assert diag[3] == 0, f"ch{c}: segments left unverified: {diag.tolist()}"
        assert diag[2] == 0, f"ch{c}: serial fallback engaged, scans={diag.tolist()}"
    d.close()


@pytest.mark.parametrize("lean", ["1", "0"], ids=["lean", "round3"])
def test_two_overlapped_calls_at_the_headline_plan(pkg, monkeypatch, lean):
    """Two 64-batch calls in flight at once (MI_OPT_EARLY_INPUT, the bench's way of driving the library) on the headline plan and
    its gated signal: audio and flags are the oracle's, the channel statistics those of the serial kernel on the same capture."""
    import torch
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.setenv("MI_AIRBAND_CORE_LEAN", lean)
    centre, chans = pkg.config2_channels()
    dev = pkg.device_cfg(centerfreq=centre)
    calls = [64, 64]
    nbat = sum(calls)
    iq, _ = gen_iq(pkg, dev, centre, chans, nbat, gate_div=1)
    nb, owo, oaxc, _ = oracle_run(dev, chans, iq, nbat)
    assert nb == nbat
    pad = (iq.size + 255) // 256 * 256
    d_iq = torch.zeros(pad, dtype=torch.uint8, device="cuda")
    d_iq[:iq.size] = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.current_stream().cuda_stream
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
    d.set_option(pkg.OPT_EARLY_INPUT, 1)
    outs, flags, done = [], [], 0
    for k in calls:
        pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        wo = torch.empty((1, len(chans), k * WAVE_BATCH), dtype=torch.float32, device="cuda")
        ax = torch.empty((1, len(chans), k), dtype=torch.uint8, device="cuda")
        d.process_device(d_iq.data_ptr() + pos, pad - pos, k, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        assert d.last_path()[0] == 1
        outs.append(wo)
        flags.append(ax)
        done += k
    torch.cuda.synchronize()
    wo = torch.cat(outs, dim=2).cpu().numpy()
    ax = torch.cat(flags, dim=2).cpu().numpy()
    st = d.stats()
    d.close()
    assert (oaxc == 42).any() and (oaxc == 32).any()
    assert_same(ax[0], oaxc, "axcindicate")
    assert_same(wo[0], owo, "audio")
    monkeypatch.setenv("MI_AIRBAND_TP", "0")
    d2 = pkg.Demod(dev, chans, nstreams=1, max_batches=nbat)
    d2.process([iq], nbat)
    st2 = d2.stats()
    d2.close()
    for c in range(len(chans)):
        for f in ("noise_level", "signal_level", "squelch_level", "agcavgfast", "open_count", "flappy_count", "active_counter", "squelch_state"):
            assert getattr(st[c], f) == getattr(st2[c], f), (c, f)
