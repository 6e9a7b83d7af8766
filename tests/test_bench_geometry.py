"""Oracle parity at the geometries bench.py times, the two fuzzers as seeded tests, and the handle's device memory.

The product's claim is "bit for bit equal to the CPU oracle"; tests/test_gpu_parity.py proves it on small shapes.  Here the plans and
captures are built with the package helpers bench.py uses (config3_channels, device_cfg, carriers_for, iqgen_cfg) at the call sizes,
stream counts and options of `bench.py --workload config3` and `--workload config4`, through the C ABI (pkg.Demod), and every float of
the audio, every batch flag and the raw I/Q of the rows that have it are compared with the oracle (assert_same).  What a capture has
to exercise (rows that open and close, no clipped byte, ...) is asserted on the oracle's output, so a changed generator cannot
hollow a test out.  Every test prints the path the library took, its stage-1 variant and the open fractions it ran on."""
import hashlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import fuzz_plans
from common import AGC_EXTRA, WAVE_BATCH, assert_same, bytes_for_batches, gen_iq, oracle_run

pytestmark = pytest.mark.gpu

STAR = ord("*")
ORACLE_THREADS = 8  # airband_oracle.c keeps no mutable file-scope state and ctypes releases the GIL (checked in the 64-stream test)
FUZZ_SEEDS = list(range(20))


def _flag_stats(oaxc):
    """Per row of the oracle's batch flags: fraction of open batches, number of flag changes, opens and closes."""
    is_open = np.asarray(oaxc) == STAR
    return is_open.mean(axis=1), (is_open[:, 1:] != is_open[:, :-1]).sum(axis=1), is_open.any(axis=1) & ~is_open.all(axis=1)


def _clipped(iq):
    return int(np.count_nonzero((iq == 0) | (iq == 255)))


def _pos(d, done):
    """Byte offset of a stream after `done` batches (input_t.bufs advances hop bytes per window, rtl_airband.cpp:691)."""
    return 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes


def _kernel_names(d, age):
    """Kernels of the call `age` calls back, from its timing events: unlike last_path() this does not wait for the whole device, so
    the path of an earlier call can be read after the calls have overlapped."""
    return [t[0] for t in d.kernel_times(age=age)]


SERIAL_KERNELS = ["k_channelize", "k_demod"]


# ---- 1. bench.py --workload config3 -------------------------------------------------------------------------------------------

# Open batches per row out of the 128, as whole counts: the fractions the captures were specified with (bench signal: AM rows 0.50-0.52
# of the batches; all on: AM 0.62-0.65, NFM 0.57-0.66, CTCSS rows 0.57-0.58) times 128, rounded inwards -- except the upper end of the
# bench signal's AM rows, where the figure is the two-decimal print of 67 / 128 = 0.5234.
CONFIG3_CAPTURES = {
    # the carriers bench.py's run_workload generates: one on every AM row, none on an NFM row, gate 1 s
    "bench-signal": dict(gen=dict(gate_div=1, amp_q8=1024), iq_rows=(), am_open=(64, 67), nfm_open=None, ctcss_open=None,
                         am_changes=15, nfm_changes=None),
    # a carrier on every row (CTCSS rows with their tone), gate 1/3 s; raw I/Q on NFM rows only: on an AM row it would move the row
    # to the serial half and change the 16 + 16 split
    "all-carriers-on": dict(gen=dict(gate_div=3, amp_q8=768, active=lambda k: True), iq_rows=(1, 17), am_open=(80, 83),
                            nfm_open=(73, 84), ctcss_open=(73, 74), am_changes=47, nfm_changes=47),
}


@pytest.mark.parametrize("capture", list(CONFIG3_CAPTURES))
def test_config3_geometry_mixed_split_at_fft_2048_in_two_overlapping_64_batch_calls(pkg, monkeypatch, capture):
    """bench.py --workload config3: the 32-channel plan at fft 2048, one stream, 64-batch device calls overlapping on a stream of
    the caller's own with MI_OPT_EARLY_INPUT, every other option at its default.  From 64 batches on the mixed plan splits by
    itself: the 16 plain AM rows go down the time-parallel path, the 16 NFM rows through the serial kernel on a stream of its own,
    k_channelize<11> feeding alternating complex plane sets.  Two such calls back to back against one 128-batch oracle run --
    on the benchmark's own signal (no carrier on any NFM row) and with every carrier on (open NFM + low-pass + CTCSS + notch rows)."""
    import torch
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    case = CONFIG3_CAPTURES[capture]
    calls = [64, 64]
    nbat = sum(calls)
    centre, chans = pkg.config3_channels()
    for c in case["iq_rows"]:
        assert chans[c].modulation == pkg.MOD_NFM
        chans[c].has_iq_outputs = 1
    nch = len(chans)
    am = np.array([fuzz_plans.is_plain_am(pkg, c) for c in chans])
    ctcss = np.array([c.ctcss_freq > 0 for c in chans])
    assert am.sum() == 16 and (~am).sum() == 16 and ctcss.sum() == 4, "the benchmark's row split: 16 time-parallel + 16 serial"
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=11)
    iq, _ = gen_iq(pkg, dev, centre, chans, nbat, **case["gen"])

    # what the capture has to exercise, from the oracle alone
    nb, owo, oaxc, oiq = oracle_run(dev, chans, iq, nbat, want_iq=bool(case["iq_rows"]))
    assert nb == nbat
    frac, changes, both = _flag_stats(oaxc)
    print(f"config3 {capture}: open fraction AM {frac[am].min():.4f}-{frac[am].max():.4f}, NFM {frac[~am].min():.4f}-{frac[~am].max():.4f}, "
          f"CTCSS {frac[ctcss].min():.4f}-{frac[ctcss].max():.4f}; flag changes AM {changes[am].min()}-{changes[am].max()}, "
          f"NFM {changes[~am].min()}-{changes[~am].max()}; clipped bytes {_clipped(iq)}")
    assert _clipped(iq) == 0
    assert not np.isnan(owo).any()
    nopen = (oaxc == STAR).sum(axis=1)
    lo, hi = case["am_open"]
    assert (nopen[am] >= lo).all() and (nopen[am] <= hi).all(), "AM rows: open batches"
    assert both[am].all(), "every AM row opens and closes"
    assert (changes[am] >= case["am_changes"]).all()
    if case["nfm_open"] is None:
        assert not (oaxc[~am] == STAR).any(), "the benchmark's signal opens no NFM row"
        assert (changes[~am] == 0).all()
    else:
        assert both.all(), "every one of the 32 rows opens and closes"
        lo, hi = case["nfm_open"]
        assert (nopen[~am] >= lo).all() and (nopen[~am] <= hi).all(), "NFM rows: open batches"
        lo, hi = case["ctcss_open"]
        assert (nopen[ctcss] >= lo).all() and (nopen[ctcss] <= hi).all(), "CTCSS rows: open batches"
        assert (changes >= case["nfm_changes"]).all()

    pad = (iq.size + 255) // 256 * 256
    d_iq = torch.zeros(pad, dtype=torch.uint8, device="cuda")
    d_iq[:iq.size] = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    # Two readings.  "in flight": both calls enqueued with no host synchronisation between them, so the second overlaps the first;
    # the first call's path is then read from its timing events.  "drained": last_path() after each call, which waits for the device.
    for reading in ("in flight", "drained"):
        what = f"config3 {capture}, calls {reading}"
        d = pkg.Demod(dev, chans, nstreams=1, max_batches=max(calls))
        d.set_option(pkg.OPT_EARLY_INPUT, 1)
        outs = [(torch.empty((1, nch, k * WAVE_BATCH), dtype=torch.float32, device="cuda"), torch.empty((1, nch, k), dtype=torch.uint8, device="cuda"),
                 torch.zeros((1, nch, k * WAVE_BATCH, 2), dtype=torch.float32, device="cuda") if case["iq_rows"] else None) for k in calls]
        torch.cuda.synchronize()
        paths, done = [], 0
        for k, (wo, ax, zo) in zip(calls, outs):
            pos = _pos(d, done)
            d.process_device(d_iq.data_ptr() + pos, pad - pos, k, wo.data_ptr(), ax.data_ptr(), d_iq_out_ptr=None if zo is None else zo.data_ptr(),
                             hip_stream=side.cuda_stream)
            if reading == "drained":
                paths.append(d.last_path())
            done += k
        stage1 = d.last_stage1()
        kernels = [_kernel_names(d, age) for age in (1, 0)]
        paths.append(d.last_path())
        torch.cuda.synchronize()
        timeouts = d.pre_wave_timeouts()
        d.close()
        print(f"{what}: last_path {paths}, last_stage1 {stage1}, pre_wave_timeouts {timeouts}, kernels of the first call {kernels[0]}")
        assert all(p == (1, 0) for p in paths), f"{what}: every call splits: plain AM rows time-parallel, every segment verified"
        assert all("k_tp_core" in k and "k_demod" in k for k in kernels), f"{what}: both calls ran the time-parallel passes and the serial kernel"
        assert timeouts == 0
        ax = torch.cat([o[1] for o in outs], dim=2).cpu().numpy()
        wo = torch.cat([o[0] for o in outs], dim=2).cpu().numpy()
        assert_same(ax[0], oaxc, f"{what}: flags")
        assert_same(wo[0], owo, f"{what}: audio")
        for c in case["iq_rows"]:
            zo = torch.cat([o[2][0, c] for o in outs], dim=0).cpu().numpy()
            assert_same(zo.reshape(-1), oiq[c], f"{what}: raw I/Q, channel {c}")
        del outs


# ---- 2. bench.py --workload config4 -------------------------------------------------------------------------------------------

CONFIG4_IQ_ROWS = (1, 6, 17, 31)


def _digest(res):
    nb, owo, oaxc, oiq = res
    h = hashlib.sha256()
    for a in (owo, oaxc, oiq):
        h.update(np.ascontiguousarray(a).tobytes())
    return nb, h.hexdigest()


def _config4_geometry(pkg, monkeypatch, nstreams, check_threads):
    """`nstreams` streams x the 32-channel plan at fft 512, captures generated on the device (seeded by stream id) with every
    carrier on, three 16-batch device calls back to back on the current stream with MI_OPT_EARLY_INPUT: what run_workload does for
    config4.  Every stream against its own 48-batch oracle run, the oracle runs spread over a small thread pool."""
    import torch
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    calls = [16, 16, 16]
    nbat = sum(calls)
    centre, chans = pkg.config3_channels()
    for c in CONFIG4_IQ_ROWS:
        chans[c].has_iq_outputs = 1
    nch = len(chans)
    nfm = np.array([c.modulation == pkg.MOD_NFM for c in chans])
    ctcss = np.array([c.ctcss_freq > 0 for c in chans])
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=9)
    nbytes = (bytes_for_batches(dev, nbat) + 255) // 256 * 256
    gcfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate // 3,
                         carriers=pkg.carriers_for(centre, chans, amp_q8=768, active=lambda k: True))
    s = torch.cuda.current_stream().cuda_stream
    d_iq = torch.zeros((nstreams, nbytes), dtype=torch.uint8, device="cuda")
    pkg.iqgen_device(gcfg, 0, nstreams, nbytes, 0, nbytes // 2, d_iq.data_ptr(), s)
    outs = [(torch.empty((nstreams, nch, k * WAVE_BATCH), dtype=torch.float32, device="cuda"),
             torch.empty((nstreams, nch, k), dtype=torch.uint8, device="cuda"),
             torch.empty((nstreams, nch, k * WAVE_BATCH, 2), dtype=torch.float32, device="cuda")) for k in calls]
    torch.cuda.synchronize()
    iq_host = d_iq.cpu().numpy()
    assert nstreams == 1 or not np.array_equal(iq_host[0], iq_host[1]), "streams carry different noise"

    d = pkg.Demod(dev, chans, nstreams=nstreams, max_batches=max(calls))
    d.set_option(pkg.OPT_EARLY_INPUT, 1)
    done = 0
    for k, (wo, ax, zo) in zip(calls, outs):  # (no host synchronisation in between: stage 1 of a call runs under k_demod of the one before)
        d.process_device(d_iq.data_ptr() + _pos(d, done), nbytes, k, wo.data_ptr(), ax.data_ptr(), d_iq_out_ptr=zo.data_ptr(), hip_stream=s)
        done += k
    stage1 = d.last_stage1()
    kernels = [_kernel_names(d, age) for age in (2, 1, 0)]
    path = d.last_path()
    torch.cuda.synchronize()
    timeouts = d.pre_wave_timeouts()
    d.close()
    print(f"config4 x {nstreams} streams: last_path {path}, last_stage1 {stage1}, pre_wave_timeouts {timeouts}, kernels per call {kernels}")
    assert path[0] == 0, "the serial kernel for every row"
    assert kernels == [SERIAL_KERNELS] * 3
    assert timeouts == 0
    wo = torch.cat([o[0] for o in outs], dim=2).cpu().numpy()
    ax = torch.cat([o[1] for o in outs], dim=2).cpu().numpy()
    zo = torch.cat([o[2][:, list(CONFIG4_IQ_ROWS)] for o in outs], dim=2).cpu().numpy()
    del outs

    def check_stream(st):
        res = oracle_run(dev, chans, iq_host[st], nbat, want_iq=True)
        nb, owo, oaxc, oiq = res
        assert nb == nbat
        assert_same(ax[st], oaxc, f"config4 x {nstreams}: flags, stream {st}")
        assert_same(wo[st], owo, f"config4 x {nstreams}: audio, stream {st}")
        for i, c in enumerate(CONFIG4_IQ_ROWS):
            assert_same(zo[st, i].reshape(-1), oiq[c], f"config4 x {nstreams}: raw I/Q, stream {st} channel {c}")
        return oaxc, _digest(res) if st < 2 else None

    with ThreadPoolExecutor(ORACLE_THREADS) as pool:
        threaded = list(pool.map(check_stream, range(nstreams)))
    if check_threads:
        # the claim the thread pool rests on: the oracle gives the same bits threaded and alone
        for st in range(2):
            assert _digest(oracle_run(dev, chans, iq_host[st], nbat, want_iq=True)) == threaded[st][1], f"oracle, stream {st}: threaded run differs"
    for st, (oaxc, _) in enumerate(threaded):
        frac, changes, both = _flag_stats(oaxc)
        assert both[nfm].any(), f"stream {st}: some NFM row opens and closes"
        assert both[ctcss].any(), f"stream {st}: some CTCSS row opens and closes"
        if st == 0:
            print(f"config4 x {nstreams} streams, stream 0: open fraction {frac.min():.4f}-{frac.max():.4f} (NFM {frac[nfm].min():.4f}-"
                  f"{frac[nfm].max():.4f}, CTCSS {frac[ctcss].min():.4f}-{frac[ctcss].max():.4f}), flag changes >= {changes.min()}, "
                  f"rows that open and close {int(both.sum())}, clipped bytes {_clipped(iq_host[0])}")
            assert both.all(), "stream 0: all 32 rows open and close"
            assert (frac >= 0.56).all() and (frac <= 0.65).all()
            assert (changes >= 17).all()
            assert _clipped(iq_host[0]) == 0


def test_config4_geometry_64_streams_in_three_overlapping_16_batch_calls(pkg, monkeypatch):
    """bench.py --workload config4 at full width: 64 streams x 32 channels = 2048 rows, one channel per wave beside stage 1 of the
    next call, every NFM + low-pass + CTCSS + notch row open for more than half of the capture."""
    _config4_geometry(pkg, monkeypatch, 64, check_threads=True)


@pytest.mark.parametrize("nstreams", [8, 24])
def test_config4_calls_at_narrower_widths(pkg, monkeypatch, nstreams):
    """The same calls at widths the benchmark does not reach: 8 streams (256 rows: four waves per channel) and 24 streams (768 rows:
    two waves per channel, k_demod_pw2)."""
    _config4_geometry(pkg, monkeypatch, nstreams, check_threads=False)


# ---- 3. the fuzzers of tools/ as seeded tests -----------------------------------------------------------------------------------

def _compare_iq_rows(chans, zo, oiq, what):
    for c, ch in enumerate(chans):
        if ch.has_iq_outputs:
            assert_same(zo[c].reshape(-1), oiq[c], f"{what}: raw I/Q, channel {c}")


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_mixed_plans_equal_the_oracle(pkg, monkeypatch, seed):
    """tools/fuzz_oracle.py for seeds 0-19 (fuzz_plans.mixed_plan, fft 256 .. 2048): the host entry in `per_call`-batch calls against
    the oracle; then the same capture as one 8-batch call with MI_OPT_TIME_PARALLEL = 1, which forces the mixed split wherever the
    plan has a plain AM row: equal to the oracle as well, and split exactly when there is such a row."""
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    dev, chans, iq, nbat, per_call = fuzz_plans.mixed_plan(pkg, seed)
    nplain = sum(fuzz_plans.is_plain_am(pkg, c) for c in chans)
    nb, owo, oaxc, oiq = oracle_run(dev, chans, iq, nbat, want_iq=True)
    assert nb == nbat and not np.isnan(owo).any()
    d = pkg.Demod(dev, chans, max_batches=per_call)
    outs, flags, zs = [], [], []
    for call in range(nbat // per_call):
        wo, ax, zo, _ = d.process([iq[_pos(d, call * per_call):]], per_call, want_iq=True)
        outs.append(wo[:, :, :per_call * WAVE_BATCH].copy())
        flags.append(ax.copy())
        zs.append(zo.copy())
    stage1 = d.last_stage1()
    path = d.last_path()
    d.close()
    what = f"fuzz seed {seed} ({len(chans)} channels, fft {1 << dev.fft_size_log}, {per_call} batches a call)"
    assert_same(np.concatenate(flags, axis=2)[0], oaxc, f"{what}: flags")
    assert_same(np.concatenate(outs, axis=2)[0], owo, f"{what}: audio")
    _compare_iq_rows(chans, np.concatenate(zs, axis=2)[0], oiq, what)
    # second reading: one call, the split forced
    d = pkg.Demod(dev, chans, max_batches=nbat)
    d.set_option(pkg.OPT_TIME_PARALLEL, 1)
    wo, ax, zo, _ = d.process([iq], nbat, want_iq=True)
    forced = d.last_path()
    timeouts = d.pre_wave_timeouts()
    d.close()
    print(f"{what}: {nplain} plain AM rows, last_path {path} / forced {forced}, last_stage1 {stage1}, open batches {(oaxc == STAR).mean():.3f}")
    what += ", one forced call"
    assert forced == ((1, 0) if nplain > 0 else (0, 0)), f"{what}: {nplain} plain AM rows"
    assert timeouts == 0
    assert_same(ax[0], oaxc, f"{what}: flags")
    assert_same(wo[0, :, :nbat * WAVE_BATCH], owo, f"{what}: audio")
    _compare_iq_rows(chans, zo[0], oiq, what)


def test_fuzz_mixed_plans_cover_every_channel_kind(pkg):
    """Oracle only, over the whole seed set: what the mixed-plan fuzz exercises.  Every channel kind has rows that open and close,
    (nearly) no seed is silent, and at least 12 seeds have a plain AM row beside others.  Every seed of
    test_fuzz_mixed_plans_equal_the_oracle asserts that its forced reading splits exactly when the plan has such a row: the two
    assertions together are the claim that at least 12 seeds took the split.  (6 of the 20 seeds land on fft 2048, all with such
    a row.)"""
    kinds = {"NFM": lambda c: c.modulation == pkg.MOD_NFM, "CTCSS": lambda c: c.ctcss_freq > 0, "notch": lambda c: c.notch_freq > 0,
             "manual threshold": lambda c: c.squelch_threshold_dbfs != 0, "raw I/Q": lambda c: bool(c.has_iq_outputs)}
    rows = {k: 0 for k in kinds}
    lively = {k: 0 for k in kinds}
    silent, split, ffts = 0, [], {}
    for seed in FUZZ_SEEDS:
        dev, chans, iq, nbat, _ = fuzz_plans.mixed_plan(pkg, seed)
        nb, owo, oaxc, _ = oracle_run(dev, chans, iq, nbat)
        assert nb == nbat and not np.isnan(owo).any()
        _, _, both = _flag_stats(oaxc)
        silent += int(not (oaxc == STAR).any())
        nplain = sum(fuzz_plans.is_plain_am(pkg, c) for c in chans)
        if 0 < nplain < len(chans):
            split.append(seed)
        ffts[1 << dev.fft_size_log] = ffts.get(1 << dev.fft_size_log, 0) + 1
        for c, b in zip(chans, both):
            for k, has in kinds.items():
                if has(c):
                    rows[k] += 1
                    lively[k] += int(b)
    print(f"mixed-plan fuzz, seeds {FUZZ_SEEDS[0]}-{FUZZ_SEEDS[-1]}: fft sizes {ffts}, rows that open and close "
          + ", ".join(f"{k} {lively[k]} of {rows[k]}" for k in kinds) + f"; silent seeds {silent}; seeds with a split {split}")
    for k in kinds:
        assert lively[k] >= 5, f"{k}: only {lively[k]} of {rows[k]} rows open and close"
    assert silent <= 2
    assert ffts.get(2048, 0) >= 1, "no seed reaches fft 2048"
    assert len(split) >= 12, "too few seeds have a plain AM row beside others: the forced split would hardly run"


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_time_parallel_plans(pkg, monkeypatch, seed):
    """tools/fuzz_tp.py for seeds 0-19 (fuzz_plans.tp_plan: plain AM plans, carriers from under the squelch level to clipping) with
    the oracle as the reference for audio and flags: one 16-batch call (time-parallel), 4-batch calls (serial kernel), overlapping
    device calls with MI_OPT_EARLY_INPUT (option switches varying with the seed), submit / wait with calls in flight; the
    statistics of every reading equal those of the serial one."""
    import torch
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    dev, chans, iq, nbat = fuzz_plans.tp_plan(pkg, seed)
    nb, owo, oaxc, _ = oracle_run(dev, chans, iq, nbat)
    assert nb == nbat and not np.isnan(owo).any()
    what = f"tp fuzz seed {seed} ({len(chans)} channels, fft {1 << dev.fft_size_log})"
    # one call: time-parallel
    d = pkg.Demod(dev, chans, max_batches=nbat)
    wo_a, ax_a, _, _ = d.process([iq], nbat)
    path = d.last_path()
    stage1 = d.last_stage1()
    st_a = bytes(d.stats())
    d.close()
    print(f"{what}: last_path {path}, last_stage1 {stage1}, open batches {(oaxc == STAR).mean():.3f}")
    assert path == (1, 0)
    assert_same(ax_a[0], oaxc, f"{what}, one call: flags")
    assert_same(wo_a[0, :, :nbat * WAVE_BATCH], owo, f"{what}, one call: audio")
    # 4-batch calls: serial kernel
    e = pkg.Demod(dev, chans, max_batches=4)
    outs, flags = [], []
    for call in range(nbat // 4):
        wo, ax, _, _ = e.process([iq[_pos(e, call * 4):]], 4)
        assert e.last_path()[0] == 0
        outs.append(wo[:, :, :4 * WAVE_BATCH].copy())
        flags.append(ax.copy())
    st_b = bytes(e.stats())
    e.close()
    assert_same(np.concatenate(flags, axis=2)[0], oaxc, f"{what}, serial calls: flags")
    assert_same(np.concatenate(outs, axis=2)[0], owo, f"{what}, serial calls: audio")
    assert st_a == st_b, f"{what}: statistics of the time-parallel call differ from the serial calls'"
    # overlapping device calls (the NULL stream, or one of the caller's own: the wide passes then run on the CU-restricted streams)
    pad = (iq.size + 255) // 256 * 256
    d_iq = torch.zeros(pad, dtype=torch.uint8, device="cuda")
    d_iq[:iq.size] = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream() if seed % 3 == 0 else None
    s = side.cuda_stream if side is not None else torch.cuda.current_stream().cuda_stream
    sizes = fuzz_plans.tp_call_sizes(seed)
    assert sum(sizes) == nbat
    f = pkg.Demod(dev, chans, max_batches=max(sizes))
    f.set_option(pkg.OPT_EARLY_INPUT, 1)
    if seed % 5 == 0:
        f.set_option(pkg.OPT_SPEC_HEAD, 0)
    if seed % 7 == 0:
        f.set_option(pkg.OPT_CORE_SPLIT, 0)
    outs, flags, paths, done = [], [], [], 0
    for k in sizes:
        pos = _pos(f, done)
        wo = torch.empty((1, len(chans), k * WAVE_BATCH), dtype=torch.float32, device="cuda")
        ax = torch.empty((1, len(chans), k), dtype=torch.uint8, device="cuda")
        f.process_device(d_iq.data_ptr() + pos, pad - pos, k, wo.data_ptr(), ax.data_ptr(), hip_stream=s)
        outs.append(wo)
        flags.append(ax)
        done += k
    kernels = [_kernel_names(f, age) for age in range(len(sizes))]  # (the calls before the last: read without draining the device first)
    paths.append(f.last_path())
    assert all("k_tp_core" in k for k in kernels), f"{what}, device calls {sizes}: kernels {kernels}"
    torch.cuda.synchronize()
    st_c = bytes(f.stats())
    f.close()
    assert all(p == (1, 0) for p in paths), f"{what}, device calls {sizes}: paths {paths}"
    assert_same(torch.cat(flags, dim=2).cpu().numpy()[0], oaxc, f"{what}, device calls {sizes}: flags")
    assert_same(torch.cat(outs, dim=2).cpu().numpy()[0], owo, f"{what}, device calls {sizes}: audio")
    assert st_c == st_b, f"{what}, device calls {sizes}: statistics"
    # host entry, calls in flight
    g = pkg.Demod(dev, chans, max_batches=8)
    for call in range(2):
        g.submit([iq[_pos(g, call * 8):]], 8)
    r0, r1 = g.wait(), g.wait()
    g.close()
    assert_same(np.concatenate([r0[1], r1[1]], axis=2)[0], oaxc, f"{what}, submit / wait: flags")
    assert_same(np.concatenate([r0[0][:, :, :8 * WAVE_BATCH], r1[0][:, :, :8 * WAVE_BATCH]], axis=2)[0], owo, f"{what}, submit / wait: audio")
    assert bytes(r1[3]) == st_b, f"{what}, submit / wait: statistics"


# ---- 4. a handle gives back what it took ----------------------------------------------------------------------------------------

CHUNK = 2 << 20  # the runtime takes device memory from the driver in pieces of 2 MiB and serves small allocations out of them


def test_create_destroy_returns_the_handle_s_device_memory(pkg):
    """A time-parallel-eligible handle (config2 plan x 64 streams, max_batches = 64: six scratch sets) created and destroyed 50
    times: the free device memory after the loop is within one handle's footprint of what it was after the first create /
    destroy.  That bound alone is far too wide to see a forgotten buffer (a handle's footprint is gigabytes of magnitude planes),
    so the loss must also stay within one 2 MiB piece of the allocator, free memory moving in such pieces: the smallest per-row
    buffer of a handle, the audio lookahead of one scratch set (rows x AGC_EXTRA floats), forgotten once per destroy, costs
    nearly five of them over the 49 further pairs.  (mi_demod_destroy freed the lookahead of four of the six sets: 20 MiB and more
    lost here.  With one stream the two forgotten buffers are 3 200 bytes each and 49 pairs of them vanish inside one piece, so
    the handle is as wide as the am64 plan.)
    Free device memory is a figure of the whole card: another process on it, or a pool the runtime grows for itself, moves it as
    well.  A buffer the handle forgets is lost in every loop of 50, such a movement is not: the loop runs up to three times and
    the smallest loss counts."""
    import torch
    centre, chans = pkg.config2_channels()
    dev = pkg.device_cfg(centerfreq=centre)
    rounds, nstreams, attempts = 50, 64, 3
    smallest = nstreams * len(chans) * AGC_EXTRA * 4
    assert (rounds - 1) * smallest >= 4 * CHUNK, "a forgotten buffer has to show"

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def loop():
        footprint = base = None
        for i in range(rounds):
            before = free_bytes()
            d = pkg.Demod(dev, chans, nstreams=nstreams, max_batches=64)
            if i == 0:
                footprint = before - free_bytes()
            d.close()
            if i == 0:
                base = free_bytes()  # (after the first pair: whatever the runtime keeps for itself once is taken by now)
        return footprint, base - free_bytes()

    torch.zeros(1, device="cuda")
    seen = []
    for _ in range(attempts):
        seen.append(loop())
        print(f"create / destroy x {rounds}: one handle takes {seen[-1][0]} bytes, the {rounds - 1} pairs after the first lost {seen[-1][1]} bytes")
        if seen[-1][1] <= CHUNK:
            break
    footprint, lost = min(seen, key=lambda fl: fl[1])
    assert max(f for f, _ in seen) >= 6 * nstreams * len(chans) * 64 * WAVE_BATCH * 4, "six sets of magnitude planes at least"
    assert lost <= footprint
    assert lost <= CHUNK, f"{lost} bytes of device memory lost over {rounds - 1} create / destroy pairs (every loop: {seen})"


def test_create_destroy_returns_what_a_mixed_handle_took_while_it_ran(pkg, monkeypatch):
    """The same measurement and the same bound as above -- at most one 2 MiB piece lost over the pairs after the first -- on handles
    that have run, so that what a handle creates on its way is in play as well.  Each is a mixed plan (config3 channels x 16 streams,
    max_batches = 64: 512 rows, 256 of them plain AM) and does, before it is destroyed:
      - three 1-batch device calls with MI_OPT_EARLY_INPUT on a stream of the caller's: the first of a handle takes the plain serial
        branch, the two after it overlap (the second complex plane set; with 512 rows the CU-masked pair of streams and their events
        where the device grants them);
      - one 64-batch call, which takes the mixed split (the chunk events of its scratch set, the serial kernel's stream, with
        MI_OPT_RESERVE_CUS the CU-masked twins of the front and segment streams where the device grants them);
      - one submit / wait pair (a staging slot with its pinned buffers and events, the upload and download streams).
    The smallest per-row buffer, the audio lookahead of one scratch set (rows x AGC_EXTRA floats), forgotten once per destroy, costs
    nearly five pieces over the 49 further pairs, as the docstring above argues; a slot's or a plane set's buffers are thousands of
    times that.  The input is the constant byte 0x80 (mi_demod_prepare's rehearsal input): the paths do not depend on the signal."""
    import torch
    monkeypatch.delenv("MI_AIRBAND_TP", raising=False)
    monkeypatch.delenv("MI_AIRBAND_MIXED", raising=False)
    centre, chans = pkg.config3_channels()
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=11)
    rounds, nstreams, attempts, long_call = 50, 16, 3, 64
    nch = len(chans)
    nplain = sum(fuzz_plans.is_plain_am(pkg, c) for c in chans)
    assert 0 < nplain < nch, "a mixed plan"
    smallest = nstreams * nch * AGC_EXTRA * 4
    assert (rounds - 1) * smallest >= 4 * CHUNK, "a forgotten buffer has to show"
    nbytes = (bytes_for_batches(dev, long_call) + 255) // 256 * 256
    d_iq = torch.full((nstreams, nbytes), 0x80, dtype=torch.uint8, device="cuda")
    wo = torch.empty((nstreams, nch, long_call * WAVE_BATCH), dtype=torch.float32, device="cuda")
    ax = torch.empty((nstreams, nch, long_call), dtype=torch.uint8, device="cuda")
    h_iq = np.full(bytes_for_batches(dev, 1), 0x80, np.uint8)
    side = torch.cuda.Stream()

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def run(d):
        d.set_option(pkg.OPT_EARLY_INPUT, 1)
        d.set_option(pkg.OPT_RESERVE_CUS, 32)
        for _ in range(3):
            d.process_device(d_iq.data_ptr(), nbytes, 1, wo.data_ptr(), ax.data_ptr(), hip_stream=side.cuda_stream)
        serial = [_kernel_names(d, age) for age in range(3)]
        d.process_device(d_iq.data_ptr(), nbytes, long_call, wo.data_ptr(), ax.data_ptr(), hip_stream=side.cuda_stream)
        split, path = _kernel_names(d, 0), d.last_path()
        d.submit([h_iq] * nstreams, 1)
        d.wait()
        assert serial == [SERIAL_KERNELS] * 3, serial
        assert path[0] == 1 and "k_tp_core" in split and "k_demod" in split, f"the {long_call}-batch call splits: {path}, {split}"

    def loop():
        footprint = base = None
        for i in range(rounds):
            before = free_bytes()
            d = pkg.Demod(dev, chans, nstreams=nstreams, max_batches=long_call)
            run(d)
            if i == 0:
                footprint = before - free_bytes()
            d.close()
            if i == 0:
                base = free_bytes()  # (after the first pair: whatever the runtime keeps for itself once is taken by now)
        return footprint, base - free_bytes()

    seen = []
    for _ in range(attempts):
        seen.append(loop())
        print(f"mixed handle, create / run / destroy x {rounds}: one handle takes {seen[-1][0]} bytes, the {rounds - 1} pairs after the first lost {seen[-1][1]} bytes")
        if seen[-1][1] <= CHUNK:
            break
    footprint, lost = min(seen, key=lambda fl: fl[1])
    assert max(f for f, _ in seen) >= 6 * nstreams * nch * long_call * WAVE_BATCH * 4, "six sets of magnitude planes at least"
    assert lost <= footprint
    assert lost <= CHUNK, f"{lost} bytes of device memory lost over {rounds - 1} create / run / destroy pairs (every loop: {seen})"
