"""The HIP stage 2 against the oracle's plane entry on adversarial planes, bit for bit, on every path.

The other stage-2 parity tests feed the kernels what mi_iqgen_* generated and stage 1 channelised.  The exactness of the
time-parallel path (csrc/tp.hip) and of the multi-wave serial kernel (csrc/demod.hip) rests on properties of the input that such
signals never stress; tests/plane_cases.py chooses every sample instead (edges on block / group / pass / segment / lead / batch
boundaries, threshold grazing, flapping, lone regime-breaking samples, a stepping noise floor, 10^12 of dynamic range, silence
down to the subnormals), mi_demod_process_planes feeds them to the same kernels along the same paths as mi_demod_process, and
ao_demod_run_planes (tests/test_oracle_planes.py pins it to the IQ entry and to squelch.cpp) says what must come out.

Compared after every call, == up to the sign of zero for audio / raw I/Q / flags and by bits for the levels: the audio with its
AGC_EXTRA lookahead, raw I/Q, per-batch flags, every field of mi_channel_stats; last_path()[1] == 0 and pre_wave_timeouts() == 0.
No tolerance anywhere (the 1e-4 RMS bar is asserted as well)."""
import functools

import numpy as np
import pytest

import libs
import plane_plans as pp
from common import AGC_EXTRA, WAVE_BATCH, assert_same, rms

pytestmark = pytest.mark.gpu

TOL_RMS = 1e-4
NB = 24
CALLS = (9, 1, 11, 3)
ENV = ("MI_AIRBAND_TP", "MI_AIRBAND_TP_SEGMENT", "MI_AIRBAND_CORE_SPLIT", "MI_AIRBAND_CORE_GUESS", "MI_AIRBAND_CORE_LEAN",
       "MI_AIRBAND_CORE_DECAY", "MI_AIRBAND_CORE_LEAD", "MI_AIRBAND_TP_CHUNKS", "MI_AIRBAND_TP_RATIO", "MI_AIRBAND_TP_LPW",
       "MI_AIRBAND_UNI_ROWS", "MI_AIRBAND_STEADY", "MI_AIRBAND_PRE_WAVE", "MI_AIRBAND_AUDIO_WAVE", "MI_AIRBAND_MIXED",
       "MI_AIRBAND_SPEC_HEAD", "MI_AIRBAND_TP_EAGER", "MI_AIRBAND_AGC_HINT")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def set_env(monkeypatch, **env):
    """A handle takes its tuning defaults from the environment when it is created: start from a clean one."""
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv("MI_AIRBAND_" + name, str(value))


@functools.lru_cache(maxsize=None)
def am_reference(name, nbatches, L, calls):
    """(rows, mag, oracle result per call, per row the exact squelch core state before every block of 16 steps)."""
    rows, mag = pp.am_planes(name, nbatches, L)
    res, _ = pp.oracle_calls(libs.device_cfg(centerfreq=pp.CENTRE), pp.am_chans(libs.channel_cfg, rows), mag, None, calls)
    core16 = [libs.oracle_core_trace(mag[r, AGC_EXTRA:], 16, **pp.squelch_kw(st)) for r, (_, _, st) in enumerate(rows)]
    return rows, mag, res, core16


@functools.lru_cache(maxsize=None)
def mixed_reference(nbatches, calls, fm_quadri):
    mag, cplx = pp.mixed_planes(nbatches)
    dev = libs.device_cfg(centerfreq=pp.CENTRE, tau=75, fm_quadri=fm_quadri)
    res, _ = pp.oracle_calls(dev, pp.mixed_chans(libs.channel_cfg), mag, cplx, calls, want_iq=True)
    return mag, cplx, res


def check_call(tag, got, want, has_iq=()):
    """One call's outputs of the HIP path against the oracle's CallResult, rows = streams x channels flattened."""
    wo, axc, iqo, st = got
    rows = want.wo.shape[0]
    n = want.wo.shape[1]
    wo = wo.reshape(rows, n + AGC_EXTRA)
    assert_same(axc.reshape(rows, -1), want.axc, f"{tag}: flags per batch")
    assert_same(wo[:, :n] != 0, want.wo != 0, f"{tag}: per-sample squelch mask")
    worst = max(rms(wo[r, :n] - want.wo[r]) for r in range(rows))
    print(f"{tag}: worst RMS difference of a row's audio {worst:.3g}")
    assert worst <= TOL_RMS
    assert_same(wo[:, :n], want.wo, f"{tag}: audio")
    assert_same(wo[:, n:], want.look, f"{tag}: the AGC_EXTRA lookahead")
    for r in has_iq:
        assert_same(iqo.reshape(rows, -1)[r], want.iqo[r], f"{tag}: raw I/Q of row {r}")
    for r in range(rows):
        for f in libs.STATS_LEVELS:
            g, w = bits([getattr(st[r], f)])[0], bits([getattr(want.stats[r], f)])[0]
            assert g == w, f"{tag}: row {r} {f}: {getattr(st[r], f)!r} vs the oracle's {getattr(want.stats[r], f)!r}"
        for f in libs.STATS_COUNTS:
            assert getattr(st[r], f) == getattr(want.stats[r], f), f"{tag}: row {r} {f}: {getattr(st[r], f)} vs {getattr(want.stats[r], f)}"


def feed(d, mag, cplx, calls, want, tag, has_iq=(), paths=None, options=None, first=0, after_call=None):
    """Run calls[first:] on handle d over the planes (the handle has consumed calls[:first]) and check each against the oracle."""
    at = sum(calls[:first]) * WAVE_BATCH + (AGC_EXTRA if first else 0)
    for ci in range(first, len(calls)):
        k = calls[ci]
        count = k * WAVE_BATCH + (AGC_EXTRA if ci == 0 else 0)
        if options is not None:
            for opt, val in options(ci, k):
                d.set_option(opt, val)
        got = d.process_planes(mag[:, at:at + count], k, cplx=None if cplx is None else cplx[:, at:at + count], want_iq=bool(has_iq))
        path = d.last_path()
        assert path[1] == 0, f"{tag} call {ci}: {path[1]} rows left unverified"
        if paths is not None:
            assert path[0] == paths[ci], f"{tag} call {ci}: stage-2 path {path[0]}, expected {paths[ci]}"
        check_call(f"{tag} call {ci} ({k} batches, path {path[0]})", got, want[ci], has_iq)
        if after_call is not None:
            after_call(ci, at - (AGC_EXTRA if ci else 0), k)
        at += count
    assert d.pre_wave_timeouts() == 0


def check_core(d, rows, core16, start, nsteps, L, tag, table=None):
    """tp_debug after a time-parallel call that began at step `start`: the exact core state at every segment boundary of the call equals
    the oracle's serial trace, and the final scan is clean.  Which scans re-ran segments and whether the serial fallback ran is
    recorded in `table` (a matter of speed: these inputs are meant to defeat the guesses)."""
    for r, (family, seed, setting) in enumerate(rows):
        core, diag = d.tp_debug(r)
        nseg = core.shape[0] - 1
        assert nseg == (nsteps + L - 1) // L
        idx = [(start + min(k * L, nsteps)) // 16 for k in range(nseg + 1)]
        assert_same(bits(core), bits(core16[r][idx]), f"{tag}: core state at the segment boundaries of row {r} ({family} seed {seed}, {setting})")
        assert diag[3] == 0, f"{tag}: row {r}: segments left unverified: {diag.tolist()}"
        if table is not None:
            table.append((family, seed, setting, nseg, diag[:4].tolist()))


def print_table(tag, table):
    print(f"\n{tag}: segments not accepted in scans 0 / 1 / 2 (2: the serial fallback ran) per row")
    for family, seed, setting, nseg, diag in table:
        print(f"  {family:20s} seed {seed:2d} {setting:8s} segments {nseg:3d}  re-run {diag[0]:3d} {diag[1]:3d}  fallback {diag[2]:3d}")


def am_handle(pkg, rows, nstreams, max_batches):
    chans = pp.am_chans(pkg.channel_cfg, rows[:len(rows) // nstreams])
    return pkg.Demod(pkg.device_cfg(centerfreq=pp.CENTRE), chans, nstreams=nstreams, max_batches=max_batches, gpu=0)


# ---------------------------------------------------------------- plain AM, 1 stream x 16 channels (and the two families of their own)
@pytest.mark.parametrize("name", ["am16", "dynamic_range", "silence"])
@pytest.mark.parametrize("steady", [1, 0])
def test_serial_kernel_one_batch_per_call(pkg, monkeypatch, name, steady):
    set_env(monkeypatch)
    calls = (1,) * NB
    rows, mag, want, _ = am_reference(name, NB, 512, calls)
    d = am_handle(pkg, rows, 1, 1)
    d.set_option(pkg.OPT_STEADY_BLOCKS, steady)
    feed(d, mag, None, calls, want, f"{name} serial steady={steady}", paths=[0] * NB)
    d.close()


TP_SWITCHES = ([{"TP_SEGMENT": s} for s in (512, 1024, 2048, 4096)] + [{"CORE_SPLIT": v} for v in (0, 1)] +
               [{"CORE_GUESS": v} for v in (0, 1, 2)] + [{"CORE_LEAN": v} for v in (0, 1)] + [{"CORE_DECAY": 0}] +
               [{"CORE_LEAD": v} for v in (128, 1920)] +
               [{"TP_CHUNKS": c, "TP_RATIO": r, "TP_LPW": w} for c, r, w in ((1, 1, 64), (2, 1, 16), (5, 2, 1), (3, 1.5, 4))])


# the 16-row plan takes every switch; the two families of their own the segment lengths and the ways the chain can walk
TP_CASES = [("am16", s) for s in [{}] + TP_SWITCHES] + [(n, s) for n in ("dynamic_range", "silence") for s in [{}] + TP_SWITCHES
                                                        if not s or "TP_SEGMENT" in s or "CORE_GUESS" in s or "CORE_SPLIT" in s]


@pytest.mark.parametrize("name,switch", TP_CASES, ids=lambda v: v if isinstance(v, str) else ("-".join(f"{k}={x}" for k, x in v.items()) or "default"))
def test_time_parallel_one_call(pkg, monkeypatch, name, switch):
    """One 24-batch call down the time-parallel path, one switch at a time against the default."""
    set_env(monkeypatch, TP=1, **switch)
    L = switch.get("TP_SEGMENT", 512)
    rows, mag, want, core16 = am_reference(name, NB, L, (NB,))
    d = am_handle(pkg, rows, 1, NB)
    tag = f"{name} time-parallel {switch or 'default'}"
    table = []
    feed(d, mag, None, (NB,), want, tag, paths=[1],
         after_call=lambda ci, start, k: check_core(d, rows, core16, start, k * WAVE_BATCH, L, tag, table))
    d.close()
    print_table(tag, table)


@pytest.fixture(scope="module")
def default_call_table(pkg):
    """Per row of the 16-row plan: what tp_debug reports after one 24-batch time-parallel call under the default switches."""
    mp = pytest.MonkeyPatch()
    try:
        set_env(mp, TP=1)
        rows, mag, want, core16 = am_reference("am16", NB, 512, (NB,))
        d = am_handle(pkg, rows, 1, NB)
        table = []
        feed(d, mag, None, (NB,), want, "am16 default switches", paths=[1],
             after_call=lambda ci, start, k: check_core(d, rows, core16, start, k * WAVE_BATCH, 512, "am16 default switches", table))
        d.close()
    finally:
        mp.undo()
    return table


def test_inputs_both_engage_and_avoid_the_serial_fallback(default_call_table):
    """A coverage condition on the inputs that only the device can settle: under the default switches some row of the 16-row plan
    defeats the guesses so thoroughly that the serial fallback runs, and some row is settled by the scans alone."""
    engaged = sorted({f for f, _, _, _, dg in default_call_table if dg[2]})
    avoided = sorted({f for f, _, _, _, dg in default_call_table if not dg[2]})
    print(f"fallback engaged by: {engaged}; avoided by: {avoided}")
    assert engaged, "no row engaged the serial fallback: add a seed that does"
    assert avoided, "every row engaged the serial fallback: add a seed that does not"


@pytest.mark.parametrize("name", ["am16", "dynamic_range", "silence"])
def test_calls_of_9_1_11_3_alternate_paths(pkg, monkeypatch, name):
    set_env(monkeypatch)
    rows, mag, want, core16 = am_reference(name, NB, 512, CALLS)
    d = am_handle(pkg, rows, 1, max(CALLS))
    tag = f"{name} calls {CALLS}"

    def after(ci, start, k):
        if k >= 8:
            check_core(d, rows, core16, start, k * WAVE_BATCH, 512, f"{tag} call {ci}")
    feed(d, mag, None, CALLS, want, tag, paths=[1, 0, 1, 0], after_call=after)
    d.close()


@pytest.mark.parametrize("first_tp", [1, 0])
def test_checkpoint_into_a_handle_on_the_other_path(pkg, monkeypatch, first_tp):
    """get_state after call 2 of (9, 1, 11, 3), set_state into a fresh handle created with the other stage-2 path forced: the
    remaining calls equal the oracle."""
    set_env(monkeypatch, TP=first_tp)
    rows, mag, want, _ = am_reference("am16", NB, 512, CALLS)
    d = am_handle(pkg, rows, 1, max(CALLS))
    feed(d, mag, None, CALLS[:2], want, f"before the checkpoint (TP={first_tp})", paths=[first_tp] * 2)
    state = d.get_state().copy()
    d.close()
    set_env(monkeypatch, TP=1 - first_tp)
    d = am_handle(pkg, rows, 1, max(CALLS))
    d.set_state(state)
    feed(d, mag, None, CALLS, want, f"after the checkpoint (TP={1 - first_tp})", paths=[1 - first_tp] * 4, first=2)
    d.close()


# ---------------------------------------------------------------- 3 streams x 32 channels: every row a different plane
def test_96_rows_time_parallel_long_segments(pkg, monkeypatch):
    """> 64 rows: the row chunking of the time-parallel path and its 1024-step segments; the [nstreams * nch][count] addressing."""
    set_env(monkeypatch, TP=1)
    nb = 16
    rows, mag, want, core16 = am_reference("am96", nb, 1024, (nb,))
    d = am_handle(pkg, rows, 3, nb)
    table = []
    feed(d, mag, None, (nb,), want, "96 rows time-parallel", paths=[1],
         after_call=lambda ci, start, k: check_core(d, rows, core16, start, k * WAVE_BATCH, 1024, "96 rows", table))
    d.close()
    print_table("96 rows, segments of 1024", table)


def test_96_rows_lane_packed_serial_kernel(pkg, monkeypatch):
    set_env(monkeypatch, UNI_ROWS=1)
    nb = 16
    calls = (1,) * nb
    rows, mag, want, _ = am_reference("am96", nb, 1024, calls)
    d = am_handle(pkg, rows, 3, 1)
    feed(d, mag, None, calls, want, "96 rows lane-packed k_demod", paths=[0] * nb)
    d.close()


# ---------------------------------------------------------------- the mixed plan: rows with raw I/Q beside plain AM rows
MIXED_NB = 64
MIXED_IQ_ROWS = (3, 5, 6)  # channels of pp.mixed_chans with has_iq_outputs


def mixed_handle(pkg, max_batches, fm_quadri=0):
    chans = pp.mixed_chans(pkg.channel_cfg, pkg.MOD_NFM)
    return pkg.Demod(pkg.device_cfg(centerfreq=pp.CENTRE, tau=75, fm_quadri=fm_quadri), chans, nstreams=1, max_batches=max_batches, gpu=0)


@pytest.mark.parametrize("per_call", [1, 5])
@pytest.mark.parametrize("pre_wave,audio_wave", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_mixed_plan_serial_kernel_waves(pkg, monkeypatch, per_call, pre_wave, audio_wave):
    set_env(monkeypatch)
    nb = 20
    calls = (per_call,) * (nb // per_call)
    mag, cplx, want = mixed_reference(nb, calls, 0)
    d = mixed_handle(pkg, per_call)
    d.set_option(pkg.OPT_PRE_WAVE, pre_wave)
    d.set_option(pkg.OPT_AUDIO_WAVE, audio_wave)
    feed(d, mag, cplx, calls, want, f"mixed plan, {per_call} per call, pre_wave={pre_wave} audio_wave={audio_wave}", MIXED_IQ_ROWS, paths=[0] * len(calls))
    d.close()


@pytest.mark.parametrize("fm_quadri", [0, 1])
@pytest.mark.parametrize("mixed", [1, 0])
def test_mixed_plan_one_64_batch_call(pkg, monkeypatch, mixed, fm_quadri):
    """MI_OPT_MIXED_PLAN 1: the plain AM rows time-parallel, the rest serial, side by side in one call; 0: every row serial."""
    set_env(monkeypatch)
    mag, cplx, want = mixed_reference(MIXED_NB, (MIXED_NB,), fm_quadri)
    d = mixed_handle(pkg, MIXED_NB, fm_quadri)
    d.set_option(pkg.OPT_MIXED_PLAN, mixed)
    feed(d, mag, cplx, (MIXED_NB,), want, f"mixed plan, one call, MIXED_PLAN={mixed} fm_quadri={fm_quadri}", MIXED_IQ_ROWS, paths=[mixed])
    st = d.stats()
    assert st[4].ctcss_count > 0 and st[4].no_ctcss_count > 0, "the CTCSS row hears its tone and misses it"
    d.close()
