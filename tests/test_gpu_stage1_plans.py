"""Stage 1 on the GPU at the plans of tests/stage1_plans.py: hop 128 and 160, N = 512 / 1024 / 2048, the edge bins, one channel,
8 .. 64 live classes on both sides of every threshold of Geo::round_windows, 64 channels that all need raw I/Q, and 65.  Each
handle -- the plan-compiled lane kernel, its prebuilt full-graph instance and the exchange kernel -- runs two calls of one batch
and its planes are read back after each: every magnitude plane and the complex plane of every NFM channel equal the oracle's
stage 1 bit for bit, and stay within STAGE1_BOUND of the float64 model (redundant once the equality holds: it says which side
moved when it does not).  tests/test_oracle_stage1_plans.py holds the oracle to the same model on the same inputs."""
import numpy as np
import pytest

import signal_model as sm
import stage1_plans as sp
from common import AGC_EXTRA, WAVE_BATCH

pytestmark = pytest.mark.gpu

CASES = [(rate, log2n, name) for rate in sp.RATES for log2n in sp.SIZES for name in sp.PLAN_NAMES]


def _same(got, want, what, bins, first_window):
    """Bit-exact up to the sign of zero, like common.assert_same, naming the channel and the window of the first difference.
    got / want: [nch][windows] or [nch][windows][2]."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        c, w = int(bad[0][0]), int(bad[0][1])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, first at channel {c} (bin {bins[c]}), window {first_window + w}: "
                             f"{got[c, w]!r} vs {want[c, w]!r}")


def _within_bound(what, model, win, mag, z, nfm, bins):
    """mag [nch][NWIN], z [nch][NWIN][2] (NaN where the planes no longer hold the window) against the model on `win`."""
    e_iq, e_mag, scale = sp.residuals(model, mag[:, win], z[:, win], nfm)
    if not (e_iq <= sp.STAGE1_BOUND and e_mag <= sp.STAGE1_BOUND):
        d = np.abs(mag[:, win].astype(np.float64) - np.abs(model))
        c, k = np.unravel_index(int(np.nanargmax(np.where(np.isnan(d), np.inf, d))), d.shape)
        raise AssertionError(f"{what}: complex {e_iq:.3e}, magnitude {e_mag:.3e} of the model's RMS {scale:.4g}, bound {sp.STAGE1_BOUND:.3e}; "
                             f"largest magnitude residual at channel {c} (bin {bins[c]}), window {int(win[k])}")
    return e_iq, e_mag


def _run_handle(pkg, what, dev, chans, bins, raws, options, omags, ozs, models, win):
    """Two 1-batch host-entry calls on len(raws) streams; after each, the planes and the carried entries against the oracle's
    windows of that call, then the whole of what was read against the model.  Returns the stage-1 kind the calls reported."""
    nch, ns = len(chans), len(raws)
    nfm = [c.modulation == pkg.MOD_NFM for c in chans]
    d = pkg.Demod(dev, chans, nstreams=ns, max_batches=1)
    for k, v in options.items():
        d.set_option(getattr(pkg, k), v)
    gmag = np.full((ns, nch, sp.NWIN), np.nan, np.float32)
    gz = np.full((ns, nch, sp.NWIN, 2), np.nan, np.float32)
    kinds, done = set(), 0
    for call, nw in enumerate(sp.CALLS):
        pos = done * d.hop_bytes
        _, axc, _, _ = d.process([r[pos:] for r in raws], 1)
        kinds.add(d.last_stage1())
        assert (axc == ord(" ")).all(), f"{what}, call {call}: a squelch opened: {bytes(axc.reshape(-1))!r}"
        # the planes now hold [the AGC_EXTRA carried entries | this call's windows from AGC_EXTRA on]
        lo, hi = done + nw - WAVE_BATCH, done + nw
        for s in range(ns):
            carry_m = np.zeros((nch, AGC_EXTRA), np.float32)
            carry_z = np.zeros((nch, AGC_EXTRA, 2), np.float32)
            for c in range(nch):
                m, z = d.read_planes(s, c, AGC_EXTRA, WAVE_BATCH, want_iq=nfm[c])
                gmag[s, c, lo:hi] = m
                cm, cz = d.read_planes(s, c, 0, AGC_EXTRA, want_iq=nfm[c])
                carry_m[c] = cm
                if nfm[c]:
                    gz[s, c, lo:hi] = z
                    carry_z[c] = cz
            rows = [c for c in range(nch) if nfm[c]]
            tag = f"{what}, stream {s}, call {call}"
            _same(gmag[s, :, lo:hi], omags[s][:, lo:hi], f"{tag}: magnitude planes", bins, lo)
            _same(carry_m, omags[s][:, hi - AGC_EXTRA:hi], f"{tag}: carried magnitudes", bins, hi - AGC_EXTRA)
            _same(gz[s, rows, lo:hi], ozs[s][rows, lo:hi], f"{tag}: complex planes", [bins[c] for c in rows], lo)
            _same(carry_z[rows], ozs[s][rows, hi - AGC_EXTRA:hi], f"{tag}: carried complex entries", [bins[c] for c in rows], hi - AGC_EXTRA)
        done += nw
    assert d.pre_wave_timeouts() == 0
    d.close()
    assert len(kinds) == 1, f"{what}: the two calls ran different stage-1 kernels: {kinds}"
    for s in range(ns):
        assert all(np.nanmax(gmag[s, c]) > 0 for c in range(nch)), f"{what}, stream {s}: an all-zero magnitude plane"
        _within_bound(f"{what}, stream {s}: planes against the float64 model", models[s], win, gmag[s], gz[s], nfm, bins)
    return kinds.pop()


def _case(pkg, rate, log2n, name, sfmt="u8", seeds=(1,), variants=tuple(sp.VARIANTS)):
    freqs, mods, bins = sp.plan(name, rate, log2n)
    dev = sp.device(pkg.device_cfg, rate, log2n, sfmt)
    chans = sp.channels(pkg.channel_cfg, freqs, mods)
    sp.assert_bins(pkg, dev, chans, bins)
    raws = [sp.capture(rate, log2n, freqs, seed=s, sfmt=sfmt) for s in seeds]
    assert all(not np.array_equal(raws[0], r) for r in raws[1:])
    win = sp.subset_windows()
    win = win[win >= AGC_EXTRA]  # the first AGC_EXTRA windows of the first call are overwritten by the carried ones
    omags, ozs, models = [], [], []
    for raw in raws:  # the references, once per capture, shared by the variants
        m, z = sp.oracle_planes(dev, chans, raw)
        omags.append(m), ozs.append(z)
        models.append(sp.model_planes(dev, chans, raw, win))
        assert sm.rms(models[-1]) > 0 and all(np.abs(m[c]).max() > 0 for c in range(len(chans)))
    ran = {}
    for variant in variants:
        what = f"{rate} S/s, fft {1 << log2n}, {sfmt}, {name}, {variant}"
        kind = _run_handle(pkg, what, dev, chans, bins, raws, sp.VARIANTS[variant], omags, ozs, models, win)
        assert kind == sp.expected_kind(variant, name, log2n), f"{what}: the handle ran stage-1 kernel kind {kind}"
        ran[variant] = kind
    print(f"stage 1 on the GPU: {rate} S/s (hop {sm.hop_of(rate)}), fft {1 << log2n}, {sfmt}, {name}: {len(chans)} channels, "
          f"{sp.live_classes(bins)} live classes, {len(raws)} stream(s); kinds that ran: {ran}")


@pytest.mark.parametrize("rate,log2n,name", CASES, ids=[f"{r}-{1 << l}-{n}" for r, l, n in CASES])
def test_planes_equal_the_oracle_and_the_model(pkg, rate, log2n, name):
    _case(pkg, rate, log2n, name)


def test_three_streams_of_64_classes_at_hop_128(pkg):
    """all64 at N = 1024, hop 128, three streams with captures of their own: runs of tiles cross from one stream into the
    next, and each stream equals its own oracle run."""
    _case(pkg, sp.RATES[0], 10, "all64", seeds=(1, 2, 3))


@pytest.mark.parametrize("sfmt,log2n", [("s8", 9), ("s16", 10), ("f32", 11)])
def test_wider_formats_at_hop_128(pkg, sfmt, log2n):
    """The edge bins at hop 128 in s8 / s16 / f32 (the other format tests all run hop 160)."""
    _case(pkg, sp.RATES[0], log2n, "edges", sfmt=sfmt)
