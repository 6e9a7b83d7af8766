"""The reference side of tests/test_gpu_stage1_plans.py, without a GPU: at hop 128 and 160, N = 512 / 1024 / 2048, the edge
bins, 1 .. 64 live classes and 65 channels, the oracle's stage 1 stays within STAGE1_BOUND of the float64 signal model (the
DFT definition, one bin per channel as a dot product), and the plan derives the lane-resident stage 1 the GPU tests expect to
run: on for every list of up to 64 channels with exactly the intended number of live classes, off for 65."""
import numpy as np
import pytest

import libs
import signal_model as sm
import stage1_plans as sp

CASES = [(rate, log2n, name) for rate in sp.RATES for log2n in sp.SIZES for name in sp.PLAN_NAMES]


def _oracle_against_model(rate, log2n, name, sfmt="u8"):
    freqs, mods, bins = sp.plan(name, rate, log2n)
    dev = sp.device(libs.device_cfg, rate, log2n, sfmt)
    chans = sp.channels(libs.channel_cfg, freqs, mods)
    n = 1 << log2n
    assert [libs.oracle_lib().ao_bin_for_freq(f, sp.CENTRE, rate, n) for f in freqs] == bins
    raw = sp.capture(rate, log2n, freqs, sfmt=sfmt)
    mag, z = sp.oracle_planes(dev, chans, raw)
    win = sp.subset_windows()
    model = sp.model_planes(dev, chans, raw, win)
    e_iq, e_mag, scale = sp.residuals(model, mag[:, win], z[:, win], [True] * len(chans))
    print(f"stage 1, oracle vs float64 model: {rate} S/s, fft {n}, {sfmt}, {name}: {len(chans)} channels, {sp.live_classes(bins)} classes, "
          f"complex {e_iq:.3e}, magnitude {e_mag:.3e} of the model's RMS {scale:.4g}")
    assert all(np.abs(mag[c]).max() > 0 for c in range(len(chans)))
    # what the GPU cases rely on: no magnitude reaches the -1 dBFS squelch level, and the oracle's whole chain opens nothing
    level = libs.oracle_lib().ao_dbfs_to_level(-1.0, n)
    assert mag.max() < 0.95 * level, f"largest magnitude {mag.max():.4g} against the squelch level {level:.4g}"
    if sfmt == "u8":
        od = libs.OracleDemod(dev, chans)
        nb, _, axc, _ = od.run(raw, 2)
        od.close()
        assert nb == 2 and (axc == ord(" ")).all(), bytes(axc.reshape(-1))
    assert e_iq <= sp.STAGE1_BOUND and e_mag <= sp.STAGE1_BOUND, (e_iq, e_mag)
    return dev, chans, bins


@pytest.mark.parametrize("rate,log2n,name", CASES, ids=[f"{r}-{1 << l}-{n}" for r, l, n in CASES])
def test_oracle_stage1_and_plan_derivation(pkg, rate, log2n, name):
    _, _, bins = _oracle_against_model(rate, log2n, name)
    freqs, mods, _ = sp.plan(name, rate, log2n)
    dev = sp.device(pkg.device_cfg, rate, log2n)
    chans = sp.channels(pkg.channel_cfg, freqs, mods)
    sp.assert_bins(pkg, dev, chans, bins)
    p = pkg.Plan(dev, chans)
    enabled, need, lanes, slots, _ = p.lane_fft()
    p.close()
    if name == "over":
        assert len(chans) == 65 and not enabled
        return
    assert enabled and lanes == (1 << log2n) // 64
    want = {"one": 1, "all64": 64, "all64_iq": 64}.get(name)
    if name.startswith("classes"):
        want = int(name[len("classes"):])
    if want is None:  # edges: {0, 1, 62, 63} and the mid-band class
        want = 5
    assert sp.live_classes(bins) == want
    assert bin(need[5]).count("1") == want, f"need[5] = {need[5]:#x}"
    classes = sorted({b % 64 for b in bins})
    assert slots.tolist() == [classes.index(b % 64) for b in bins]


def test_named_edge_frequencies_map_to_the_recorded_bins(pkg):
    """centre, centre + 1, centre +- spacing, centre +- rate / 2 and centre - rate / 2 + 1 by the oracle, the plan and the model."""
    for rate in sp.RATES:
        for log2n in sp.SIZES:
            n = 1 << log2n
            dev = sp.device(pkg.device_cfg, rate, log2n)
            named = sp.named_edges(rate, log2n)
            for _, f, b in named:
                assert libs.oracle_lib().ao_bin_for_freq(f, sp.CENTRE, rate, n) == b
            sp.assert_bins(pkg, dev, sp.channels(pkg.channel_cfg, [f for _, f, _ in named], [0] * len(named)), [b for _, _, b in named])


def test_the_lists_cover_every_kernel_kind_and_round_regime():
    """What the GPU cases assert per handle adds up to: all four stage-1 kinds, both exchange kernels at N = 512, and 1, 8, 9,
    16, 17, 32, 33 and 64 live classes at both hops and all three sizes."""
    for rate in sp.RATES:
        for log2n in sp.SIZES:
            counts = {sp.live_classes(sp.plan(name, rate, log2n)[2]) for name in sp.PLAN_NAMES if name != "over"}
            assert counts >= {1, 8, 9, 16, 17, 32, 33, 64}, (rate, log2n, counts)
    kinds = {sp.expected_kind(v, name, l) for v in sp.VARIANTS for name in sp.PLAN_NAMES for l in sp.SIZES}
    assert kinds == {0, 1, 2, 3}
    assert {sp.expected_kind("exchange kernel", name, 9) for name in sp.PLAN_NAMES} == {0, 1}


@pytest.mark.parametrize("sfmt", ["s8", "s16", "f32"])
def test_oracle_stage1_wider_formats_at_hop_128(sfmt):
    for log2n in sp.SIZES:
        _oracle_against_model(sp.RATES[0], log2n, "edges", sfmt)
