"""The lane-resident stage 1 as the plan derives it (mi_plan_lane_fft, no GPU needed): which residues of the picked bins stay
live through the six in-lane stages, where a channel's class sits among the live ones, and the twiddles of the combining stages
7 .. log2 N -- each checked against a brute-force restatement from the channels' bins and the plan's own twiddle table."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_channels(pkg, rng, centre, rate):
    nch = int(rng.integers(1, 65))
    chans = []
    for _ in range(nch):
        f = centre + int(rng.integers(-rate // 2 + 20000, rate // 2 - 20000))
        chans.append(pkg.channel_cfg(f, modulation=pkg.MOD_NFM if rng.integers(0, 2) else pkg.MOD_AM))
    return chans


@pytest.mark.parametrize("log2n", [9, 10, 11])
def test_lane_fft_derivation_equals_brute_force(pkg, log2n):
    centre = 120000000
    n = 1 << log2n
    for seed in range(20):
        rng = np.random.default_rng(1000 * log2n + seed)
        rate = 2560000 if seed % 4 else 2048000  # hop 160 and, every fourth list, hop 128
        dev = pkg.device_cfg(sample_rate=rate, centerfreq=centre, fft_size_log=log2n)
        chans = _random_channels(pkg, rng, centre, rate)
        p = pkg.Plan(dev, chans)
        enabled, need, lanes, slots, tw = p.lane_fft()
        table = p.twiddles().view(np.uint32)
        bins = [int(p.channel(i).bin) for i in range(len(chans))]
        p.close()
        assert enabled, f"seed {seed}: {len(chans)} channels at fft {n}, rate {rate}"
        assert lanes == n // 64
        for s in range(1, 7):
            want = 0
            for b in bins:
                want |= 1 << (b % (1 << s))
            assert need[s - 1] == want, f"seed {seed}: need[{s - 1}] = {need[s - 1]:#x}, expected {want:#x}"
        classes = sorted({b % 64 for b in bins})
        assert slots.tolist() == [classes.index(b % 64) for b in bins]
        assert tw.shape == (len(chans), log2n - 6, 2)
        got = tw.view(np.uint32)
        for i, b in enumerate(bins):
            for s in range(7, log2n + 1):
                e = (b % (1 << (s - 1))) * n // (1 << s)
                want = table[e].copy()
                if (b >> (s - 1)) & 1:
                    want ^= np.uint32(0x80000000)  # negated: the upper output of the stage
                assert got[i, s - 7].tolist() == want.tolist(), f"seed {seed}: channel {i} (bin {b}), stage {s}"


def test_lane_fft_is_off_where_the_plan_does_not_allow_it(pkg):
    centre = 120000000
    some = [pkg.channel_cfg(centre + 25000 * k) for k in range(1, 9)]
    cases = [(pkg.device_cfg(centerfreq=centre, fft_size_log=l), some, f"fft 2^{l}") for l in (8, 12, 13)]
    for l in (9, 10, 11):
        dev = pkg.device_cfg(centerfreq=centre, fft_size_log=l)
        cases.append((dev, [pkg.channel_cfg(centre + 100000, afc=1)] + some, f"afc at 2^{l}"))
        cases.append((dev, [pkg.channel_cfg(centre - 1000000 + 30000 * k) for k in range(65)], f"65 channels at 2^{l}"))
        cases.append((pkg.device_cfg(sample_rate=2400000, centerfreq=centre, fft_size_log=l), some, f"2.4 MS/s at 2^{l}"))
    for dev, chans, what in cases:
        p = pkg.Plan(dev, chans)
        enabled, need, lanes, slots, tw = p.lane_fft()
        p.close()
        assert not enabled, what
        assert need == [0] * 6 and lanes == 0 and not slots.any() and not tw.any(), what
    # ... and the same lists are on where nothing stands in the way
    for l in (9, 10, 11):
        p = pkg.Plan(pkg.device_cfg(centerfreq=centre, fft_size_log=l), some)
        assert p.lane_fft()[0]
        p.close()


def test_committed_twiddle_literals_are_the_generators_output(tmp_path):
    """csrc/tw64.inc is generated (tools/gen_tw64.py) and committed; a stale or hand-edited copy would only show at run time,
    as a plan that quietly loses the lane kernel."""
    fresh = tmp_path / "tw64.inc"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tw64.py"), str(fresh)], check=True, capture_output=True)
    committed = os.path.join(ROOT, "boondock-airband_amd", "csrc", "tw64.inc")
    assert open(fresh).read() == open(committed).read()
