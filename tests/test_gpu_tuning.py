"""The two routes to a tuning switch end at the same handle: one created under MI_AIRBAND_<NAME> and one created with a clean
environment and the matching mi_demod_set_option take the same stage-2 path and the same stage-1 kernel, and both equal the oracle
bit for bit.  (tests/test_tuning.py pins how the values are normalised, without a GPU; the other GPU tests steer by the variables.)"""
import os

import pytest

from common import WAVE_BATCH, assert_same, gen_iq, oracle_run

NBAT = 8  # the shortest call the time-parallel path takes by itself


@pytest.fixture(scope="module")
def case(pkg):
    centre, chans = pkg.config2_channels()  # 8 AM channels
    dev = pkg.device_cfg(centerfreq=centre)  # fft 512
    iq, _ = gen_iq(pkg, dev, centre, chans, NBAT, gate_div=2)
    nb, owo, oaxc, _ = oracle_run(dev, chans, iq, NBAT)
    assert nb == NBAT and (oaxc == ord("*")).any() and (oaxc != ord("*")).any()
    return dev, chans, iq, owo, oaxc


# (variable, its text, option, its value, stage-2 path, stage-1 kinds): MI_STAGE1_* 3 = the plan's own lane kernel, 2 = the full-graph
# lane kernel, 1 / 0 = the exchange kernels (pruned where the plan prunes)
SWITCHES = [
    ("MI_AIRBAND_TP", "0", "OPT_TIME_PARALLEL", 0, 0, (3,)),
    ("MI_AIRBAND_TP", "1", "OPT_TIME_PARALLEL", 1, 1, (3,)),
    ("MI_AIRBAND_L64", "0", "OPT_LANE_FFT", 0, 1, (0, 1)),
    ("MI_AIRBAND_L64_JIT", "0", "OPT_LANE_FFT_JIT", 0, 1, (2,)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("var,text,option,value,path,kinds", SWITCHES, ids=[f"{s[0]}={s[1]}" for s in SWITCHES])
def test_environment_and_option_routes_agree(pkg, case, monkeypatch, var, text, option, value, path, kinds):
    dev, chans, iq, owo, oaxc = case
    for k in [k for k in os.environ if k.startswith("MI_AIRBAND_")]:
        monkeypatch.delenv(k)
    seen = []
    for route in ("environment", "option"):
        if route == "environment":
            monkeypatch.setenv(var, text)
        else:
            monkeypatch.delenv(var)
        d = pkg.Demod(dev, chans, nstreams=1, max_batches=NBAT, gpu=0)
        if route == "option":
            d.set_option(getattr(pkg, option), value)
        wo, axc, _, _ = d.process([iq], NBAT)
        seen.append((d.last_path(), d.last_stage1()))
        d.close()
        print(f"{var}={text} by {route}: path {seen[-1][0]}, stage 1 kind {seen[-1][1]}")
        assert_same(axc[0], oaxc, f"{var}={text} by {route}: flags")
        assert_same(wo[0, :, :NBAT * WAVE_BATCH], owo, f"{var}={text} by {route}: audio")
    assert seen[0] == seen[1], seen
    assert seen[0][0] == (path, 0) and seen[0][1] in kinds, seen
