"""The lane-resident stage 1 at fft_size 1024 and 2048 (l64_kernel.h with 16 / 32 lanes per window): the same radix-2 DIT graph
as the exchange kernel and the oracle, so every output is compared bit for bit -- per instantiation, on the planes, for the
other sample formats, over many streams with a tail tile, and for the plans that must keep falling back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import libs
from common import AGC_EXTRA, WAVE_BATCH, assert_same, bytes_for_batches, gen_iq, oracle_run, to_oracle_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VARIANTS = {
    # name: (options, the MI_STAGE1_* kind the handle must report)
    "lane-resident, compiled for the plan (default)": ({}, 3),
    "lane-resident, prebuilt full graph": ({"OPT_LANE_FFT_JIT": 0}, 2),
    "exchange kernel": ({"OPT_LANE_FFT": 0}, 0),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("log2n", [10, 11])
def test_stage1_instantiations_keep_every_bit_at_1024_and_2048(pkg, log2n, variant):
    """Audio, flags and raw I/Q equal the oracle for the plan-compiled lane kernel, its prebuilt full-graph instance and the
    exchange kernel, on the 8-channel AM plan and the 32-channel mixed plan, in calls of 6 and of 1 + 5 batches; the handle
    reports the kernel it ran.  The captures open AM rows and NFM rows in the oracle itself (asserted), so nothing passes on
    silence."""
    opts, kind = VARIANTS[variant]
    am_open = nfm_open = False
    for name in ("config2", "config3"):
        centre, chans = getattr(pkg, name + "_channels")()
        if name == "config3":
            for c in (1, 6, 17):
                chans[c].has_iq_outputs = 1
        dev = pkg.device_cfg(centerfreq=centre, fft_size_log=log2n)
        nbat = 6
        kw = {} if name == "config2" else dict(amp_q8=1024, active=lambda k: k % 4 != 2)
        iq, _ = gen_iq(pkg, dev, centre, chans, nbat, gate_div=2, **kw)
        nb, owo, oaxc, oiq = oracle_run(dev, chans, iq, nbat, want_iq=True)
        assert nb == nbat
        opened = (oaxc == ord("*")).any(axis=1)
        am_open = am_open or any(opened[i] for i, c in enumerate(chans) if c.modulation == pkg.MOD_AM)
        nfm_open = nfm_open or any(opened[i] for i, c in enumerate(chans) if c.modulation == pkg.MOD_NFM)
        if name == "config3":
            assert am_open and nfm_open, "the oracle must open an AM row and an NFM row on these captures"
        for calls in ([6], [1, 5]):
            d = pkg.Demod(dev, chans, max_batches=max(calls))
            for k, v in opts.items():
                d.set_option(getattr(pkg, k), v)
            outs, flags, iqs, done = [], [], [], 0
            for k in calls:
                pos = 0 if done == 0 else (done * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
                wo, axc, iqo, _ = d.process([iq[pos:]], k, want_iq=True)
                outs.append(wo[:, :, :k * WAVE_BATCH]), flags.append(axc), iqs.append(iqo)
                done += k
            got = d.last_stage1()
            d.close()
            assert got == kind, f"{variant}, fft {1 << log2n}: the handle ran stage-1 kernel kind {got}"
            wo, axc, iqo = np.concatenate(outs, axis=2), np.concatenate(flags, axis=2), np.concatenate(iqs, axis=2)
            assert_same(axc[0], oaxc, f"{variant}, {name}, calls {calls}: flags")
            assert_same(wo[0], owo, f"{variant}, {name}, calls {calls}: audio")
            for c, ch in enumerate(chans):
                if ch.has_iq_outputs:
                    assert_same(iqo[0, c].reshape(-1), oiq[c], f"{variant}, {name}, calls {calls}: raw I/Q ch{c}")


@pytest.mark.parametrize("log2n", [10, 11])
def test_planes_equal_the_oracles_stage1(pkg, log2n):
    """Magnitude and complex planes after one 3-batch call equal the oracle's stage 1 on the same bytes for every channel of
    the 32-channel plan.  Stage 2 rewrites the planes of a raw-I/Q channel while its squelch sees a signal
    (rtl_airband.cpp:532-546), so the NFM channels get no carrier and a manual squelch level they cannot reach: their bins,
    their rows in the complex plane -- all stage 1 knows of a channel -- are those of the plan as it stands."""
    centre, chans = pkg.config3_channels()
    for c in chans:
        if c.modulation == pkg.MOD_NFM:
            c.squelch_threshold_dbfs = -1
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=log2n)
    nbat = 3
    iq, _ = gen_iq(pkg, dev, centre, chans, nbat, gate_div=8, amp_q8=1024, active=lambda k: k % 2 == 0)
    nfft = nbat * WAVE_BATCH + AGC_EXTRA
    odev, ochans = to_oracle_cfg(dev, chans)
    od = libs.OracleDemod(odev, ochans)
    omag, oiq = od.stage1(iq, nfft)
    od.close()
    assert all(np.abs(omag[c]).max() > 0 for c in range(len(chans)))
    d = pkg.Demod(dev, chans, max_batches=nbat)
    d.process([iq], nbat)
    assert d.last_stage1() == 3
    # after the call the plane holds [carry(100) | ...]: indices AGC_EXTRA .. still hold this call's windows
    planes = [d.read_planes(0, c, AGC_EXTRA, nfft - AGC_EXTRA, want_iq=True) for c in range(len(chans))]
    carry = [d.read_planes(0, c, 0, AGC_EXTRA, want_iq=True) for c in range(len(chans))]
    d.close()
    for c, ch in enumerate(chans):
        assert_same(planes[c][0], omag[c, AGC_EXTRA:], f"magnitude plane ch{c}")
        assert_same(carry[c][0], omag[c, nfft - AGC_EXTRA:], f"carried magnitudes ch{c}")
        if ch.modulation == pkg.MOD_NFM:
            assert_same(np.asarray(planes[c][1]).reshape(-1, 2), oiq[c, AGC_EXTRA:], f"complex plane ch{c}")


@pytest.mark.parametrize("sfmt", ["s8", "s16", "f32"])
@pytest.mark.parametrize("misalign", [0, 1])
def test_formats_and_odd_alignment_at_2048(pkg, sfmt, misalign):
    """s8 / s16 / f32 samples and a capture that starts on an odd sample, at N = 2048: the lane kernel and the exchange kernel
    (which the other tests pin to the oracle) agree on planes, audio and flags."""
    import torch
    centre, chans = pkg.config2_channels()
    chans[2].has_iq_outputs = 1
    chans[2].bandwidth = 8000
    code = {"s8": pkg.SFMT_S8, "s16": pkg.SFMT_S16, "f32": pkg.SFMT_F32}[sfmt]
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=11, sfmt=code, fullscale={"s8": 127.5, "s16": 32767.0, "f32": 1.0}[sfmt])
    nbat = 3
    u8, _ = gen_iq(pkg, pkg.device_cfg(centerfreq=centre, fft_size_log=11), centre, chans, nbat, gate_div=8)
    x = u8.astype(np.float32) - 127.5
    raw = {"s8": lambda: np.round(x - 0.5).astype(np.int8), "s16": lambda: np.round(x * 200.0).astype(np.int16),
           "f32": lambda: (x / 128.0).astype(np.float32)}[sfmt]()
    bps2 = 2 * raw.itemsize
    pad = np.zeros(2 * misalign, raw.dtype)  # one complex sample in front: the capture then starts on an odd sample
    buf = np.concatenate([pad, raw, np.zeros(64, raw.dtype)]).view(np.uint8)
    d_buf = torch.from_numpy(buf).cuda()
    base = d_buf.data_ptr() + misalign * bps2
    assert base % bps2 == 0 and (base % (2 * bps2) != 0) == bool(misalign)
    res = {}
    for lane_fft in (1, 0):
        d = pkg.Demod(dev, chans, max_batches=nbat)
        d.set_option(pkg.OPT_LANE_FFT, lane_fft)
        d_wo = torch.zeros((1, len(chans), nbat * WAVE_BATCH), dtype=torch.float32, device="cuda")
        d_ax = torch.zeros((1, len(chans), nbat), dtype=torch.uint8, device="cuda")
        d_zo = torch.zeros((1, len(chans), nbat * WAVE_BATCH, 2), dtype=torch.float32, device="cuda")
        d.process_device(base, 0, nbat, d_wo.data_ptr(), d_ax.data_ptr(), d_iq_out_ptr=d_zo.data_ptr(), hip_stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert d.last_stage1() == (3 if lane_fft else 0)
        planes = [d.read_planes(0, c, 0, nbat * WAVE_BATCH + AGC_EXTRA, want_iq=True) for c in range(len(chans))]
        d.close()
        res[lane_fft] = (d_wo.cpu().numpy(), d_ax.cpu().numpy(), d_zo.cpu().numpy(), planes)
    assert (res[0][1] == ord("*")).any()
    assert_same(res[1][0], res[0][0], "audio")
    assert_same(res[1][1], res[0][1], "flags")
    assert_same(res[1][2][0, 2], res[0][2][0, 2], "raw I/Q")
    for c in range(len(chans)):
        assert_same(res[1][3][c][0], res[0][3][c][0], f"magnitude plane ch{c}")
    assert_same(res[1][3][2][1], res[0][3][2][1], "complex plane ch2")


def test_many_streams_and_a_tail_tile_at_1024(pkg):
    """5 streams x 8 AM channels at N = 1024, 3 batches: the first call has 6 100 windows per stream, whole tiles and a tail;
    runs of tiles cross from one stream into the next.  Every stream equals its own oracle run."""
    centre, chans = pkg.config2_channels()
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=10)
    nbat, nstreams = 3, 5
    iqs = [gen_iq(pkg, dev, centre, chans, nbat, stream=s, gate_div=8)[0] for s in range(nstreams)]
    d = pkg.Demod(dev, chans, nstreams=nstreams, max_batches=nbat)
    wo, axc, _, _ = d.process(iqs, nbat)
    assert d.last_stage1() == 3
    d.close()
    any_open = False
    for s in range(nstreams):
        nb, owo, oaxc, _ = oracle_run(dev, chans, iqs[s], nbat)
        assert nb == nbat
        any_open = any_open or (oaxc == ord("*")).any()
        assert_same(axc[s], oaxc, f"stream {s}: flags")
        assert_same(wo[s, :, :nbat * WAVE_BATCH], owo, f"stream {s}: audio")
    assert any_open
    assert any(not np.array_equal(iqs[0], iqs[s]) for s in range(1, nstreams))


def _afc_case(pkg, nbat, log2n):
    centre = 120_000_000
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=log2n)
    binw = dev.sample_rate // (1 << log2n)
    freqs = [centre - 900_000 + 300_000 * k for k in range(6)]
    afcs = [1, 2, 0, 5, 255, 1]
    deltas = [2 * binw, -2 * binw, 2 * binw, 3 * binw, -binw, 0]
    mods = [pkg.MOD_AM, pkg.MOD_AM, pkg.MOD_AM, pkg.MOD_AM, pkg.MOD_NFM, pkg.MOD_AM]
    chans = [pkg.channel_cfg(f, modulation=m, afc=a) for f, m, a in zip(freqs, mods, afcs)]
    carriers = [(f - centre + d, 0 if m == pkg.MOD_AM else 1, 3072, 0) for f, d, m in zip(freqs, deltas, mods)]
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, gate_samples=dev.sample_rate // 4, carriers=carriers)
    return dev, chans, pkg.iqgen_host(cfg, 0, 0, bytes_for_batches(dev, nbat) // 2)


@pytest.mark.parametrize("case", ["afc at 1024", "2.4 MS/s at 1024", "fft 4096"])
def test_fallbacks_stay_fallbacks(pkg, case):
    """Plans the lane kernel does not serve keep the exchange kernel (kind 0) and equal the oracle: AFC, a hop that is not a
    multiple of 8 samples (2.4 MS/s: 150), a size above 2048."""
    nbat = 4
    centre, chans = pkg.config2_channels()
    if case == "afc at 1024":
        dev, chans, iq = _afc_case(pkg, nbat, 10)
    elif case == "2.4 MS/s at 1024":
        centre = 120000000
        chans = [pkg.channel_cfg(centre - 900000 + 25000 + k * 230000) for k in range(8)]
        dev = pkg.device_cfg(sample_rate=2400000, centerfreq=centre, fft_size_log=10)
        iq, _ = gen_iq(pkg, dev, centre, chans, nbat, gate_div=8)
    else:
        dev = pkg.device_cfg(centerfreq=centre, fft_size_log=12)
        iq, _ = gen_iq(pkg, dev, centre, chans, nbat, gate_div=8)
    nb, owo, oaxc, _ = oracle_run(dev, chans, iq, nbat)
    assert nb == nbat and (oaxc == ord("*")).any()
    d = pkg.Demod(dev, chans, max_batches=nbat)
    wo, axc, _, _ = d.process([iq], nbat)
    got = d.last_stage1()
    d.close()
    assert got == 0, f"{case}: the handle ran stage-1 kernel kind {got}"
    assert_same(axc[0], oaxc, f"{case}: flags")
    assert_same(wo[0, :, :nbat * WAVE_BATCH], owo, f"{case}: audio")


KEYS_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(tests)r)
from conftest import load_package
from common import WAVE_BATCH, gen_iq, oracle_run
pkg = load_package()
pkg.set_cache_dir(sys.argv[1])
centre = 120000000
chans = [pkg.channel_cfg(centre + 320000 * j) for j in (-3, -2, -1, 1, 2, 3)]  # bins = -1 mod 64 at every size: the same masks
kinds, equal, masks = [], [], []
for log2n in (9, 10, 11):
    dev = pkg.device_cfg(centerfreq=centre, fft_size_log=log2n)
    p = pkg.Plan(dev, chans)
    masks.append(p.lane_fft()[1])
    p.close()
    iq, _ = gen_iq(pkg, dev, centre, chans, 1, gate_div=8)
    d = pkg.Demod(dev, chans, nstreams=1, max_batches=1, gpu=0)
    wo, axc, _, _ = d.process([iq], 1)
    kinds.append(d.last_stage1())
    d.close()
    nb, owo, oaxc, _ = oracle_run(dev, chans, iq, 1)
    equal.append(bool(nb == 1 and np.array_equal(axc[0], oaxc) and np.array_equal(wo[0, :, :WAVE_BATCH], owo) and np.abs(owo).max() > 0))
print(json.dumps(dict(counts=pkg.jit_counts(), kinds=kinds, equal=equal, same_masks=bool(masks[0] == masks[1] == masks[2]))))
"""


def test_code_objects_are_keyed_by_fft_size(tmp_path):
    """A channel list whose pruning masks are identical at fft 512, 1024 and 2048 (every bin is -1 mod 64; same hop) still gets
    three code objects: N is part of the key.  Three compilations and three files in a fresh cache directory, three loads from
    it on the next start, each handle equal to the oracle (a code object shared across sizes would not be)."""
    cache = tmp_path / "co"
    cache.mkdir()
    code = KEYS_CHILD % {"tests": os.path.join(ROOT, "tests")}

    def child():
        r = subprocess.run([sys.executable, "-c", code, str(cache)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])

    a = child()
    files = sorted(os.listdir(cache))
    assert a["same_masks"], a
    assert a["counts"] == [3, 0], a
    assert a["kinds"] == [3, 3, 3] and a["equal"] == [True, True, True], a
    assert len(files) == 3 and all(f.startswith("l64_") and f.endswith(".co") for f in files), files
    b = child()
    assert b["counts"] == [0, 3], b
    assert b["kinds"] == [3, 3, 3] and b["equal"] == [True, True, True], b
    assert sorted(os.listdir(cache)) == files
