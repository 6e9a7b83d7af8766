"""The host mirror's turn rule: an engine gets a turn when at least one running member has a batch; members whose ring is
short sit the turn out through the engine's active-stream mask.  Four devices of one plan on one engine with captures of
5, 3, 4 and 2 batches: every device delivers all of its own batches, each bit for bit its own oracle run, no ring overflows
and no batch is overrun.  (With a turn only when every member has a batch, the siblings of the shortest capture stop with it.)"""
import os
import subprocess

import numpy as np
import pytest

from common import assert_same, gen_iq, oracle_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "boondock-airband_amd", "host")
TOOL = os.path.join(HOST, "airband_replay")


@pytest.mark.gpu
def test_devices_of_one_engine_with_captures_of_unequal_length(pkg, tmp_path):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    centre = 120000000
    chans = [pkg.channel_cfg(centre + 250000), pkg.channel_cfg(centre - 500000, bandwidth=8000, has_iq_outputs=1),
             pkg.channel_cfg(centre + 750000, modulation=pkg.MOD_NFM, ctcss=100.0, bandwidth=12500)]
    dev = pkg.device_cfg(centerfreq=centre)
    lengths = [5, 3, 4, 2]
    caps, iqs = [], []
    for d, nbat in enumerate(lengths):
        iq, _ = gen_iq(pkg, dev, centre, chans, nbat, stream=d, gate_div=5 + d, active=lambda k: True)
        path = tmp_path / f"cap{d}.iq"
        iq.tofile(path)
        caps.append(str(path))
        iqs.append(iq)
    cfg = tmp_path / "cfg.txt"
    with open(cfg, "w") as f:
        f.write(f"{dev.sample_rate} {dev.centerfreq} {dev.fft_size_log} {dev.sfmt} {dev.tau} {dev.fm_quadri}\n")
        for c in chans:
            f.write(f"{c.freq} {c.modulation} {c.squelch_threshold_dbfs} {c.has_snr_threshold} {c.squelch_snr_db} {c.notch_freq} "
                    f"{c.notch_q} {c.ctcss_freq} {c.bandwidth} {c.ampfactor} {c.tau} {c.afc} {c.has_iq_outputs}\n")
    r = subprocess.run([TOOL, str(cfg), ",".join(caps), str(tmp_path / "out")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert f"devices=4 engines=1 batches={','.join(str(n) for n in lengths)} overruns=0 overflows=0" in r.stdout, r.stdout + r.stderr
    for d, nbat in enumerate(lengths):
        nb, owo, oaxc, _ = oracle_run(dev, chans, iqs[d], nbat)
        assert nb == nbat
        flags = open(tmp_path / f"out_d{d}_axc.txt").read().splitlines()
        for c in range(len(chans)):
            got = np.fromfile(tmp_path / f"out_d{d}_ch{c}.f32", dtype=np.float32)
            assert_same(got, owo[c], f"device {d} ch{c} audio")
            assert flags[c] == bytes(oaxc[c]).decode(), f"device {d} ch{c} axcindicate"
