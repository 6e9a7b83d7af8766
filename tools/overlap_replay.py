"""Overlapping time-parallel calls against the oracle, call by call (the loop of bench.py: 1 stream x 8 AM channels, 16 batches per
call, MI_OPT_EARLY_INPUT, the steps on alternating audio buffers, the same capture replayed every step).

    python tools/overlap_replay.py [runs per variant] [NAME=VALUE ...]

The oracle side is stage 1 once and then ao_demod_run_planes over the same planes call after call.  Every run is a fresh process;
a variant is a set of MI_AIRBAND_* switches (default: none, and MI_AIRBAND_RESERVE_CUS=0, under which the defect of DESIGN.md
"Known defect: the split core chain under overlapping calls" shows in most processes).  Prints per variant how many processes
differed from the oracle, with (step, channel) and the rows' tp_debug counters; exits 1 if any did."""
import os, subprocess, sys, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # tools/ sits beside tests/
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
from conftest import load_package
import libs
from common import to_oracle_cfg
WB, EX, HOP = 2000, 100, 320
NBAT, NCALLS = 16, 5
pkg = load_package()
centre, chans = pkg.config2_channels()
dev = pkg.device_cfg(centerfreq=centre, fft_size_log=9)
nsteps = NBAT * WB
nbytes = ((nsteps + EX) * HOP + 2 * 512 + 255) // 256 * 256
gcfg = pkg.iqgen_cfg(sample_rate=2560000, gate_samples=2560000, carriers=pkg.carriers_for(centre, chans))
iq = pkg.iqgen_host(gcfg, 0, 0, nbytes // 2)

def child():
    import torch
    stream = torch.cuda.Stream(); torch.cuda.set_stream(stream)
    d_iq = torch.from_numpy(iq).cuda()
    wos = [torch.empty((1, 8, nsteps), dtype=torch.float32, device="cuda") for _ in range(5)]
    axs = [torch.empty((1, 8, NBAT), dtype=torch.uint8, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    h = pkg.Demod(dev, chans, nstreams=1, max_batches=NBAT, gpu=0)
    h.set_option(pkg.OPT_EARLY_INPUT, 1)
    h.process_device(d_iq.data_ptr(), nbytes, NBAT, wos[0].data_ptr(), axs[0].data_ptr(), hip_stream=stream.cuda_stream)
    for k in range(NCALLS - 1):
        h.process_device(d_iq.data_ptr() + EX * HOP, nbytes, NBAT, wos[k % 5].data_ptr(), axs[k % 5].data_ptr(), hip_stream=stream.cuda_stream)
    torch.cuda.synchronize()
    # buffers: prime -> 0, then steps 0..3 -> buffers 0,1,2,3 (as bench.py: nstep % nbuf): the prime's output is overwritten by step 0
    res = []
    for k in range(NCALLS - 1):
        a = wos[k].cpu().numpy()[0]; f = axs[k].cpu().numpy()[0]
        res.append(" ".join(f"{zlib.crc32(a[c].tobytes()) & 0xffffffff:08x}:{zlib.crc32(f[c].tobytes()) & 0xffffffff:08x}" for c in range(8)))
    diag = [h.tp_debug(c)[1].tolist() for c in range(8)]
    for k, r in enumerate(res):
        print("STEP", k, r)
    print("DIAG", diag)
    h.close()

if "child" in sys.argv[1:]:
    child()
    sys.exit(0)

odev, ochans = to_oracle_cfg(dev, chans)
od = libs.OracleDemod(odev, ochans)
mag, _ = od.stage1(iq, nsteps + EX, want_iq=False)
od.close()
od = libs.OracleDemod(odev, ochans)
want = []
for k in range(NCALLS):
    nb, wo, axc, _ = od.run_planes(mag if k == 0 else mag[:, EX:], NBAT)
    if k:
        want.append(" ".join(f"{zlib.crc32(wo[c].tobytes()) & 0xffffffff:08x}:{zlib.crc32(axc[c].tobytes()) & 0xffffffff:08x}" for c in range(8)))
args = [a for a in sys.argv[1:] if a != "child"]
runs = int(args[0]) if args and args[0].isdigit() else 8
extra = dict(a.split("=", 1) for a in args if "=" in a)
variants = [("switches " + str(extra), extra)] if extra else [("default", {}), ("MI_AIRBAND_RESERVE_CUS=0", {"MI_AIRBAND_RESERVE_CUS": "0"})]
total_bad = 0
for name, env in variants:
    bad = 0
    for i in range(runs):
        r = subprocess.run([sys.executable, __file__, "child"], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))
        if r.returncode != 0:
            print(name, "child failed", r.returncode, r.stderr[-1500:]); sys.exit(1)
        lines = [l for l in r.stdout.splitlines() if l.startswith("STEP")]
        wrong = []
        for k, l in enumerate(lines):
            got = l.split()[2:]
            w = want[k].split()
            wrong += [(k, c, "audio" if got[c][:8] != w[c][:8] else "", "flags" if got[c][9:] != w[c][9:] else "") for c in range(8) if got[c] != w[c]]
        if wrong:
            bad += 1
            print(name, "run", i, "WRONG (step, ch):", wrong, [l for l in r.stdout.splitlines() if l.startswith("DIAG")])
    print(name, ":", bad, f"of {runs} processes differ from the oracle", flush=True)
    total_bad += bad
sys.exit(1 if total_bad else 0)
