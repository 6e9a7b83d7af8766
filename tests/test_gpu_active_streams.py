"""The per-call active-stream mask (mi_demod_set_active_streams) on the GPU.

A stream that sits a call out is untouched in every respect: its IQ is not read, its output regions keep the sentinel they
were filled with, its rows of the checkpoint blob keep their bytes -- and when it takes part again it continues as if the calls
in between had never been made: per stream, the concatenation of the calls it took part in equals the oracle run over the IQ
that stream consumed, bit for bit, whatever its siblings did meanwhile."""
import ctypes as C
import functools

import numpy as np
import pytest

import libs
from common import AFC_BIN_OFFSET, AGC_EXTRA, WAVE_BATCH, assert_same, blob_rows, bytes_for_batches, to_oracle_cfg

pytestmark = pytest.mark.gpu

SENT32 = 0xDEADBEEF  # what every output buffer holds before a call
SENT8 = 0xEE
SCHEDULE3 = ["111", "101", "001", "110", "010", "111"]
SCHEDULE5 = ["11111", "10101", "00100", "11010", "01011", "11111"]
CENTRE = 120_000_000


def four_kinds(pkg, k=0, spacing=0):
    """plain AM, AM with a low-pass + raw I/Q outputs, NFM + CTCSS, NFM + notch"""
    o = k * spacing
    return [pkg.channel_cfg(CENTRE + 250000 + o),
            pkg.channel_cfg(CENTRE - 500000 + o, bandwidth=8000, has_iq_outputs=1),
            pkg.channel_cfg(CENTRE + 750000 + o, modulation=pkg.MOD_NFM, ctcss=100.0, bandwidth=12500),
            pkg.channel_cfg(CENTRE - 1000000 + o, modulation=pkg.MOD_NFM, notch=1000.0, notch_q=5.0)]


def thirteen(pkg):
    chans = []
    for k in range(4):
        chans += four_kinds(pkg, k, 35000)
    return chans[:13]


def make_dev(pkg, fft_log=9, rate=2560000, sfmt="u8"):
    if sfmt == "s16":
        return pkg.device_cfg(sample_rate=rate, centerfreq=CENTRE, fft_size_log=fft_log, sfmt=pkg.SFMT_S16, fullscale=32767.5)
    return pkg.device_cfg(sample_rate=rate, centerfreq=CENTRE, fft_size_log=fft_log)


def capture(pkg, dev, chans, nbat, stream, sfmt="u8", gate_div=None, carriers=None):
    """`nbat` batches of stream `stream`: every channel's carrier gated on and off inside the run, each stream with a period of its own"""
    n = bytes_for_batches(dev, nbat) // 2
    carriers = carriers or pkg.carriers_for(CENTRE, chans, amp_q8=2048, active=lambda k: True)
    cfg = pkg.iqgen_cfg(sample_rate=dev.sample_rate, seed=0xA1B2C3D4 + stream, gate_samples=dev.sample_rate // (gate_div or (5 + stream)), carriers=carriers)
    iq = pkg.iqgen_host(cfg, stream, 0, n)
    if sfmt == "s16":
        iq = ((iq.astype(np.int32) - 128) * 256 + 37).astype(np.int16).view(np.uint8)
    return iq


def batches_of(schedule, per_call, stream):
    return per_call * sum(1 for m in schedule if m[stream] == "1")


def oracle_of(dev, chans, iq, nbat):
    """(audio, flags, raw I/Q, squelch levels, bins) of the oracle over one stream's IQ"""
    odev, ochans = to_oracle_cfg(dev, chans)
    od = libs.OracleDemod(odev, ochans)
    nb, wo, axc, iqo = od.run(iq, nbat, want_iq=True)
    assert nb == nbat
    out = (wo, axc, iqo, od.squelch_levels(), od.bins()[0])
    od.close()
    return out


CASES = {
    # name: (fft_log, rate, sfmt, nstreams, channels, schedule)
    "fft512": (9, 2560000, "u8", 3, four_kinds, SCHEDULE3),
    "fft1024-hop128": (10, 2048000, "u8", 3, four_kinds, SCHEDULE3),
    "fft256": (8, 2560000, "u8", 3, four_kinds, SCHEDULE3),
    "fft2048": (11, 2560000, "u8", 3, four_kinds, SCHEDULE3),
    "s16": (9, 2560000, "s16", 3, four_kinds, SCHEDULE3),
    "65rows": (9, 2560000, "u8", 5, thirteen, SCHEDULE5),
}
PER_CALL = 2


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Computed once per case and shared (nothing changes it): the plan, every stream's IQ, its oracle run, and the statistics a
    handle of its own leaves after the same calls."""
    from conftest import load_package
    pkg = load_package()
    fft_log, rate, sfmt, ns, mk, schedule = CASES[name]
    dev = make_dev(pkg, fft_log, rate, sfmt)
    chans = mk(pkg)
    iqs, oracle, solo = [], [], []
    for s in range(ns):
        nbat = batches_of(schedule, PER_CALL, s)
        iq = capture(pkg, dev, chans, nbat, s, sfmt)
        iq.setflags(write=False)
        iqs.append(iq)
        oracle.append(oracle_of(dev, chans, iq, nbat))
        d = pkg.Demod(dev, chans, nstreams=1, max_batches=PER_CALL)
        pos = 0
        for c in range(nbat // PER_CALL):
            st = d.process([iq[pos:]], PER_CALL)[3]
            pos = ((c + 1) * PER_CALL * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes
        solo.append(bytes(st))
        d.close()
    return dev, chans, iqs, oracle, solo, schedule


class HostCall:
    """mi_demod_process / mi_demod_submit into buffers that hold a sentinel bit pattern"""

    def __init__(self, pkg, d, k):
        ns, nch, n = d.nstreams, d.nch, k * WAVE_BATCH
        self.wo = np.full((ns, nch, n + AGC_EXTRA), SENT32, np.uint32)
        self.iqo = np.full((ns, nch, n, 2), SENT32, np.uint32)
        self.axc = np.full((ns, nch, k), SENT8, np.uint8)
        self.stats = (pkg.ChannelStats * (ns * nch))()
        C.memset(self.stats, SENT8, C.sizeof(self.stats))
        self.k, self.n, self.nch = k, n, nch

    def args(self, d, ptrs):
        vp = C.c_void_p
        return (d._h, ptrs, self.k, self.wo.ctypes.data_as(vp), self.iqo.ctypes.data_as(vp), self.axc.ctypes.data_as(vp), C.cast(self.stats, vp))

    def stats_bytes(self, s):
        sz = C.sizeof(self.stats) // (len(self.stats) // self.nch)
        return bytes(self.stats)[s * sz:(s + 1) * sz]

    def check_untouched(self, s, what):
        assert (self.wo[s] == SENT32).all(), f"{what}: waveout of inactive stream {s} was written"
        assert (self.iqo[s] == SENT32).all(), f"{what}: iq_out of inactive stream {s} was written"
        assert (self.axc[s] == SENT8).all(), f"{what}: axc of inactive stream {s} was written"
        assert set(self.stats_bytes(s)) == {SENT8}, f"{what}: stats of inactive stream {s} were written"


def stream_ptrs(d, iqs, pos, mask):
    keep = [iqs[s][pos[s]:] if mask[s] == "1" else None for s in range(d.nstreams)]
    for a in keep:
        assert a is None or a.size >= d.bytes_needed(PER_CALL)
    return keep, (C.c_void_p * d.nstreams)(*[None if a is None else a.ctypes.data for a in keep])


def run_schedule(pkg, name, opts, kind=None, check_state=True):
    dev, chans, iqs, oracle, solo, schedule = case_data(name)
    ns = len(iqs)
    d = pkg.Demod(dev, chans, nstreams=ns, max_batches=PER_CALL)
    for k, v in opts.items():
        d.set_option(getattr(pkg, k), v)
    lib = pkg.lib()
    got = [dict(wo=[], axc=[], iqo=[], stats=None) for _ in range(ns)]
    done = [0] * ns
    for ci, mask in enumerate(schedule):
        what = f"{name}, call {ci} (mask {mask})"
        d.set_active_streams([m == "1" for m in mask])
        assert d.get_active_streams() == [m == "1" for m in mask]
        pos = [0 if done[s] == 0 else (done[s] * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes for s in range(ns)]
        keep, ptrs = stream_ptrs(d, iqs, pos, mask)  # iq[s] = NULL for the streams that sit the call out
        before = blob_rows(d.get_state(), ns)[0] if check_state and "0" in mask else None
        call = HostCall(pkg, d, PER_CALL)
        rc = lib.mi_demod_process(*call.args(d, ptrs))
        assert rc == pkg.MI_OK, lib.mi_last_error()
        if "0" in mask:
            assert d.last_path()[0] == 0, f"{what}: a masked call takes the serial stage 2"
        if kind is not None:
            assert d.last_stage1() == kind, f"{what}: stage-1 kernel kind {d.last_stage1()}"
        after = blob_rows(d.get_state(), ns)[0] if before is not None else None
        for s in range(ns):
            if mask[s] == "0":
                call.check_untouched(s, what)
                if before is not None:
                    assert np.array_equal(before[s], after[s]), f"{what}: the state of inactive stream {s} changed"
                continue
            got[s]["wo"].append(call.wo[s, :, :call.n].view(np.float32).copy())
            got[s]["axc"].append(call.axc[s].copy())
            got[s]["iqo"].append(call.iqo[s].view(np.float32).copy())
            got[s]["stats"] = (call.stats_bytes(s), [call.stats[s * d.nch + c].squelch_level for c in range(d.nch)])
            done[s] += PER_CALL
    assert d.pre_wave_timeouts() == 0
    d.close()
    for s in range(ns):
        owo, oaxc, oiq, olevels, _ = oracle[s]
        what = f"{name}, stream {s}"
        assert_same(np.concatenate(got[s]["axc"], axis=1), oaxc, f"{what}: flags")
        assert_same(np.concatenate(got[s]["wo"], axis=1), owo, f"{what}: audio")
        iqo = np.concatenate(got[s]["iqo"], axis=1)
        for c, ch in enumerate(chans):
            if ch.has_iq_outputs:
                assert_same(iqo[c].reshape(-1), oiq[c], f"{what}: raw I/Q of channel {c}")
            else:
                assert (iqo[c].view(np.uint32) == SENT32).all(), f"{what}: iq_out of channel {c} (no iq outputs) was written"
        assert_same(np.array(got[s]["stats"][1], np.float32), olevels, f"{what}: squelch levels of the final statistics")
        assert got[s]["stats"][0] == solo[s], f"{what}: final statistics differ from the same calls on a handle of the stream's own"
        assert (oaxc == ord("*")).any() and (oaxc == ord(" ")).any(), f"{what}: the squelch should open and close inside the run"


STAGE1 = {
    "lane-plan": ({}, 3),
    "lane-full": ({"OPT_LANE_FFT_JIT": 0}, 2),
    "exchange-pruned": ({"OPT_LANE_FFT": 0}, 1),
    "exchange-full": ({"OPT_LANE_FFT": 0, "OPT_PRUNE_FFT": 0}, 0),
}


@pytest.mark.parametrize("variant", list(STAGE1))
def test_parity_and_untouched_rows_on_every_stage1_kernel(pkg, variant):
    """3 streams x 4 channels (plain AM, AM + low-pass + raw I/Q, NFM + CTCSS, NFM + notch), fft 512, u8, 2-batch calls under the masks
    111, 101, 001, 110, 010, 111: one stage-1 launch over the active streams, by each of the four kernels."""
    opts, kind = STAGE1[variant]
    run_schedule(pkg, "fft512", opts, kind)


@pytest.mark.parametrize("name,kind", [("fft1024-hop128", 3), ("fft256", 0), ("s16", 3)])
def test_parity_other_geometries(pkg, name, kind):
    """The lane kernel at N = 1024 / hop 128 (2.048 MS/s), an FFT size only the exchange kernel takes, and 16-bit samples."""
    run_schedule(pkg, name, {}, kind)


@pytest.mark.parametrize("variant", ["lane-plan", "lane-full"])
def test_parity_fft_2048_both_lane_instances(pkg, variant):
    """N = 2048 at hop 160, 32 lanes per window: the stream-list instances of the plan-compiled and of the prebuilt lane kernel."""
    opts, kind = STAGE1[variant]
    run_schedule(pkg, "fft2048", opts, kind, check_state=False)


@pytest.mark.parametrize("pre_wave", [0, 1, 2])
def test_parity_serial_kernel_flavours(pkg, pre_wave):
    """k_demod_uni / k_demod_pw / k_demod_pw2 over the row list of the active streams."""
    run_schedule(pkg, "fft512", {"OPT_PRE_WAVE": pre_wave}, check_state=False)


def test_parity_65_rows_lane_packed(pkg):
    """5 streams x 13 channels with up to 16 waves per launch: the lane-packed serial kernel sees a partial row list (26 .. 39 of the
    65 rows, 2 or 3 lanes per wave, the last wave not full)."""
    run_schedule(pkg, "65rows", {"OPT_UNI_ROWS": 16})


def test_submitted_calls_and_a_mask_change_in_between(pkg):
    """Three mi_demod_submit calls, the mask changed between the second and the third (setting it completes the two in flight):
    every result equals the same calls made one after the other, and the oracle."""
    dev, chans, iqs, oracle, _, _ = case_data("fft512")
    ns = len(iqs)
    masks = ["111", "111", "101"]

    def run(submit):
        d = pkg.Demod(dev, chans, nstreams=ns, max_batches=PER_CALL)
        done, res = [0] * ns, []
        for mask in masks:
            d.set_active_streams([m == "1" for m in mask])
            pos = [0 if done[s] == 0 else (done[s] * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes for s in range(ns)]
            streams = [iqs[s][pos[s]:] if mask[s] == "1" else None for s in range(ns)]
            if submit:
                d.submit(streams, PER_CALL, want_iq=True, waveout=np.full((ns, d.nch, PER_CALL * WAVE_BATCH + AGC_EXTRA), SENT32, np.uint32).view(np.float32))
            else:
                res.append(d.process(streams, PER_CALL, want_iq=True))
            for s in range(ns):
                done[s] += PER_CALL if mask[s] == "1" else 0
        if submit:
            res = [d.wait() for _ in masks]
        d.close()
        return res

    a, b = run(True), run(False)
    n = PER_CALL * WAVE_BATCH
    for ci, mask in enumerate(masks):
        for s in range(ns):
            if mask[s] == "0":
                assert (a[ci][0][s].view(np.uint32) == SENT32).all(), f"call {ci}: waveout of inactive stream {s} was written"
                continue
            assert_same(a[ci][0][s], b[ci][0][s], f"call {ci}, stream {s}: audio + lookahead, submitted vs one after the other")
            assert_same(a[ci][1][s], b[ci][1][s], f"call {ci}, stream {s}: flags")
            assert_same(a[ci][2][s], b[ci][2][s], f"call {ci}, stream {s}: raw I/Q")
            assert bytes(a[ci][3])[s * len(bytes(a[ci][3])) // ns:(s + 1) * len(bytes(a[ci][3])) // ns] == \
                bytes(b[ci][3])[s * len(bytes(b[ci][3])) // ns:(s + 1) * len(bytes(b[ci][3])) // ns], f"call {ci}, stream {s}: statistics"
    for s in range(ns):
        mine = [ci for ci, m in enumerate(masks) if m[s] == "1"]
        wo = np.concatenate([a[ci][0][s][:, :n] for ci in mine], axis=1)
        ax = np.concatenate([a[ci][1][s] for ci in mine], axis=1)
        assert_same(wo, oracle[s][0][:, :wo.shape[1]], f"stream {s}: audio vs the oracle")
        assert_same(ax, oracle[s][1][:, :ax.shape[1]], f"stream {s}: flags vs the oracle")


@pytest.mark.parametrize("plan", ["plain", "mixed"])
def test_masked_call_beside_the_time_parallel_path(pkg, plan):
    """2 streams x 2 plain AM channels (and, `mixed`, an NFM row beside them with MI_OPT_MIXED_PLAN), 8-batch calls on the device
    entry with MI_OPT_TIME_PARALLEL = 1 and MI_OPT_EARLY_INPUT = 1 on a side stream: full, full, masked (stream 0 alone), full, full.
    The full calls take the time-parallel path with every segment verified, the masked one the serial kernel, and the full call
    after it starts from the ChanState rows alone.  Once with two alternating output buffers and the path read after every
    call, once with all five calls enqueued back to back."""
    import torch
    chans = [pkg.channel_cfg(CENTRE + 250000), pkg.channel_cfg(CENTRE - 500000)]
    if plan == "mixed":
        chans.append(pkg.channel_cfg(CENTRE + 750000, modulation=pkg.MOD_NFM))
    dev = make_dev(pkg)
    ns, k, masks = 2, 8, ["11", "11", "10", "11", "11"]
    nbat = [k * sum(1 for m in masks if m[s] == "1") for s in range(ns)]
    iqs = [capture(pkg, dev, chans, nbat[s], s, gate_div=3 + s) for s in range(ns)]
    oracle = [oracle_of(dev, chans, iqs[s], nbat[s]) for s in range(ns)]
    d0 = pkg.Demod(dev, chans, nstreams=ns, max_batches=k)
    hop, need = d0.hop_bytes, d0.bytes_needed(k) + AGC_EXTRA * d0.hop_bytes
    d0.close()
    pad = (need + 255) // 256 * 256
    # the IQ of every call, resident before the first one is made; an inactive stream's slot holds bytes nobody may read
    d_iq, done = [], [0] * ns
    for mask in masks:
        t = torch.full((ns, pad), 0x55, dtype=torch.uint8, device="cuda")
        for s in range(ns):
            if mask[s] == "1":
                pos = 0 if done[s] == 0 else (done[s] * WAVE_BATCH + AGC_EXTRA) * hop
                part = iqs[s][pos:pos + pad]
                t[s, :part.size] = torch.from_numpy(part.copy()).cuda()
                done[s] += k
        d_iq.append(t)
    side = torch.cuda.Stream()
    sent_f = torch.tensor([SENT32 - (1 << 32)], dtype=torch.int32).view(torch.float32).item()

    def fresh():
        wo = torch.full((ns, len(chans), k * WAVE_BATCH), sent_f, dtype=torch.float32, device="cuda")
        ax = torch.full((ns, len(chans), k), SENT8, dtype=torch.uint8, device="cuda")
        return wo, ax

    for paced in (True, False):
        d = pkg.Demod(dev, chans, nstreams=ns, max_batches=k)
        d.set_option(pkg.OPT_TIME_PARALLEL, 1)
        d.set_option(pkg.OPT_EARLY_INPUT, 1)
        d.set_option(pkg.OPT_MIXED_PLAN, 1)
        bufs = [fresh(), fresh()] if paced else [fresh() for _ in masks]
        torch.cuda.synchronize()
        res = []
        for ci, mask in enumerate(masks):
            d.set_active_streams([m == "1" for m in mask])
            wo, ax = bufs[ci % len(bufs)]
            d.process_device(d_iq[ci].data_ptr(), pad, k, wo.data_ptr(), ax.data_ptr(), hip_stream=side.cuda_stream)
            if paced:
                path = d.last_path()  # (synchronises)
                assert path == ((1, 0) if "0" not in mask else (0, path[1])), f"{plan}, call {ci} (mask {mask}): stage-2 path {path}"
                res.append((wo.cpu().numpy().copy(), ax.cpu().numpy().copy()))
                wo.fill_(sent_f), ax.fill_(SENT8)
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        if not paced:
            assert d.last_path() == (1, 0)
            res = [(wo.cpu().numpy(), ax.cpu().numpy()) for wo, ax in bufs]
        d.close()
        for s in range(ns):
            mine = [ci for ci, m in enumerate(masks) if m[s] == "1"]
            for ci in range(len(masks)):
                if ci not in mine:
                    assert (res[ci][0][s].view(np.uint32) == SENT32).all(), f"{plan}: d_waveout of inactive stream {s} was written"
                    assert (res[ci][1][s] == SENT8).all(), f"{plan}: d_axc of inactive stream {s} was written"
            what = f"{plan}, {'paced' if paced else 'back to back'}, stream {s}"
            assert_same(np.concatenate([res[ci][1][s] for ci in mine], axis=1), oracle[s][1], f"{what}: flags")
            assert_same(np.concatenate([res[ci][0][s] for ci in mine], axis=1), oracle[s][0], f"{what}: audio")


def test_afc_streams_sit_out_with_their_bins(pkg):
    """2 streams, an afc channel beside a plain one, one-batch calls under 11, 10, 01, 11: stage 1 of the AFC path reads and k_afc moves
    the bins of the active streams alone.  Audio, the `<` / `>` flags and the bins after every call equal the oracle's."""
    dev = make_dev(pkg)
    binw = dev.sample_rate // 512
    chans = [pkg.channel_cfg(CENTRE - 600000, afc=1), pkg.channel_cfg(CENTRE + 300000)]
    carriers = [(-600000 + 2 * binw, 0, 3072, 0), (300000, 0, 3072, 0)]
    masks, ns = ["11", "10", "01", "11"], 2
    nbat = [sum(1 for m in masks if m[s] == "1") for s in range(ns)]
    # the carrier is on in every other batch: the afc channel finds it two bins up, reports it, and falls back when it goes
    iqs = [capture(pkg, dev, chans, nbat[s], s, gate_div=8, carriers=carriers) for s in range(ns)]
    oracle = [[oracle_of(dev, chans, iqs[s], nb) for nb in range(1, nbat[s] + 1)] for s in range(ns)]
    d = pkg.Demod(dev, chans, nstreams=ns, max_batches=1)
    lib = pkg.lib()
    done, wo, ax = [0] * ns, [[] for _ in range(ns)], [[] for _ in range(ns)]
    for ci, mask in enumerate(masks):
        d.set_active_streams([m == "1" for m in mask])
        pos = [0 if done[s] == 0 else (done[s] * WAVE_BATCH + AGC_EXTRA) * d.hop_bytes for s in range(ns)]
        keep = [iqs[s][pos[s]:] if mask[s] == "1" else None for s in range(ns)]
        ptrs = (C.c_void_p * ns)(*[None if a is None else a.ctypes.data for a in keep])
        call = HostCall(pkg, d, 1)
        assert lib.mi_demod_process(*call.args(d, ptrs)) == pkg.MI_OK, lib.mi_last_error()
        blob = d.get_state()
        state = blob_rows(blob, ns)[1]
        for s in range(ns):
            if mask[s] == "0":
                call.check_untouched(s, f"afc, call {ci}")
                continue
            done[s] += 1
            wo[s].append(call.wo[s, :, :WAVE_BATCH].view(np.float32).copy()), ax[s].append(call.axc[s].copy())
        for s in range(ns):  # the bins of every stream, the ones sitting out included, are where the oracle left them
            bins = [int(blob[32 + (s * 2 + c) * state + AFC_BIN_OFFSET:][:4].view(np.uint32)[0]) for c in range(2)]
            assert bins == list(oracle[s][done[s] - 1][4]), f"afc, call {ci}: bins of stream {s}"
    d.close()
    seen = set()
    for s in range(ns):
        owo, oaxc = oracle[s][-1][0], oracle[s][-1][1]
        assert_same(np.concatenate(ax[s], axis=1), oaxc, f"afc, stream {s}: flags")
        assert_same(np.concatenate(wo[s], axis=1), owo, f"afc, stream {s}: audio")
        seen |= {chr(x) for x in oaxc[0]}
    assert seen & {"<", ">"}, "the afc channel should report a move inside the run"


def test_checkpoint_after_a_masked_call(pkg):
    """get_state after a masked call, set_state into a fresh handle: both handles then produce the same bits, and the oracle's, on
    the next full call."""
    dev, chans, iqs, oracle, _, schedule = case_data("fft512")
    ns = len(iqs)
    a = pkg.Demod(dev, chans, nstreams=ns, max_batches=PER_CALL)
    done = [0] * ns
    for mask in schedule[:5]:  # 111, 101, 001, 110, 010
        a.set_active_streams([m == "1" for m in mask])
        pos = [0 if done[s] == 0 else (done[s] * WAVE_BATCH + AGC_EXTRA) * a.hop_bytes for s in range(ns)]
        a.process([iqs[s][pos[s]:] if mask[s] == "1" else None for s in range(ns)], PER_CALL)
        for s in range(ns):
            done[s] += PER_CALL if mask[s] == "1" else 0
    blob = a.get_state()
    b = pkg.Demod(dev, chans, nstreams=ns, max_batches=PER_CALL)
    b.set_state(blob)
    a.set_active_streams(None)
    pos = [(done[s] * WAVE_BATCH + AGC_EXTRA) * a.hop_bytes for s in range(ns)]
    ra = a.process([iqs[s][pos[s]:] for s in range(ns)], PER_CALL, want_iq=True)
    rb = b.process([iqs[s][pos[s]:] for s in range(ns)], PER_CALL, want_iq=True)
    a.close(), b.close()
    assert_same(ra[0], rb[0], "audio + lookahead after the checkpoint")
    assert_same(ra[1], rb[1], "flags after the checkpoint")
    assert_same(ra[2], rb[2], "raw I/Q after the checkpoint")
    assert bytes(ra[3]) == bytes(rb[3]), "statistics after the checkpoint"
    n = PER_CALL * WAVE_BATCH
    for s in range(ns):
        assert_same(ra[0][s][:, :n], oracle[s][0][:, done[s] * WAVE_BATCH:done[s] * WAVE_BATCH + n], f"stream {s}: audio vs the oracle")
        assert_same(ra[1][s], oracle[s][1][:, done[s]:done[s] + PER_CALL], f"stream {s}: flags vs the oracle")


def test_mask_errors(pkg):
    dev, chans, iqs, _, _, _ = case_data("fft512")
    ns = len(iqs)
    d = pkg.Demod(dev, chans, nstreams=ns, max_batches=PER_CALL)
    assert d.get_active_streams() == [True] * ns
    with pytest.raises(pkg.MiError) as e:
        d.set_active_streams([False] * ns)
    assert e.value.code == pkg.MI_ERR_INVALID
    assert d.get_active_streams() == [True] * ns
    d.set_active_streams([True, False, True])
    assert d.get_active_streams() == [True, False, True]
    with pytest.raises(pkg.MiError) as e:  # the handle's first call needs every stream
        d.process([iqs[0], None, iqs[2]], PER_CALL)
    assert e.value.code == pkg.MI_ERR_INVALID
    mag = np.zeros((ns * len(chans), PER_CALL * WAVE_BATCH + AGC_EXTRA), np.float32)
    cplx = np.zeros((ns * 3, PER_CALL * WAVE_BATCH + AGC_EXTRA, 2), np.float32)
    with pytest.raises(pkg.MiError) as e:
        d.process_planes(mag, PER_CALL, cplx=cplx)
    assert e.value.code == pkg.MI_ERR_UNSUPPORTED
    d.set_active_streams(None)  # NULL restores all
    assert d.get_active_streams() == [True] * ns
    wo, axc, _, _ = d.process([iq for iq in iqs], PER_CALL)  # ... and the handle is as good as new
    d.close()
    _, _, _, oracle, _, _ = case_data("fft512")
    for s in range(ns):
        assert_same(wo[s][:, :PER_CALL * WAVE_BATCH], oracle[s][0][:, :PER_CALL * WAVE_BATCH], f"stream {s}: audio of the first call")
