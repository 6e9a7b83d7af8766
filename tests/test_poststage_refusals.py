"""What the post-stages refuse, and in which words, without a GPU: the output gate, the transmission splitter, the tone finder, the PCM,
voice band and limiter stages, the mixer and the two host twins.  Every code and text below was copied from the sources as they stood before the stages came to share one error helper and one set
of argument checks; a call that is refused must be refused with the same code and the same bytes of mi_last_error() after it."""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE = -1, -2
NULL = b"NULL argument"
GATE_GEOMETRY = b"output gate needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
GATE_RULE = b"gate rule out of range 0..3"
GATE_STATE = b"output gate state: NULL argument or wrong length"
TX_GEOMETRY = b"transmission splitter needs 1 <= rows < 2^20, max_batches >= 1 and rows * (max_batches + 1) < 2^24"
TX_STATE = b"transmission splitter state: NULL argument or wrong length"
STRIDE = b"a row stride is shorter than the call"
WAVE_BATCH = 2000


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def refused(pkg, rc, code, text):
    assert rc == code
    assert pkg.lib().mi_last_error() == text


@pytest.fixture()
def L(pkg):
    return pkg.lib()


def test_output_gate(pkg, L):
    out = C.c_void_p()
    rule, some = np.ones(4, np.uint8), np.zeros(64, np.uint8)
    create = L.mi_outgate_create
    refused(pkg, create(None, None, 4, 1, 0, 0, C.byref(out)), INVALID, NULL)
    refused(pkg, create(ptr(rule), None, 4, 1, 0, 0, None), INVALID, NULL)
    for rows, max_batches in ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, 1 << 12), ((1 << 20) - 1, 17)):
        refused(pkg, create(ptr(rule), None, rows, max_batches, 0, 0, C.byref(out)), INVALID, GATE_GEOMETRY)
    for bad in (4, 255):
        refused(pkg, create(ptr(np.array([0, 3, bad, 1], np.uint8)), None, 4, 1, 0, 0, C.byref(out)), INVALID, GATE_RULE)
    assert not out.value
    if pkg.device_count() < 1:
        refused(pkg, create(ptr(rule), None, 4, 1, 0, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the output gate runs on the GPU only")
        refused(pkg, create(ptr(rule), ptr(rule), 4, 2, 3, -1, C.byref(out)), NO_DEVICE, b"no HIP device: the output gate runs on the GPU only")
        assert not out.value
    # every other entry point refuses a NULL handle, and a NULL argument, before it looks at anything else
    refused(pkg, L.mi_outgate_set_rules(None, ptr(rule)), INVALID, NULL)
    refused(pkg, L.mi_outgate_process_device(None, ptr(some), 0, None, 0, ptr(some), 0, 1, ptr(some), None, ptr(some), ptr(some), ptr(some), None),
            INVALID, NULL)
    refused(pkg, L.mi_outgate_download(None, None, None, None, None, None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_outgate_set_timing(None, 1), INVALID, NULL)
    refused(pkg, L.mi_outgate_last_launch_ms(None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_outgate_get_state(None, ptr(some), 4), INVALID, GATE_STATE)
    refused(pkg, L.mi_outgate_set_state(None, ptr(some), 4), INVALID, GATE_STATE)
    assert L.mi_outgate_state_size(None) == 0
    L.mi_outgate_destroy(None)


def test_transmission_splitter(pkg, L):
    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(64, np.uint8)
    cfg = pkg.TxCfg(0, 0, 0)
    create = L.mi_txsplit_create
    refused(pkg, create(C.byref(cfg), None, 4, 1, 0, 0, C.byref(out)), INVALID, NULL)
    refused(pkg, create(C.byref(cfg), ptr(en), 4, 1, 0, 0, None), INVALID, NULL)
    for rows, max_batches in ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, (1 << 12) - 1), ((1 << 20) - 1, 16)):
        refused(pkg, create(None, ptr(en), rows, max_batches, 0, 0, C.byref(out)), INVALID, TX_GEOMETRY)
    assert not out.value
    if pkg.device_count() < 1:
        refused(pkg, create(None, ptr(en), 4, 1, 0, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the transmission splitter runs on the GPU only")
        refused(pkg, create(C.byref(cfg), ptr(en), 4, 2, 3, -1, C.byref(out)), NO_DEVICE,
                b"no HIP device: the transmission splitter runs on the GPU only")
        assert not out.value
    refused(pkg, L.mi_txsplit_set_rows(None, ptr(en)), INVALID, NULL)
    refused(pkg, L.mi_txsplit_process_device(None, ptr(some), 0, ptr(some), 0, 1, ptr(some), ptr(some), ptr(some), None), INVALID, NULL)
    refused(pkg, L.mi_txsplit_download(None, None, None, None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_txsplit_set_timing(None, 1), INVALID, NULL)
    refused(pkg, L.mi_txsplit_last_launch_ms(None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_txsplit_get_state(None, ptr(some), 32), INVALID, TX_STATE)
    refused(pkg, L.mi_txsplit_set_state(None, ptr(some), 32), INVALID, TX_STATE)
    assert L.mi_txsplit_state_size(None) == 0
    L.mi_txsplit_destroy(None)


GEOMETRY_PAIRS = ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, 1 << 12), ((1 << 20) - 1, 17))  # (the gate's)
TONES_GEOMETRY = b"tone finder needs 1 <= rows < 2^20, 1 <= max_batches <= 2^20 and rows * ((window - 1 + 2000 * max_batches) / window) < 2^24"
TONES_WINDOW = b"tone finder: window_samples outside 800 .. 64000 (0 = the default 6400)"
TONES_STATE = b"tone finder state: NULL argument or wrong length"
PCM_GEOMETRY = b"PCM stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
PCM_RATE = b"PCM stage: rate must be 8000 or 16000 (0 = 8000)"
PCM_FORMAT = b"PCM stage: format must be MI_PCM_S16 or MI_PCM_IMA4 (0 = MI_PCM_S16)"
PCM_STATE = b"PCM stage state: NULL argument or wrong length"
VBAND_GEOMETRY = b"voice band stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
VBAND_STATE = b"voice band stage state: NULL argument or wrong length"
LIMIT_GEOMETRY = b"limiter stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
LIMIT_STATE = b"limiter stage state: NULL argument or wrong length"


def test_tone_finder(pkg, L):
    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(64, np.uint8)
    cfg = pkg.TonesCfg(0)
    create = L.mi_tones_create
    refused(pkg, create(C.byref(cfg), None, 4, 1, 0, 0, C.byref(out)), INVALID, NULL)
    refused(pkg, create(C.byref(cfg), ptr(en), 4, 1, 0, 0, None), INVALID, NULL)
    # the gate's pairs as far as the finder's own rule refuses them (its product counts windows, 2000 * max_batches / 6400 of them, so
    # the gate's last two pass it), then that rule's own edges: max_batches over 2^20 and the product on both of its sides
    for rows, max_batches in GEOMETRY_PAIRS[:5] + ((4, (1 << 20) + 1), (1 << 12, 1 << 14), ((1 << 20) - 1, 52)):
        refused(pkg, create(None, ptr(en), rows, max_batches, 0, 0, C.byref(out)), INVALID, TONES_GEOMETRY)
    for window in (1, 799, 64001, 0xFFFFFFFF):
        refused(pkg, create(C.byref(pkg.TonesCfg(window)), ptr(en), 4, 1, 0, 0, C.byref(out)), INVALID, TONES_WINDOW)
    refused(pkg, create(C.byref(pkg.TonesCfg(799)), None, 0, 1, 0, 0, C.byref(out)), INVALID, NULL)  # the order: NULL, the window, the geometry
    refused(pkg, create(C.byref(pkg.TonesCfg(799)), ptr(en), 0, 1, 0, 0, C.byref(out)), INVALID, TONES_WINDOW)
    assert not out.value
    if pkg.device_count() < 1:
        refused(pkg, create(None, ptr(en), 4, 1, 0, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the tone finder runs on the GPU only")
        refused(pkg, create(C.byref(pkg.TonesCfg(800)), ptr(en), 4, 2, 3, -1, C.byref(out)), NO_DEVICE,
                b"no HIP device: the tone finder runs on the GPU only")
        assert not out.value
    refused(pkg, L.mi_tones_set_rows(None, ptr(en)), INVALID, NULL)
    refused(pkg, L.mi_tones_process_device(None, ptr(some), 0, ptr(some), 0, 1, ptr(some), None, ptr(some), ptr(some), None), INVALID, NULL)
    refused(pkg, L.mi_tones_download(None, None, None, None, None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_tones_set_timing(None, 1), INVALID, NULL)
    refused(pkg, L.mi_tones_last_launch_ms(None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_tones_get_state(None, ptr(some), 520), INVALID, TONES_STATE)
    refused(pkg, L.mi_tones_set_state(None, ptr(some), 520), INVALID, TONES_STATE)
    assert L.mi_tones_state_size(None) == 0
    L.mi_tones_destroy(None)


def test_pcm_stage(pkg, L):
    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(64, np.uint8)
    cfg = pkg.PcmCfg(0, 0)
    create = L.mi_pcm_create
    refused(pkg, create(C.byref(cfg), None, 4, 1, 0, 0, C.byref(out)), INVALID, NULL)
    refused(pkg, create(C.byref(cfg), ptr(en), 4, 1, 0, 0, None), INVALID, NULL)
    for rows, max_batches in GEOMETRY_PAIRS:
        refused(pkg, create(None, ptr(en), rows, max_batches, 0, 0, C.byref(out)), INVALID, PCM_GEOMETRY)
    for rate in (1, 7999, 44100, 0xFFFFFFFF):
        refused(pkg, create(C.byref(pkg.PcmCfg(rate, 0)), ptr(en), 4, 1, 0, 0, C.byref(out)), INVALID, PCM_RATE)
    for fmt in (3, 0xFFFFFFFF):
        refused(pkg, create(C.byref(pkg.PcmCfg(16000, fmt)), ptr(en), 4, 1, 0, 0, C.byref(out)), INVALID, PCM_FORMAT)
    refused(pkg, create(C.byref(pkg.PcmCfg(1, 3)), None, 0, 1, 0, 0, C.byref(out)), INVALID, NULL)  # the order: NULL, rate, format, the geometry
    refused(pkg, create(C.byref(pkg.PcmCfg(1, 3)), ptr(en), 0, 1, 0, 0, C.byref(out)), INVALID, PCM_RATE)
    refused(pkg, create(C.byref(pkg.PcmCfg(8000, 3)), ptr(en), 0, 1, 0, 0, C.byref(out)), INVALID, PCM_FORMAT)
    assert not out.value
    if pkg.device_count() < 1:
        refused(pkg, create(None, ptr(en), 4, 1, 0, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the PCM stage runs on the GPU only")
        refused(pkg, create(C.byref(pkg.PcmCfg(16000, pkg.PCM_IMA4)), ptr(en), 4, 2, 3, -1, C.byref(out)), NO_DEVICE,
                b"no HIP device: the PCM stage runs on the GPU only")
        assert not out.value
    refused(pkg, L.mi_pcm_set_rows(None, ptr(en)), INVALID, NULL)
    refused(pkg, L.mi_pcm_process_device(None, ptr(some), 0, 1, ptr(some), ptr(some), ptr(some), None), INVALID, NULL)
    refused(pkg, L.mi_pcm_download(None, None, None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_pcm_set_timing(None, 1), INVALID, NULL)
    refused(pkg, L.mi_pcm_last_launch_ms(None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_pcm_get_state(None, ptr(some), 248), INVALID, PCM_STATE)
    refused(pkg, L.mi_pcm_set_state(None, ptr(some), 248), INVALID, PCM_STATE)
    assert L.mi_pcm_state_size(None) == 0
    L.mi_pcm_destroy(None)


def plane_stage(pkg, L, prefix, row_dtype, good, bad_rows, geometry, state_text, state_row_bytes, no_device):
    """mi_vband_* and mi_limit_* have one shape: (row_cfg, row_enabled, rows, max_batches, gpu, out), settings looked at behind the geometry"""
    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(64, np.uint8)
    cfg = np.array([good] * 4, row_dtype)
    create = getattr(L, prefix + "_create")
    refused(pkg, create(ptr(cfg), None, 4, 1, 0, C.byref(out)), INVALID, NULL)
    refused(pkg, create(ptr(cfg), ptr(en), 4, 1, 0, None), INVALID, NULL)
    for rows, max_batches in GEOMETRY_PAIRS:
        refused(pkg, create(None, ptr(en), rows, max_batches, 0, C.byref(out)), INVALID, geometry)
    for bad, text in bad_rows:
        worse = np.array([good, good, bad, good], row_dtype)  # (one row is enough, wherever it stands)
        refused(pkg, create(ptr(worse), ptr(en), 4, 1, 0, C.byref(out)), INVALID, text)
        refused(pkg, create(ptr(worse), None, 0, 1, 0, C.byref(out)), INVALID, NULL)  # the order: NULL, the geometry, the settings
        refused(pkg, create(ptr(worse), ptr(en), 4, 0, 0, C.byref(out)), INVALID, geometry)
    assert not out.value
    if pkg.device_count() < 1:
        refused(pkg, create(None, ptr(en), 4, 1, 0, C.byref(out)), NO_DEVICE, no_device)
        refused(pkg, create(ptr(cfg), ptr(en), 4, 2, -1, C.byref(out)), NO_DEVICE, no_device)
        assert not out.value
    refused(pkg, getattr(L, prefix + "_set_rows")(None, ptr(cfg), ptr(en)), INVALID, NULL)
    refused(pkg, getattr(L, prefix + "_process_device")(None, ptr(some), 0, 1, ptr(some), 0, None), INVALID, NULL)
    refused(pkg, getattr(L, prefix + "_set_timing")(None, 1), INVALID, NULL)
    refused(pkg, getattr(L, prefix + "_last_launch_ms")(None, ptr(some)), INVALID, NULL)
    refused(pkg, getattr(L, prefix + "_get_state")(None, ptr(some), state_row_bytes), INVALID, state_text)
    refused(pkg, getattr(L, prefix + "_set_state")(None, ptr(some), state_row_bytes), INVALID, state_text)
    assert getattr(L, prefix + "_state_size")(None) == 0
    getattr(L, prefix + "_destroy")(None)


def test_voice_band_stage(pkg, L):
    hp, lp, gap = (b"voice band stage: hp_hz must be 0 or 50 .. 4000", b"voice band stage: lp_hz must be 0 or 500 .. 7800",
                   b"voice band stage: lp_hz must be 0 or at least hp_hz + 200")
    bad_rows = [((49, 2500), hp), ((4001, 0), hp), ((100, 499), lp), ((100, 7801), lp), ((400, 599), gap), ((4001, 499), hp)]
    plane_stage(pkg, L, "mi_vband", pkg.VBAND_ROW_DTYPE, (100, 2500), bad_rows, VBAND_GEOMETRY, VBAND_STATE, 2040,
                b"no HIP device: the voice band stage runs on the GPU only")


def test_limiter_stage(pkg, L):
    pregain, ceiling = b"limiter stage: pregain must be finite and within 2^-10 .. 2^10", b"limiter stage: ceiling must be finite and within 0.0625 .. 1"
    bad_rows = [((0.0009765624, 0.5), pregain), ((1024.0001, 0.5), pregain), ((float("nan"), 0.5), pregain), ((float("inf"), 0.5), pregain),
                ((1.0, 0.0624), ceiling), ((1.0, 1.0000001), ceiling), ((1.0, float("nan")), ceiling), ((0.0, 2.0), pregain)]
    plane_stage(pkg, L, "mi_limit", pkg.LIMIT_ROW_DTYPE, (1.0, 0.5), bad_rows, LIMIT_GEOMETRY, LIMIT_STATE, 4344,
                b"no HIP device: the limiter stage runs on the GPU only")


def test_mixer(pkg, L):
    out = C.c_void_p()
    one = (pkg.MixInput * 1)(pkg.MixInput(0, 1.0, 0.0))
    some = np.zeros(64, np.uint8)
    refused(pkg, L.mi_mixer_create(None, 1, 0, C.byref(out)), INVALID, b"mixer needs at least one input")
    refused(pkg, L.mi_mixer_create(one, 1, 0, None), INVALID, b"mixer needs at least one input")
    refused(pkg, L.mi_mixer_create(one, 0, 0, C.byref(out)), INVALID, b"mixer needs at least one input")
    assert not out.value
    if pkg.device_count() < 1:
        refused(pkg, L.mi_mixer_create(one, 1, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the mixer runs on the GPU only")
        bad = (pkg.MixInput * 1)(pkg.MixInput(-1, 1.0, 2.0))  # (its inputs are looked at after the device)
        refused(pkg, L.mi_mixer_create(bad, 1, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the mixer runs on the GPU only")
        assert not out.value
    refused(pkg, L.mi_mixer_process_device(None, ptr(some), 0, ptr(some), 0, 1, ptr(some), None, ptr(some), None), INVALID, NULL)
    assert L.mi_mixer_is_stereo(None) == 0
    L.mi_mixer_destroy(None)


STAGES = {"probe": ("channel probe", "mi_probe_create", "mi_probe_destroy", b"no HIP device: the channel probe runs on the GPU only"),
          "survey": ("band survey", "mi_survey_create", "mi_survey_destroy", b"no HIP device: the band survey runs on the GPU only")}


def stage_create(pkg, L, stage, dev, out):
    if stage == "probe":
        return L.mi_probe_create(C.byref(dev), 1, 1, 1, 1, 0, C.byref(out))
    return L.mi_survey_create(C.byref(dev), 1, 1, 1, 0, C.byref(out))


def lds_refusal(stage, log2n, sfmt, hop):
    """the words of the refusal, with the need that tests/survey_model.py restates from the stage's one LDS function"""
    import survey_model as sv
    return (f"{STAGES[stage][0]}: a workgroup would need {sv.lds_bytes(stage, log2n, sfmt, hop)} bytes of LDS at this fft_size, sample format and hop "
            f"({hop * sv.COMPLEX_BYTES[sfmt]} bytes), over the limit of {sv.LDS_LIMIT} (160 KiB): lower the sample rate").encode()


@pytest.mark.parametrize("stage", ["probe", "survey"])
def test_lds_limit_refused_at_create(pkg, L, stage):
    """A workgroup of k_probe / k_survey keeps TW windows of span in LDS, so the need grows with the hop, and a geometry that needs more
    than 160 KiB can never launch: create refuses it, before it looks for a device, with the need and the limit in the message.
    The largest accepted hop comes from the stage's formula as tests/survey_model.py restates it: at fft 256 with s16 it is 568 samples
    (9 088 000 S/s, 163 632 bytes) and 569 (9 104 000 S/s, 163 888 bytes) is refused, for both stages (the survey's fold region, 24 KB at
    most, is the smaller one anywhere near the limit); with f32 it is 282 samples (4 512 000 S/s).  The rate just under the limit passes the check: without a
    device the refusal is then the missing device's, with one the handle is made.  The messages state the hop as sample_rate / 16000."""
    import survey_model as sv
    _, _, destroy, no_device = STAGES[stage]
    out = C.c_void_p()
    hop = sv.largest_hop(stage, 8, sv.SFMT_S16)
    assert hop == 568 and sv.lds_bytes(stage, 8, sv.SFMT_S16, hop) == 163632 and sv.lds_bytes(stage, 8, sv.SFMT_S16, hop + 1) == 163888
    # every FFT size (each has its own piece length TW, exchange slots and, in the survey, fold region) and every format
    cases = [(8, sv.SFMT_S16, 32767.0), (8, sv.SFMT_F32, 2.0), (9, sv.SFMT_U8, 127.5), (10, sv.SFMT_S16, 32767.0), (11, sv.SFMT_S8, 127.5),
             (12, sv.SFMT_U8, 127.5), (13, sv.SFMT_U8, 127.5), (13, sv.SFMT_F32, 2.0)]
    for log2n, sfmt, fullscale in cases:
        hop = sv.largest_hop(stage, log2n, sfmt)
        over = pkg.device_cfg(sample_rate=(hop + 1) * sv.WAVE_RATE, fft_size_log=log2n, sfmt=sfmt, fullscale=fullscale)
        assert sv.hop_samples(over.sample_rate) == hop + 1
        refused(pkg, stage_create(pkg, L, stage, over, out), INVALID, lds_refusal(stage, log2n, sfmt, hop + 1))
        assert not out.value
        # the last rate that still rounds to the largest accepted hop
        under = pkg.device_cfg(sample_rate=hop * sv.WAVE_RATE + sv.WAVE_RATE // 2 - 1, fft_size_log=log2n, sfmt=sfmt, fullscale=fullscale)
        assert sv.hop_samples(under.sample_rate) == hop
        rc = stage_create(pkg, L, stage, under, out)
        if pkg.device_count() < 1:
            refused(pkg, rc, NO_DEVICE, no_device)
            assert not out.value
        else:
            assert rc == 0 and out.value
            getattr(L, destroy)(out)
            out = C.c_void_p()
    assert sv.largest_hop(stage, 8, sv.SFMT_F32) == 282
    # far over the limit, and the hop check that stands before it: f32 at 2.1 GS/s is a hop of 131 250 samples = 1 050 000 bytes > 2^20
    far = pkg.device_cfg(sample_rate=10000000, fft_size_log=8, sfmt=sv.SFMT_S16, fullscale=32767.0)
    refused(pkg, stage_create(pkg, L, stage, far, out), INVALID, lds_refusal(stage, 8, sv.SFMT_S16, 625))
    wide = pkg.device_cfg(sample_rate=2100000000, fft_size_log=8, sfmt=sv.SFMT_F32, fullscale=2.0)
    refused(pkg, stage_create(pkg, L, stage, wide, out), INVALID, f"{STAGES[stage][0]}: the hop (sample_rate / 16000 samples) is out of range".encode())
    assert not out.value


def test_gate_plan_host(pkg, L):
    rows, nb = 3, 5
    rule, axc, carried = np.ones(rows, np.uint8), np.full((rows, nb), ord("*"), np.uint8), np.zeros(rows, np.uint8)
    index, first, count = np.zeros((rows * nb, 2), np.uint32), np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)
    good = [ptr(rule), rows, ptr(axc), nb, nb, ptr(carried), ptr(index), ptr(first), ptr(count)]
    assert L.mi_gate_plan_host(*good) == 0 and count[0] == rows * nb
    for i in (0, 2, 5, 6, 7, 8):
        refused(pkg, L.mi_gate_plan_host(*[None if j == i else a for j, a in enumerate(good)]), INVALID, NULL)
    geometry = b"gate plan needs rows >= 1 and 1 <= nbatches <= axc_stride"
    for r, stride, n in ((0, nb, nb), (-1, nb, nb), (rows, nb, 0), (rows, nb, -1), (rows, nb - 1, nb)):  # (the last: row stride too short)
        refused(pkg, L.mi_gate_plan_host(ptr(rule), r, ptr(axc), stride, n, ptr(carried), ptr(index), ptr(first), ptr(count)), INVALID, geometry)
    refused(pkg, L.mi_gate_plan_host(ptr(rule), 1 << 20, ptr(axc), 1 << 12, 1 << 12, ptr(carried), ptr(index), ptr(first), ptr(count)), INVALID,
            b"gate plan: rows * nbatches does not fit the 32-bit block index")
    for bad in (4, 255):
        worse = np.array([1, 1, bad], np.uint8)
        refused(pkg, L.mi_gate_plan_host(*([ptr(worse)] + good[1:])), INVALID, GATE_RULE)


def test_tx_plan_host(pkg, L):
    rows, nb = 3, 5
    en, axc = np.ones(rows, np.uint8), np.full((rows, nb), ord("*"), np.uint8)
    wave = np.zeros((rows, nb * WAVE_BATCH), np.float32)
    state = np.zeros(rows, pkg.TX_STATE_DTYPE)
    cap = rows * (nb + 1)
    records, first, count = np.zeros(cap, pkg.TX_RECORD_DTYPE), np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32)

    def call(**over):
        a = dict(cfg=None, en=ptr(en), rows=rows, axc=ptr(axc), axc_stride=nb, nb=nb, wave=ptr(wave), row_stride=nb * WAVE_BATCH, state=ptr(state),
                 records=ptr(records), cap=cap, first=ptr(first), count=ptr(count))
        a.update(over)
        return L.mi_tx_plan_host(*a.values())

    assert call() == 0 and count[0] == rows
    state[:] = 0
    for name in ("en", "axc", "state", "records", "first", "count"):
        refused(pkg, call(**{name: None}), INVALID, NULL)
    geometry = b"tx plan needs rows >= 1, 1 <= nbatches <= axc_stride and max_records >= 1"
    for over in (dict(rows=0), dict(rows=-1), dict(nb=0), dict(nb=-1), dict(axc_stride=nb - 1), dict(cap=0)):
        refused(pkg, call(**over), INVALID, geometry)
    refused(pkg, call(row_stride=nb * WAVE_BATCH - 1), INVALID, STRIDE)
    assert call(wave=None, row_stride=0) == 0  # (no audio, no stride to check)
    state[:] = 0
    refused(pkg, call(rows=1 << 20, nb=1 << 12, axc_stride=1 << 12, wave=None), INVALID,
            b"tx plan: rows * (nbatches + 1) does not fit the 32-bit record count")
    for field, value in (("open", 2), ("active", 2), ("zero", 1)):
        state[:] = 0
        state[field][rows - 1] = value
        before = state.copy()
        refused(pkg, call(), INVALID, b"tx plan: malformed state blob")
        assert np.array_equal(state, before)
