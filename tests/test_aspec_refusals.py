"""What the audio spectrum stage refuses, and in which words, without a GPU: mi_aspec_create, every entry point on a NULL handle, the
host-only calls and the twin.  A call that is refused must be refused with the code and the bytes of mi_last_error() stated here."""
import ctypes as C

import numpy as np
import pytest

INVALID, NO_DEVICE = -1, -2
NULL = b"NULL argument"
GEOMETRY = b"audio spectrum stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
BAND = b"audio spectrum stage: the band needs 1 <= lo_bin <= hi_bin <= 1023 (lo_hz 0 = 60, hi_hz 0 = 3800)"
ROW_MEAN = b"audio spectrum stage: a row mean needs the power rows, the row starts and the row counts"
RATIO = b"audio spectrum stage: the ratio must be finite and not negative (0 = 16)"
STRIDE = b"a row stride is shorter than the call"
PLAN = b"audio spectrum plan needs rows >= 1 and nbatches >= 1"
WAVE_BATCH, BINS = 2000, 1024
# on both sides of every edge of the band rule: lo_bin = ceil(lo_hz * 2048 / 16000), hi_bin = floor(hi_hz * 2048 / 16000)
BANDS_REFUSED = [(3801, 3800), (3797, 3800), (60, 7), (60, 8000), (60, 100000), (8000, 0), (4000, 0), (0, 62), (0xFFFFFFFF, 0xFFFFFFFF)]
BANDS_ACCEPTED = {(0, 0): (8, 486), (60, 3800): (8, 486), (1, 8): (1, 1), (3796, 3800): (486, 486), (60, 7999): (8, 1023), (0, 63): (8, 8),
                  (62, 0): (8, 486), (63, 0): (9, 486), (7992, 7999): (1023, 1023), (300, 3000): (39, 384)}


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def refused(pkg, rc, code, text):
    assert rc == code
    assert pkg.lib().mi_last_error() == text


@pytest.fixture()
def L(pkg):
    return pkg.lib()


def test_create_and_the_null_handle(pkg, L):
    out = C.c_void_p()
    some = np.zeros(64, np.uint8)
    create = L.mi_aspec_create
    refused(pkg, create(None, 4, 1, 0, 0, None), INVALID, NULL)
    for rows, max_batches in ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, 1 << 12), ((1 << 20) - 1, 17)):
        refused(pkg, create(None, rows, max_batches, 0, 0, C.byref(out)), INVALID, GEOMETRY)
    for lo, hi in BANDS_REFUSED:
        refused(pkg, create(C.byref(pkg.AspecCfg(lo, hi)), 4, 1, 0, 0, C.byref(out)), INVALID, BAND)
    assert not out.value
    if pkg.device_count() < 1:
        refused(pkg, create(None, 4, 1, 0, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the audio spectrum stage runs on the GPU only")
        refused(pkg, create(C.byref(pkg.AspecCfg(300, 3000)), 4, 2, 3, -1, C.byref(out)), NO_DEVICE,
                b"no HIP device: the audio spectrum stage runs on the GPU only")
        assert not out.value
    # every other entry point refuses a NULL handle, and a NULL argument, before it looks at anything else
    refused(pkg, L.mi_aspec_process_device(None, ptr(some), 0, 1, ptr(some), ptr(some), ptr(some), ptr(some), None, None, None, None), INVALID, NULL)
    refused(pkg, L.mi_aspec_download(None, None, None, None, None, None, ptr(some)), INVALID, NULL)
    refused(pkg, L.mi_aspec_set_timing(None, 1), INVALID, NULL)
    refused(pkg, L.mi_aspec_last_launch_ms(None, ptr(some)), INVALID, NULL)
    L.mi_aspec_destroy(None)


def test_band_and_window(pkg, L):
    lo, hi = C.c_uint32(77), C.c_uint32(77)
    refused(pkg, L.mi_aspec_band(None, None, C.byref(hi)), INVALID, NULL)
    refused(pkg, L.mi_aspec_band(None, C.byref(lo), None), INVALID, NULL)
    refused(pkg, L.mi_aspec_window(None), INVALID, NULL)
    for band in BANDS_REFUSED:
        refused(pkg, L.mi_aspec_band(C.byref(pkg.AspecCfg(*band)), C.byref(lo), C.byref(hi)), INVALID, BAND)
        assert (lo.value, hi.value) == (77, 77)
    for band, bins in BANDS_ACCEPTED.items():
        assert pkg.aspec_band(*band) == bins, band
    assert L.mi_aspec_band(None, C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == (8, 486)


def test_the_twin_and_the_vote(pkg, L):
    rows, nb = 2, 2
    wave = np.zeros((rows, nb * WAVE_BATCH), np.float32)
    index = np.array([[0, 0], [1, 1]], np.uint32)
    first = np.array([0, 1, 2], np.uint32)
    rec = np.zeros(2, pkg.ASPEC_RECORD_DTYPE)
    power, mean, blocks = np.zeros((2, BINS), np.float32), np.zeros((rows, BINS), np.float32), np.zeros(rows, np.uint32)
    plan = L.mi_aspec_plan_host

    def call(cfg=None, rows_=rows, nb_=nb, wave_=ptr(wave), stride=nb * WAVE_BATCH, index_=ptr(index), n=2, first_=ptr(first), rec_=ptr(rec),
             power_=ptr(power), mean_=ptr(mean), blocks_=ptr(blocks)):
        return plan(cfg, rows_, nb_, wave_, stride, index_, n, first_, rec_, power_, mean_, blocks_)

    assert call() == 0 and (rec["peak_bin"] == 8).all() and (blocks == 1).all()
    assert call(n=0, index_=None, rec_=None, power_=None) == 0 and (blocks == 0).all()  # an empty index is a call like any other
    assert call(first_=None, mean_=None, blocks_=None) == 0 and call(power_=None, first_=None, mean_=None, blocks_=None) == 0
    for bad in (dict(wave_=None), dict(index_=None), dict(rec_=None)):
        refused(pkg, call(**bad), INVALID, NULL)
    for bad in (dict(rows_=0), dict(nb_=0), dict(rows_=-1)):
        refused(pkg, call(**bad), INVALID, PLAN)
    refused(pkg, call(stride=nb * WAVE_BATCH - 1), INVALID, STRIDE)
    refused(pkg, call(cfg=C.byref(pkg.AspecCfg(4000, 0))), INVALID, BAND)
    for bad in (dict(power_=None), dict(first_=None), dict(blocks_=None), dict(mean_=None)):
        refused(pkg, call(**bad), INVALID, ROW_MEAN)
    vote = L.mi_aspec_notch_host
    out = pkg.AspecNotch()
    row = np.ones(BINS, np.float32)
    assert vote(ptr(row), 8, None, 0, None, None, C.byref(out)) == 0
    refused(pkg, vote(None, 8, None, 0, None, None, C.byref(out)), INVALID, NULL)
    refused(pkg, vote(ptr(row), 8, None, 0, None, None, None), INVALID, NULL)
    refused(pkg, vote(ptr(row), 8, None, 1, None, None, C.byref(out)), INVALID, NULL)
    refused(pkg, vote(ptr(row), 8, None, 0, C.byref(pkg.AspecCfg(0, 62)), None, C.byref(out)), INVALID, BAND)
    for ratio in (-1.0, float("inf"), float("nan")):
        refused(pkg, vote(ptr(row), 8, None, 0, None, C.byref(pkg.AspecRule(0, ratio)), C.byref(out)), INVALID, RATIO)


def test_sizes_and_symbols(pkg, L):
    assert pkg.ASPEC_RECORD_DTYPE.itemsize == C.sizeof(pkg.AspecRecord) == 32 and C.sizeof(pkg.AspecNotch) == 40
    assert C.sizeof(pkg.AspecCfg) == C.sizeof(pkg.AspecRule) == 8
    assert [pkg.ASPEC_RECORD_DTYPE.fields[n][1] for n in ("row", "batch", "peak_bin", "peak_power", "band_power", "line_power")] == [0, 4, 8, 12, 16, 24]
    for name in ("mi_aspec_create", "mi_aspec_destroy", "mi_aspec_process_device", "mi_aspec_download", "mi_aspec_set_timing", "mi_aspec_last_launch_ms",
                 "mi_aspec_window", "mi_aspec_band", "mi_aspec_plan_host", "mi_aspec_notch_host"):
        assert name in pkg.ABI_SYMBOLS and hasattr(L, name), name
