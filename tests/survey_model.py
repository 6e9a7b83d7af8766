"""Reference model of the band survey (mi_survey_*, csrc/survey.hip) and the small captures its tests share.

The model is the oracle's, not a twin of the code under test: per window the float32 converted x windowed samples exactly as the
oracle's convert_window forms them (ao_levels_u8 / ao_levels_s8 tables, scale * sample * window for s16 / f32, ao_window), through
the oracle's ao_fft_forward, and the float32 magnitude sqrtf(re * re + im * im).  Per cell of `wpc` consecutive windows and per bin:
  peak = the max of those magnitudes                    (order-free: the device must match bit for bit)
  mean = their float64 sum / wpc, kept in float64       (the device's float32 must be the correctly rounded value or its neighbour)
The oracle library is bound here with ctypes (ao_fft_plan_init / ao_fft_forward / ao_window / ao_levels_u8 / ao_levels_s8)."""
import ctypes as C

import numpy as np

import libs

CENTRE = 120000000
SFMT_U8, SFMT_S8, SFMT_S16, SFMT_F32 = 1, 2, 3, 4
SAMPLE_DTYPE = {SFMT_U8: np.uint8, SFMT_S8: np.int8, SFMT_S16: np.int16, SFMT_F32: np.float32}
WAVE_RATE = 16000


class FftPlan(C.Structure):  # ao_fft_plan
    _fields_ = [("log2n", C.c_int), ("n", C.c_size_t), ("tw_re", C.c_void_p), ("tw_im", C.c_void_p), ("bitrev", C.c_void_p)]


_plans = {}


def _oracle():
    lib = libs.oracle_lib()
    if not getattr(lib, "_survey_bound", False):
        lib.ao_fft_plan_init.argtypes = [C.POINTER(FftPlan), C.c_int]
        lib.ao_fft_plan_init.restype = C.c_int
        lib.ao_fft_forward.argtypes = [C.POINTER(FftPlan), C.c_void_p, C.c_void_p]
        lib.ao_fft_forward.restype = None
        lib.ao_levels_u8.argtypes = [libs.f32p]
        lib.ao_levels_u8.restype = None
        lib.ao_levels_s8.argtypes = [libs.f32p]
        lib.ao_levels_s8.restype = None
        lib._survey_bound = True
    return lib


def fft_plan(log2n):
    if log2n not in _plans:
        p = FftPlan()
        assert _oracle().ao_fft_plan_init(C.byref(p), log2n) == 0
        _plans[log2n] = p
    return _plans[log2n]


def hop_samples(sample_rate):
    return int(round(sample_rate / WAVE_RATE))  # rtl_airband.cpp:416


# ------------------------------------------------------------------ the LDS a workgroup of k_survey / k_probe asks for
# Restated from FftGeom (csrc/fft_radix8.hpp) and from survey_lds_bytes / probe_lds_bytes (csrc/survey.hip, csrc/probe.hip), the one
# function per stage that both its create and its launcher call.  mi_survey_create and mi_probe_create refuse a geometry that needs
# more than LDS_LIMIT; tests/test_poststage_refusals.py pins these formulas to the library on both sides of the limit.

LDS_LIMIT = 160 * 1024
COMPLEX_BYTES = {SFMT_U8: 2, SFMT_S8: 2, SFMT_S16: 4, SFMT_F32: 8}


def fft_geom(log2n):
    """FftGeom<log2n>: dict of N, TPF (lanes per FFT), BLOCK, F (FFTs side by side in a workgroup), TW (windows per piece), XN"""
    n = 1 << log2n
    tpf = n // 8
    block = max(256, tpf)
    return dict(N=n, TPF=tpf, BLOCK=block, F=block // tpf, TW=64 if log2n <= 10 else {11: 32, 12: 16, 13: 8}[log2n], XN=n + n // 8)


def lds_bytes(stage, log2n, sfmt, hop_samples_):
    """stage "survey" or "probe": span of TW windows + 1 KB level table + F exchange slots; the survey's fold region lies over them"""
    g = fft_geom(log2n)
    span = ((g["TW"] - 1) * hop_samples_ * COMPLEX_BYTES[sfmt] + g["N"] * COMPLEX_BYTES[sfmt] + 16 + 15) & ~15
    work = span + 1024 + g["F"] * g["XN"] * 8
    fold = g["F"] * g["N"] * 12 if stage == "survey" and g["F"] > 1 else 0
    return max(work, fold)


def largest_hop(stage, log2n, sfmt):
    """the largest hop in samples whose LDS need does not exceed LDS_LIMIT (the need grows with the hop)"""
    hop = 1
    while lds_bytes(stage, log2n, sfmt, hop + 1) <= LDS_LIMIT:
        hop += 1
    assert lds_bytes(stage, log2n, sfmt, hop) <= LDS_LIMIT < lds_bytes(stage, log2n, sfmt, hop + 1)
    return hop


def window(n):
    w = np.zeros(n, np.float32)
    _oracle().ao_window(w, n)
    return w


def levels(sfmt):
    out = np.zeros(256, np.float32)
    (_oracle().ao_levels_u8 if sfmt == SFMT_U8 else _oracle().ao_levels_s8)(out)
    return out


def samples_needed(dev, nwin):
    """complex samples a run of nwin windows covers"""
    return (nwin - 1) * hop_samples(dev.sample_rate) + (1 << dev.fft_size_log)


def converted(dev, raw):
    """raw: the capture as interleaved I, Q of the format's type -> float32 [samples][2], the oracle's conversion without the window"""
    raw = np.asarray(raw)
    assert raw.dtype == SAMPLE_DTYPE[dev.sfmt] and raw.ndim == 1 and raw.size % 2 == 0
    if dev.sfmt in (SFMT_U8, SFMT_S8):
        x = levels(dev.sfmt)[raw.view(np.uint8)]
    else:
        scale = np.float32(1.0) / np.float32(dev.fullscale)
        x = scale * raw.astype(np.float32)  # exact for int16; float32 product, rounded once
    return x.reshape(-1, 2)


def windowed(dev, raw, first, count):
    """float32 [count][N][2]: windows first .. first + count - 1 of the capture, converted x window"""
    n, hop = 1 << dev.fft_size_log, hop_samples(dev.sample_rate)
    x = converted(dev, raw)
    assert x.shape[0] >= (first + count - 1) * hop + n, "capture too short"
    idx = (first + np.arange(count))[:, None] * hop + np.arange(n)[None, :]
    return np.ascontiguousarray(x[idx] * window(n)[None, :, None])


def spectra(dev, raw, first, count):
    """float32 [count][N][2] through the oracle's ao_fft_forward"""
    xin = windowed(dev, raw, first, count)
    out = np.empty_like(xin)
    lib, plan = _oracle(), fft_plan(dev.fft_size_log)
    fwd, pp = lib.ao_fft_forward, C.byref(plan)
    a, b, step = xin.ctypes.data, out.ctypes.data, xin.strides[0]
    for i in range(count):
        fwd(pp, a + i * step, b + i * step)
    return out


def magnitudes(dev, raw, first, count):
    """float32 [count][N]: sqrtf(re * re + im * im), products and sum rounded one by one"""
    z = spectra(dev, raw, first, count)
    re, im = z[..., 0], z[..., 1]
    return np.sqrt(re * re + im * im)


def survey_model(dev, raw, wpc, ncells):
    """(mean float64 [ncells][N], peak float32 [ncells][N]) of one stream's capture"""
    n = 1 << dev.fft_size_log
    mean = np.zeros((ncells, n), np.float64)
    peak = np.zeros((ncells, n), np.float32)
    for c in range(ncells):
        m = magnitudes(dev, raw, c * wpc, wpc)
        assert m.dtype == np.float32
        peak[c] = m.max(axis=0)
        mean[c] = m.astype(np.float64).sum(axis=0) / wpc
    return mean, peak


def ulps_from_rounded(got32, want64):
    """distance in float32 steps between got32 and the correctly rounded float32 of want64 (non-negative finite values)"""
    want32 = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(np.asarray(got32, np.float32).view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------ captures

def noise_and_carriers(pkg, sample_rate, nsamples, carriers, stream=0, seed=0x5EED, amp_q8=3072, gate_samples=0):
    """u8 interleaved I, Q from mi_iqgen_host: sigma = 2 LSB noise plus one AM carrier (12 LSB) per (offset_hz, gate_phase) pair.
    gate_samples 0: every carrier is always on; else a carrier is on while ((sample / gate_samples) + gate_phase) is odd -- a carrier
    that is always on beside gated ones is the same offset listed with phases 0 and 1 (its phase is a function of the sample)."""
    cfg = pkg.iqgen_cfg(sample_rate=sample_rate, seed=seed, gate_samples=gate_samples, carriers=[(off, 0, amp_q8, ph) for off, ph in carriers])
    return pkg.iqgen_host(cfg, stream, 0, nsamples)


def as_format(u8, sfmt):
    """the same signal in another sample format, written by hand from the u8 bytes: s8 = u8 - 128; s16 = (u8 - 128) * 211 + 17 (uses
    the low byte too); f32 = (u8 - 127.5) / 64, to go with fullscale 2.0"""
    u8 = np.asarray(u8, np.uint8)
    if sfmt == SFMT_U8:
        return u8
    if sfmt == SFMT_S8:
        return (u8.astype(np.int16) - 128).astype(np.int8)
    if sfmt == SFMT_S16:
        return ((u8.astype(np.int32) - 128) * 211 + 17).astype(np.int16)
    return ((u8.astype(np.float32) - np.float32(127.5)) / np.float32(64.0)).astype(np.float32)
