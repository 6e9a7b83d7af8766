"""boondock-airband_amd -- Python view of the MI355X-native demodulate() path.

The product is `libmi_airband.so` (C ABI in include/mi_airband.h, HIP kernels in csrc/).  This module is a
thin ctypes binding used by tests/ and bench.py; it holds no DSP of its own and there is no CPU fallback:
if the shared library is missing it raises, and compute entry points fail with MI_ERR_NO_DEVICE when no
GPU is visible.

The directory name contains a hyphen (it mirrors the reference's project name), so it is loaded with
importlib under the module name `boondock_airband_amd` -- see tests/conftest.py and __graft_entry__.py.
"""
import ctypes as C
import os

import numpy as np

try:
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.so.7.  Importing torch first
    # makes libmi_airband.so (NEEDED libamdhip64.so.7) bind to that already-loaded copy; the other order
    # loads two runtimes and the second one finds no GPU.
    import torch  # noqa: F401
except ImportError:  # the C ABI itself has no torch dependency
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MI_AIRBAND_LIB") or os.path.join(_HERE, "libmi_airband.so")  # (the override: A/B of two builds, tools/ab_bench.sh)

WAVE_RATE = 16000
WAVE_BATCH = 2000
MAX_IN_FLIGHT = 3  # staging slots of mi_demod_submit (mi_airband.cpp, kSlots)
AGC_EXTRA = 100

MOD_AM, MOD_NFM = 0, 1
OPT_EARLY_INPUT = 1  # MI_OPT_EARLY_INPUT
OPT_STEADY_BLOCKS = 2  # MI_OPT_STEADY_BLOCKS
OPT_TIME_PARALLEL = 3  # result-neutral tuning switches (include/mi_airband.h)
OPT_PRUNE_FFT = 4
OPT_U8_CONVERSION = 5
OPT_UNI_ROWS = 6
OPT_TP_CHUNKS = 7
OPT_TP_RATIO_PCT = 8
OPT_TP_SEG_LANES = 9
OPT_LANE_FFT = 10
OPT_LANE_FFT_JIT = 11
OPT_CORE_SPLIT = 12
OPT_SPEC_HEAD = 13
OPT_PRE_WAVE = 14
OPT_RESERVE_CUS = 15
OPT_AUDIO_WAVE = 16
OPT_MIXED_PLAN = 17
OPT_SPLIT_CUS = 18
SFMT_U8, SFMT_S8, SFMT_S16, SFMT_F32 = 1, 2, 3, 4

MI_OK, MI_ERR_INVALID, MI_ERR_NO_DEVICE, MI_ERR_NOMEM, MI_ERR_HIP, MI_ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5


class MiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mi_airband error {code}: {msg}")
        self.code = code


class DeviceCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int), ("centerfreq", C.c_int), ("fft_size_log", C.c_int), ("sfmt", C.c_int),
                ("fullscale", C.c_float), ("tau", C.c_int), ("fm_quadri", C.c_int)]


class ChannelCfg(C.Structure):
    _fields_ = [("freq", C.c_int), ("modulation", C.c_int), ("squelch_threshold_dbfs", C.c_int), ("has_snr_threshold", C.c_int),
                ("squelch_snr_db", C.c_float), ("notch_freq", C.c_float), ("notch_q", C.c_float), ("ctcss_freq", C.c_float),
                ("bandwidth", C.c_int), ("ampfactor", C.c_float), ("tau", C.c_int), ("afc", C.c_int), ("has_iq_outputs", C.c_int)]


class ChannelStats(C.Structure):
    _fields_ = [("noise_level", C.c_float), ("signal_level", C.c_float), ("squelch_level", C.c_float), ("agcavgfast", C.c_float),
                ("open_count", C.c_uint64), ("flappy_count", C.c_uint64), ("ctcss_count", C.c_uint64), ("no_ctcss_count", C.c_uint64),
                ("active_counter", C.c_uint64), ("squelch_state", C.c_int32), ("signal_outside_filter", C.c_int32)]


class ChannelDerived(C.Structure):
    _fields_ = [("bin", C.c_uint32), ("dm_dphi", C.c_uint32), ("needs_raw_iq", C.c_int32), ("has_iq_outputs", C.c_int32),
                ("modulation", C.c_int32), ("using_manual_level", C.c_int32), ("manual_signal_level", C.c_float),
                ("normal_signal_ratio", C.c_float), ("flappy_signal_ratio", C.c_float), ("ampfactor", C.c_float), ("alpha", C.c_float),
                ("notch_enabled", C.c_int32), ("notch_d", C.c_float * 3), ("lowpass_enabled", C.c_int32), ("lowpass_gain", C.c_float),
                ("lowpass_ycoeffs", C.c_float * 2), ("ctcss_enabled", C.c_int32), ("ctcss_fast_window", C.c_int32),
                ("ctcss_slow_window", C.c_int32), ("ctcss_fast_ndet", C.c_int32), ("ctcss_slow_ndet", C.c_int32)]


class IqGenCarrier(C.Structure):
    _fields_ = [("offset_hz", C.c_int32), ("kind", C.c_int32), ("amp_q8", C.c_int32), ("gate_phase", C.c_int32)]


class IqGenCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("seed", C.c_uint64), ("noise_q8_mul", C.c_int32), ("gate_samples", C.c_uint64),
                ("ncarriers", C.c_int32), ("carriers", IqGenCarrier * 64)]


# every symbol include/mi_airband.h declares
class MixInput(C.Structure):  # mi_mix_input
    _fields_ = [("row", C.c_int), ("ampfactor", C.c_float), ("balance", C.c_float)]


class GateBlock(C.Structure):  # mi_gate_block
    _fields_ = [("row", C.c_uint32), ("batch", C.c_uint32)]


GATE_NONE, GATE_OPEN, GATE_OPEN_TRAIL, GATE_ALL = 0, 1, 2, 3  # MI_GATE_*


class TxCfg(C.Structure):  # mi_tx_cfg: 0 = the reference's 8 / 4 / 28800 batches
    _fields_ = [("min_batches", C.c_uint32), ("idle_batches", C.c_uint32), ("max_batches", C.c_uint32)]


class TxRecord(C.Structure):  # mi_tx_record
    _fields_ = [("row", C.c_uint32), ("seq", C.c_uint32), ("first_block", C.c_uint32), ("nblocks", C.c_uint32), ("first_batch", C.c_uint32),
                ("close_batch", C.c_uint32), ("flags", C.c_uint32), ("peak", C.c_float), ("energy", C.c_double)]


TX_RECORD_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in TxRecord._fields_])  # the same 40 bytes as a numpy record
TX_STATE_DTYPE = np.dtype([("clock", "<u8"), ("opened", "<u8"), ("last_write", "<u8"), ("seq", "<u4"), ("open", "u1"), ("active", "u1"),
                           ("zero", "<u2")])  # one row of the splitter's state blob, MI_TX_STATE_ROW_BYTES = 32
TX_NONE = 0xFFFFFFFF  # first_batch of a record without blocks, close_batch of a file still open


class TonesCfg(C.Structure):  # mi_tones_cfg: 0 = 6400 samples
    _fields_ = [("window_samples", C.c_uint32)]


class ToneRecord(C.Structure):  # mi_tone_record
    _fields_ = [("row", C.c_uint32), ("seq", C.c_uint32), ("end_batch", C.c_uint32), ("end_sample", C.c_uint32), ("best", C.c_uint32),
                ("second", C.c_uint32), ("best_power", C.c_float), ("second_power", C.c_float), ("mean_power", C.c_float), ("zero", C.c_uint32)]


class TonesRule(C.Structure):  # mi_tones_rule: 0 = 2 windows / 500 permille
    _fields_ = [("min_windows", C.c_uint32), ("min_share_permille", C.c_uint32)]


class TonesVote(C.Structure):  # mi_tones_vote
    _fields_ = [("windows", C.c_uint32), ("votes", C.c_uint32), ("tone", C.c_uint32), ("freq_hz", C.c_float), ("share", C.c_double),
                ("found", C.c_uint32), ("zero", C.c_uint32)]


TONES_STANDARD, TONES_LANES = 51, 64  # MI_TONES_STANDARD, MI_TONES_LANES
TONE_RECORD_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in ToneRecord._fields_])  # the same 40 bytes as a numpy record
TONES_STATE_DTYPE = np.dtype([("count", "<u4"), ("seq", "<u4"), ("q1", "<f4", (TONES_LANES,)), ("q2", "<f4", (TONES_LANES,))])  # MI_TONES_STATE_ROW_BYTES = 520


class PcmCfg(C.Structure):  # mi_pcm_cfg: 0 = 8000 / PCM_S16
    _fields_ = [("rate", C.c_uint32), ("format", C.c_uint32)]


PCM_S16, PCM_IMA4 = 1, 2  # MI_PCM_*
PCM_TAPS, PCM_HISTORY = 63, 62  # MI_PCM_TAPS, MI_PCM_HISTORY
PCM_STATE_DTYPE = np.dtype([("x", "<f4", (PCM_HISTORY,))])  # one row of the PCM stage's state blob, MI_PCM_STATE_ROW_BYTES = 248


class VbandRow(C.Structure):  # mi_vband_row: 0 = no edge on that side
    _fields_ = [("hp_hz", C.c_uint32), ("lp_hz", C.c_uint32)]


VBAND_TAPS, VBAND_HISTORY = 511, 510  # MI_VBAND_TAPS, MI_VBAND_HISTORY
VBAND_ROW_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in VbandRow._fields_])  # the same 8 bytes as a numpy record
VBAND_STATE_DTYPE = np.dtype([("x", "<f4", (VBAND_HISTORY,))])  # one row of the voice band stage's state blob, MI_VBAND_STATE_ROW_BYTES = 2040


class LimitRow(C.Structure):  # mi_limit_row
    _fields_ = [("pregain", C.c_float), ("ceiling", C.c_float)]


LIMIT_LOOKAHEAD, LIMIT_WINDOW, LIMIT_HISTORY = 63, 1024, 1086  # MI_LIMIT_*
LIMIT_ROW_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in LimitRow._fields_])  # the same 8 bytes as a numpy record
LIMIT_STATE_DTYPE = np.dtype([("x", "<f4", (LIMIT_HISTORY,))])  # one row of the limiter stage's state blob, MI_LIMIT_STATE_ROW_BYTES = 4344


class DenoiseRow(C.Structure):  # mi_denoise_row
    _fields_ = [("reduction_db", C.c_float), ("over", C.c_float)]


DENOISE_HOP, DENOISE_FRAME, DENOISE_FFT, DENOISE_BINS, DENOISE_DEPTH = 250, 500, 512, 257, 8  # MI_DENOISE_*
DENOISE_ROW_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in DenoiseRow._fields_])  # the same 8 bytes as a numpy record
# one row of the noise reduction stage's state blob, MI_DENOISE_STATE_ROW_BYTES = 9196
DENOISE_STATE_DTYPE = np.dtype([("x", "<f4", (DENOISE_FRAME,)), ("m", "<f4", (DENOISE_DEPTH - 1, DENOISE_BINS))])


class SelcalCfg(C.Structure):  # mi_selcal_cfg: 0 = MI_SELCAL_16 and the default of every setting
    _fields_ = [("mode", C.c_uint32), ("ntones", C.c_uint32), ("freq", C.c_float * 32), ("min_energy", C.c_float), ("min_tonality", C.c_float),
                ("max_twist", C.c_float), ("min_separation", C.c_float), ("min_run", C.c_uint32), ("max_run", C.c_uint32), ("max_gap", C.c_uint32),
                ("zero", C.c_uint32)]


SELCAL_16, SELCAL_32, SELCAL_CUSTOM = 0, 1, 2  # MI_SELCAL_*
SELCAL_WINDOW, SELCAL_HOP, SELCAL_HISTORY, SELCAL_MAX_TONES = 2000, 1000, 1002, 32
SELCAL_NONE, SELCAL_NONE8 = 0, 0xFF  # no pair; no third tone in a table of two
SELCAL_IDLE, SELCAL_FIRST, SELCAL_OVER, SELCAL_GAP, SELCAL_SECOND, SELCAL_DONE = range(6)
# mi_selcal_window_record (24 bytes), mi_selcal_code (32 bytes), and one row of the SELCAL stage's state blob, MI_SELCAL_STATE_ROW_BYTES = 4048
SELCAL_WINDOW_DTYPE = np.dtype([("best", "u1"), ("second", "u1"), ("third", "u1"), ("zero", "u1"), ("p_best", "<f4"), ("p_second", "<f4"),
                                ("p_third", "<f4"), ("energy", "<f4"), ("pair", "<u4")])
SELCAL_CODE_DTYPE = np.dtype([("row", "<u4"), ("seq", "<u4"), ("tone", "u1", (4,)), ("first_window", "<u4"), ("last_window", "<u4"), ("run1", "<u4"),
                              ("gap", "<u4"), ("batch", "<u4")])
SELCAL_STATE_DTYPE = np.dtype([("x", "<f4", (SELCAL_HISTORY,)), ("window", "<u4"), ("seq", "<u4"), ("phase", "<u4"), ("pair1", "<u4"), ("pair2", "<u4"),
                               ("run1", "<u4"), ("run2", "<u4"), ("gap", "<u4"), ("first_window", "<u4"), ("zero", "<u4")])


class AcarsCfg(C.Structure):  # mi_acars_cfg: 0 = the default of every setting
    _fields_ = [("sync_errors", C.c_uint32), ("keep_bad", C.c_uint32), ("min_quality", C.c_float), ("hold_timing", C.c_uint32)]


class AcarsText(C.Structure):  # mi_acars_text
    _fields_ = [("mode", C.c_char * 2), ("address", C.c_char * 8), ("ack", C.c_char * 2), ("label", C.c_char * 3), ("block_id", C.c_char * 2),
                ("text", C.c_char * 231)]


ACARS_HISTORY, ACARS_HYPOTHESES, ACARS_BITS, ACARS_BIT_WORDS, ACARS_SYNC_BITS, ACARS_HEAD_BYTES, ACARS_MAX_BYTES, ACARS_RAW_BYTES = 6, 20, 300, 10, 39, 12, 240, 248
ACARS_IDLE, ACARS_FRAME = 0, 1  # MI_ACARS_*
ACARS_SYNC_EXACT = 0x80000000  # mi_acars_cfg.sync_errors: no mismatch allowed
# mi_acars_frame (272 bytes) and one row of the ACARS stage's state blob, MI_ACARS_STATE_ROW_BYTES = 496
ACARS_FRAME_DTYPE = np.dtype([("row", "<u4"), ("batch", "<u4"), ("third", "<u4"), ("tau_sync", "u1"), ("tau_end", "u1"), ("sync_errors", "u1"),
                              ("crc_ok", "u1"), ("nbytes", "<u2"), ("parity_errors", "u1"), ("end", "u1"), ("end_batch", "<u4"),
                              ("bytes", "u1", (ACARS_RAW_BYTES,))])
ACARS_STATE_DTYPE = np.dtype([("x", "<f4", (ACARS_HISTORY,)), ("batch", "<u4"), ("phase", "<u4"), ("hist", "<u8", (ACARS_HYPOTHESES,))] +
                             [(n, "<u4") for n in ("u", "prev", "nbits", "cur", "nbytes", "tail", "crc", "parity_errors", "start_batch", "start_third",
                                                   "tau_sync", "mismatches", "end", "zero")] + [("bytes", "u1", (ACARS_RAW_BYTES,))])


class SameCfg(C.Structure):  # mi_same_cfg: 0 = the default of every setting
    _fields_ = [("sync_errors", C.c_uint32), ("max_bad", C.c_uint32), ("gap_batches", C.c_uint32), ("min_quality", C.c_float), ("space_gain", C.c_float),
                ("hold_timing", C.c_uint32)]


class SameText(C.Structure):  # mi_same_text
    _fields_ = [("originator", C.c_char * 4), ("event", C.c_char * 4), ("purge", C.c_char * 5), ("issue", C.c_char * 8), ("station", C.c_char * 9),
                ("pad", C.c_char * 2), ("nlocations", C.c_uint32), ("locations", (C.c_char * 7) * 31), ("pad2", C.c_char * 3)]


SAME_HISTORY, SAME_HYPOTHESES, SAME_BIT_UNITS, SAME_BATCH_UNITS, SAME_BIT_WORDS, SAME_MAX_BITS, SAME_MAX_BYTES, SAME_RAW_BYTES, SAME_DEAF = 30, 16, 768, 50000, 4, 66, 268, 272, 64
SAME_IDLE, SAME_BURST = 0, 1  # MI_SAME_*
SAME_HEADER, SAME_EOM = 0, 1
SAME_SYNC_EXACT = 0x80000000  # mi_same_cfg.sync_errors: no mismatch allowed
SAME_WALKER_FIELDS = ("phase", "u", "kind", "nbits", "cur", "nbytes", "nbad", "plus", "dashes", "deaf", "start_batch", "start_unit", "an", "akind", "alen0",
                      "alen1", "atrunc0", "atrunc1", "aidle", "astart_batch", "astart_unit")
# mi_same_message (304 bytes) and one row of the SAME stage's state blob, MI_SAME_STATE_ROW_BYTES = 1160
SAME_MESSAGE_DTYPE = np.dtype([("row", "<u4"), ("kind", "<u4"), ("batch", "<u4"), ("unit", "<u4"), ("end_batch", "<u4"), ("nbursts", "u1"), ("voted", "u1"),
                               ("truncated", "u1"), ("fields_ok", "u1"), ("nbytes", "<u2"), ("agree", "<u2"), ("zero", "<u4"),
                               ("bytes", "u1", (SAME_RAW_BYTES,))])
SAME_STATE_DTYPE = np.dtype([("x", "<f4", (SAME_HISTORY,)), ("batch", "<u4"), ("grid", "<u4"), ("hist", "<u8", (SAME_HYPOTHESES,))] +
                            [(n, "<u4") for n in SAME_WALKER_FIELDS + ("zero",)] + [("bytes", "u1", (3, SAME_RAW_BYTES))])


class Ax25Cfg(C.Structure):  # mi_ax25_cfg: 0 = the default of every setting
    _fields_ = [("gain", C.c_float * 3), ("strict", C.c_uint32)]


AX25_HISTORY, AX25_HYPOTHESES, AX25_SLICERS, AX25_LANES, AX25_BITS, AX25_BIT_WORDS, AX25_MIN_BYTES, AX25_MAX_BYTES, AX25_RAW_BYTES = 14, 10, 3, 30, 150, 5, 17, 330, 332
AX25_WAIT, AX25_FRAME = 0, 1  # MI_AX25_*
AX25_RESIDUE, AX25_FLAG_RESIDUE = 0xF0B8, 0x9F0B
AX25_STRICT_OFF = 0x80000000  # mi_ax25_cfg.strict: frames whose address field is not well formed are records too
AX25_TEXT_BYTES = 384
# mi_ax25_frame (352 bytes) and one row of the packet stage's state blob, MI_AX25_STATE_ROW_BYTES = 10544
AX25_FRAME_DTYPE = np.dtype([("row", "<u4"), ("batch", "<u4"), ("third", "<u4"), ("end_batch", "<u4"), ("nbytes", "<u2"), ("lane", "u1"), ("naddr", "u1"),
                             ("bytes", "u1", (AX25_RAW_BYTES,))])
AX25_STATE_DTYPE = np.dtype([("x", "<f4", (AX25_HISTORY,)), ("batch", "<u8"), ("last_end", "<u8"), ("start", "<u8", (AX25_LANES,)),
                             ("nbytes", "<u2", (AX25_LANES,)), ("crc", "<u2", (AX25_LANES,)), ("prev", "u1", (AX25_LANES,)), ("ones", "u1", (AX25_LANES,)),
                             ("phase", "u1", (AX25_LANES,)), ("nbits", "u1", (AX25_LANES,)), ("cur", "u1", (AX25_LANES,)), ("zero", "u1", (2,)),
                             ("bytes", "u1", (AX25_LANES, AX25_RAW_BYTES))])


class PocsagCfg(C.Structure):  # mi_pocsag_cfg: 0 = the default of every setting
    _fields_ = [("baud", C.c_uint32), ("sync_errors", C.c_uint32), ("preamble_errors", C.c_uint32), ("correct", C.c_uint32), ("hold_timing", C.c_uint32)]


POCSAG_HISTORY, POCSAG_MAX_HYPOTHESES, POCSAG_MAX_LANES, POCSAG_MAX_WORDS, POCSAG_TEXT_BYTES = 34, 15, 30, 80, 408
POCSAG_IDLE, POCSAG_TRANSMISSION = 0, 1  # MI_POCSAG_*
POCSAG_TEXT_AUTO, POCSAG_TEXT_NUMERIC, POCSAG_TEXT_ALPHA = 0, 1, 2
POCSAG_SYNC, POCSAG_IDLE_WORD = 0x7CD215D8, 0x7A89C197
POCSAG_SYNC_EXACT = 0x80000000  # mi_pocsag_cfg.sync_errors: no mismatch allowed
POCSAG_PREAMBLE_EXACT, POCSAG_PREAMBLE_OFF = 0x80000000, 0x80000001  # mi_pocsag_cfg.preamble_errors: none allowed; the condition dropped
POCSAG_CORRECT_NONE = 0x80000000  # mi_pocsag_cfg.correct: a word is good only as received
POCSAG_WALKER_FIELDS = ("lane", "inverted", "pos", "cur", "nbits", "gbad", "lane_sync", "mismatches", "wbatch", "wtwelfth", "open")
# mi_pocsag_message (368 bytes) and one row of the pager stage's state blob, MI_POCSAG_STATE_ROW_BYTES = 800
POCSAG_MESSAGE_DTYPE = np.dtype([("row", "<u4"), ("batch", "<u4"), ("twelfth", "<u4"), ("end_batch", "<u4"), ("address", "<u4"), ("function", "u1"),
                                 ("nwords", "u1"), ("nbad", "u1"), ("truncated", "u1"), ("corrected", "<u2"), ("inverted", "u1"), ("sync_errors", "u1"),
                                 ("lane_sync", "u1"), ("lane_end", "u1"), ("zero", "<u2"), ("bad", "<u4", (3,)), ("zero2", "<u4"),
                                 ("words", "<u4", (POCSAG_MAX_WORDS,))])
POCSAG_STATE_DTYPE = np.dtype([("x", "<f4", (POCSAG_HISTORY,)), ("batch", "<u4"), ("phase", "<u4"), ("hist", "<u8", (POCSAG_MAX_LANES,))] +
                              [(n, "<u4") for n in POCSAG_WALKER_FIELDS + ("zero",)] + [("msg", POCSAG_MESSAGE_DTYPE)])


class AspecCfg(C.Structure):  # mi_aspec_cfg: 0 = 60 / 3800
    _fields_ = [("lo_hz", C.c_uint32), ("hi_hz", C.c_uint32)]


class AspecRecord(C.Structure):  # mi_aspec_record
    _fields_ = [("row", C.c_uint32), ("batch", C.c_uint32), ("peak_bin", C.c_uint32), ("peak_power", C.c_float), ("band_power", C.c_double),
                ("line_power", C.c_double)]


class AspecRule(C.Structure):  # mi_aspec_rule: 0 = 8 blocks / ratio 16.0
    _fields_ = [("min_blocks", C.c_uint32), ("ratio", C.c_float)]


class AspecNotch(C.Structure):  # mi_aspec_notch
    _fields_ = [("found", C.c_uint32), ("bin", C.c_uint32), ("freq_hz", C.c_double), ("peak", C.c_double), ("floor", C.c_double),
                ("votes", C.c_uint32), ("blocks", C.c_uint32)]


ASPEC_FFT, ASPEC_BINS, ASPEC_LINE_HALF = 2048, 1024, 2  # MI_ASPEC_*
ASPEC_NONE = 0xFFFFFFFF  # peak_bin of an index entry that is not of the call
ASPEC_RECORD_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in AspecRecord._fields_])  # the same 32 bytes as a numpy record


class OccCfg(C.Structure):  # mi_occ_cfg: 0 = 250 permille / ratio 3.0 / 1 cell
    _fields_ = [("floor_permille", C.c_uint32), ("ratio", C.c_float), ("min_cells", C.c_uint32)]


class OccBin(C.Structure):  # mi_occ_bin
    _fields_ = [("floor", C.c_float), ("threshold", C.c_float), ("active_cells", C.c_uint32), ("first_cell", C.c_uint32), ("last_cell", C.c_uint32),
                ("runs", C.c_uint32), ("max_mean", C.c_float), ("max_peak", C.c_float)]


class OccCandidate(C.Structure):  # mi_occ_candidate
    _fields_ = [("stream", C.c_uint32), ("best_bin", C.c_uint32), ("lo_bin", C.c_uint32), ("hi_bin", C.c_uint32), ("nbins", C.c_uint32),
                ("active_cells", C.c_uint32), ("first_cell", C.c_uint32), ("last_cell", C.c_uint32), ("max_mean", C.c_float), ("max_peak", C.c_float)]


OCC_BIN_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in OccBin._fields_])  # the same 32 bytes as a numpy record
OCC_CAND_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in OccCandidate._fields_])  # the same 40 bytes
OCC_NONE = 0xFFFFFFFF  # first_cell / last_cell of a bin without an active cell


class ProbeTarget(C.Structure):  # mi_probe_target
    _fields_ = [("stream", C.c_uint32), ("bin", C.c_uint32)]


class ProbeCell(C.Structure):  # mi_probe_cell
    _fields_ = [("s1", C.c_double), ("s2", C.c_double), ("r_re", C.c_double), ("r_im", C.c_double), ("windows", C.c_uint32), ("pairs", C.c_uint32)]


class ProbeFeatures(C.Structure):  # mi_probe_features
    _fields_ = [("s1", C.c_double), ("s2", C.c_double), ("r_re", C.c_double), ("r_im", C.c_double), ("n", C.c_uint64), ("pairs", C.c_uint64),
                ("cv2", C.c_double), ("coherence", C.c_double), ("dphi", C.c_double), ("carrier_hz", C.c_double)]


class ProbeRule(C.Structure):  # mi_probe_rule: 0 = the default
    _fields_ = [("coherence_max", C.c_double), ("cv2_min", C.c_double)]


PROBE_TARGET_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in ProbeTarget._fields_])  # the same 8 bytes as a numpy record
PROBE_CELL_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in ProbeCell._fields_])  # the same 40 bytes


class EltCfg(C.Structure):  # mi_elt_cfg: 0 = the default of every setting
    _fields_ = [("min_energy", C.c_float), ("min_tonality", C.c_float), ("band_lo", C.c_uint32), ("band_hi", C.c_uint32), ("min_span", C.c_uint32),
                ("min_len", C.c_uint32), ("max_len", C.c_uint32), ("max_step", C.c_uint32), ("max_drop", C.c_uint32), ("max_gap", C.c_uint32),
                ("min_sweeps", C.c_uint32), ("zero", C.c_uint32)]


ELT_FRAME, ELT_HOP, ELT_HISTORY, ELT_FRAMES, ELT_BINS, ELT_BIN0, ELT_NONE8 = 256, 80, 178, 25, 32, 2, 0xFF  # MI_ELT_*
ELT_ONSET, ELT_END = 1, 2
ELT_UP, ELT_DOWN = 1, 2
# mi_elt_frame_record (16 bytes), mi_elt_event (32 bytes), and one row of the ELT stage's state blob, MI_ELT_STATE_ROW_BYTES = 776
ELT_FRAME_DTYPE = np.dtype([("best", "u1"), ("bin", "u1"), ("zero", "<u2"), ("energy", "<f4"), ("p_best", "<f4"), ("p3", "<f4")])
ELT_EVENT_DTYPE = np.dtype([("row", "<u4"), ("seq", "<u4"), ("kind", "u1"), ("dir", "u1"), ("bin_from", "u1"), ("bin_to", "u1"), ("frame", "<u4"),
                            ("first_frame", "<u4"), ("last_end", "<u4"), ("sweeps", "<u4"), ("batch", "<u4")])
ELT_STATE_DTYPE = np.dtype([("x", "<f4", (ELT_HISTORY,))] +
                           [(n, "<u4") for n in ("frame", "seq", "open", "start", "first_bin", "last_bin", "last_frame", "dir", "drops", "count", "chain_dir",
                                                 "chain_first", "last_end", "alarmed", "bin_from", "bin_to")])

ABI_SYMBOLS = [
    "mi_last_error", "mi_device_count", "mi_demod_create", "mi_demod_destroy", "mi_demod_prepare", "mi_set_cache_dir", "mi_jit_counts", "mi_demod_bytes_needed", "mi_demod_bytes_consumed",
    "mi_demod_hop_bytes", "mi_demod_process", "mi_demod_submit", "mi_demod_wait", "mi_host_alloc", "mi_host_free", "mi_demod_process_device", "mi_demod_set_active_streams", "mi_demod_get_active_streams", "mi_demod_get_stats", "mi_demod_state_size",
    "mi_demod_get_state", "mi_demod_set_state", "mi_demod_read_planes", "mi_demod_process_planes", "mi_demod_last_path", "mi_demod_last_stage1", "mi_demod_pre_wave_timeouts", "mi_demod_tp_debug", "mi_demod_kernel_time", "mi_demod_kernel_time_prev", "mi_demod_event_ms", "mi_demod_set_option", "mi_demod_last_kernel_ms", "mi_plan_create", "mi_plan_destroy", "mi_plan_fft_size",
    "mi_plan_window", "mi_plan_twiddles", "mi_plan_levels", "mi_plan_sincos_lut", "mi_plan_channel", "mi_plan_lane_fft", "mi_plan_ctcss_coeffs",
    "mi_iqgen_host", "mi_iqgen_device", "mi_mixer_create", "mi_mixer_destroy", "mi_mixer_is_stereo", "mi_mixer_process_device",
    "mi_outgate_create", "mi_outgate_destroy", "mi_outgate_set_rules", "mi_outgate_process_device", "mi_outgate_download", "mi_outgate_state_size",
    "mi_outgate_get_state", "mi_outgate_set_state", "mi_outgate_set_timing", "mi_outgate_last_launch_ms", "mi_gate_plan_host",
    "mi_txsplit_create", "mi_txsplit_destroy", "mi_txsplit_set_rows", "mi_txsplit_process_device", "mi_txsplit_download", "mi_txsplit_state_size",
    "mi_txsplit_get_state", "mi_txsplit_set_state", "mi_txsplit_set_timing", "mi_txsplit_last_launch_ms", "mi_tx_plan_host",
    "mi_tones_create", "mi_tones_destroy", "mi_tones_set_rows", "mi_tones_process_device", "mi_tones_download", "mi_tones_state_size",
    "mi_tones_get_state", "mi_tones_set_state", "mi_tones_set_timing", "mi_tones_last_launch_ms", "mi_tones_plan_host", "mi_tones_table",
    "mi_tones_vote_host",
    "mi_pcm_create", "mi_pcm_destroy", "mi_pcm_set_rows", "mi_pcm_process_device", "mi_pcm_download", "mi_pcm_state_size", "mi_pcm_get_state",
    "mi_pcm_set_state", "mi_pcm_set_timing", "mi_pcm_last_launch_ms", "mi_pcm_block_bytes", "mi_pcm_taps", "mi_pcm_plan_host", "mi_pcm_wav_header",
    "mi_aspec_create", "mi_aspec_destroy", "mi_aspec_process_device", "mi_aspec_download", "mi_aspec_set_timing", "mi_aspec_last_launch_ms",
    "mi_aspec_window", "mi_aspec_band", "mi_aspec_plan_host", "mi_aspec_notch_host",
    "mi_vband_default_row", "mi_vband_create", "mi_vband_destroy", "mi_vband_set_rows", "mi_vband_process_device", "mi_vband_state_size",
    "mi_vband_get_state", "mi_vband_set_state", "mi_vband_set_timing", "mi_vband_last_launch_ms", "mi_vband_taps", "mi_vband_plan_host",
    "mi_limit_default_row", "mi_limit_create", "mi_limit_destroy", "mi_limit_set_rows", "mi_limit_process_device", "mi_limit_state_size",
    "mi_limit_get_state", "mi_limit_set_state", "mi_limit_set_timing", "mi_limit_last_launch_ms", "mi_limit_plan_host", "mi_limit_pregain_host",
    "mi_denoise_default_row", "mi_denoise_create", "mi_denoise_destroy", "mi_denoise_set_rows", "mi_denoise_process_device", "mi_denoise_state_size",
    "mi_denoise_get_state", "mi_denoise_set_state", "mi_denoise_set_timing", "mi_denoise_last_launch_ms", "mi_denoise_window", "mi_denoise_plan_host",
    "mi_selcal_create", "mi_selcal_destroy", "mi_selcal_set_rows", "mi_selcal_process_device", "mi_selcal_download", "mi_selcal_state_size",
    "mi_selcal_get_state", "mi_selcal_set_state", "mi_selcal_set_timing", "mi_selcal_last_launch_ms", "mi_selcal_plan_host", "mi_selcal_table",
    "mi_selcal_settings", "mi_selcal_window", "mi_selcal_code_text",
    "mi_acars_create", "mi_acars_destroy", "mi_acars_set_rows", "mi_acars_process_device", "mi_acars_download", "mi_acars_state_size",
    "mi_acars_get_state", "mi_acars_set_state", "mi_acars_set_timing", "mi_acars_last_launch_ms", "mi_acars_plan_host", "mi_acars_settings",
    "mi_acars_templates", "mi_acars_crc", "mi_acars_frame_text",
    "mi_same_create", "mi_same_destroy", "mi_same_set_rows", "mi_same_process_device", "mi_same_download", "mi_same_state_size",
    "mi_same_get_state", "mi_same_set_state", "mi_same_set_timing", "mi_same_last_launch_ms", "mi_same_plan_host", "mi_same_settings",
    "mi_same_templates", "mi_same_message_text",
    "mi_elt_create", "mi_elt_destroy", "mi_elt_set_rows", "mi_elt_process_device", "mi_elt_download", "mi_elt_state_size", "mi_elt_get_state",
    "mi_elt_set_state", "mi_elt_set_timing", "mi_elt_last_launch_ms", "mi_elt_plan_host", "mi_elt_settings", "mi_elt_window", "mi_elt_coeffs",
    "mi_elt_event_text",
    "mi_ax25_create", "mi_ax25_destroy", "mi_ax25_set_rows", "mi_ax25_process_device", "mi_ax25_download", "mi_ax25_state_size",
    "mi_ax25_get_state", "mi_ax25_set_state", "mi_ax25_set_timing", "mi_ax25_last_launch_ms", "mi_ax25_plan_host", "mi_ax25_settings",
    "mi_ax25_templates", "mi_ax25_crc", "mi_ax25_frame_text",
    "mi_pocsag_create", "mi_pocsag_destroy", "mi_pocsag_set_rows", "mi_pocsag_process_device", "mi_pocsag_download", "mi_pocsag_state_size",
    "mi_pocsag_get_state", "mi_pocsag_set_state", "mi_pocsag_set_timing", "mi_pocsag_last_launch_ms", "mi_pocsag_plan_host", "mi_pocsag_settings",
    "mi_pocsag_geometry", "mi_pocsag_max_messages", "mi_pocsag_encode", "mi_pocsag_decode", "mi_pocsag_message_text",
    "mi_survey_create", "mi_survey_destroy", "mi_survey_set_streams", "mi_survey_bytes_needed", "mi_survey_process_device", "mi_survey_set_timing",
    "mi_survey_last_launch_ms", "mi_survey_bin_range",
    "mi_occupancy_create", "mi_occupancy_destroy", "mi_occupancy_set_streams", "mi_occupancy_process_device", "mi_occupancy_download",
    "mi_occupancy_set_timing", "mi_occupancy_last_launch_ms", "mi_occupancy_plan_host",
    "mi_probe_create", "mi_probe_destroy", "mi_probe_set_targets", "mi_probe_bytes_needed", "mi_probe_process_device", "mi_probe_download",
    "mi_probe_set_timing", "mi_probe_last_launch_ms", "mi_probe_targets_from_candidates", "mi_probe_features_host", "mi_probe_classify_host",
    "mi_gather_unique_id", "mi_gather_loopback_id", "mi_gather_create", "mi_gather_destroy", "mi_gather_audio", "mi_gather_stream_wait", "mi_gather_sync",
]

_lib = None


def lib():
    """The loaded C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `make -C boondock-airband_amd/csrc` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        vp, sz = C.c_void_p, C.c_size_t
        L.mi_last_error.restype = C.c_char_p
        L.mi_device_count.restype = C.c_int
        L.mi_demod_create.argtypes = [C.POINTER(DeviceCfg), C.POINTER(ChannelCfg), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_demod_destroy.argtypes = [vp]
        L.mi_demod_prepare.argtypes = [vp, C.c_int]
        L.mi_set_cache_dir.argtypes = [C.c_char_p]
        L.mi_jit_counts.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_demod_last_stage1.argtypes = [vp, C.POINTER(C.c_int)]
        L.mi_demod_submit.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
        L.mi_demod_wait.argtypes = [vp]
        L.mi_host_alloc.argtypes = [sz]
        L.mi_host_alloc.restype = vp
        L.mi_host_free.argtypes = [vp]
        L.mi_host_free.restype = None
        L.mi_gather_unique_id.argtypes = [vp]
        L.mi_gather_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_gather_destroy.argtypes = [vp]
        L.mi_gather_audio.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        L.mi_gather_stream_wait.argtypes = [vp, vp]
        L.mi_gather_sync.argtypes = [vp]
        L.mi_demod_destroy.restype = None
        for f in (L.mi_demod_bytes_needed, L.mi_demod_bytes_consumed):
            f.argtypes = [vp, C.c_int]
            f.restype = sz
        L.mi_demod_hop_bytes.argtypes = [vp]
        L.mi_demod_hop_bytes.restype = sz
        L.mi_demod_process.argtypes = [vp, C.POINTER(vp), C.c_int, vp, vp, vp, vp]
        L.mi_demod_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp]
        L.mi_demod_get_stats.argtypes = [vp, vp]
        L.mi_demod_set_active_streams.argtypes = [vp, vp]
        L.mi_demod_get_active_streams.argtypes = [vp, vp]
        L.mi_demod_state_size.argtypes = [vp]
        L.mi_demod_state_size.restype = sz
        L.mi_demod_get_state.argtypes = [vp, vp, sz]
        L.mi_demod_set_state.argtypes = [vp, vp, sz]
        L.mi_demod_last_path.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_demod_kernel_time.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.mi_demod_kernel_time_prev.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.mi_demod_event_ms.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.mi_demod_set_option.argtypes = [vp, C.c_int, C.c_int]
        L.mi_demod_tp_debug.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.POINTER(C.c_int)]
        L.mi_demod_read_planes.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
        L.mi_demod_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.mi_mixer_create.argtypes = [C.POINTER(MixInput), C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_mixer_destroy.argtypes = [vp]
        L.mi_mixer_destroy.restype = None
        L.mi_mixer_is_stereo.argtypes = [vp]
        L.mi_mixer_process_device.argtypes = [vp, vp, sz, vp, sz, C.c_int, vp, vp, vp, vp]
        L.mi_outgate_create.argtypes = [vp, vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_outgate_destroy.argtypes = [vp]
        L.mi_outgate_destroy.restype = None
        L.mi_outgate_set_rules.argtypes = [vp, vp]
        L.mi_outgate_process_device.argtypes = [vp, vp, sz, vp, sz, vp, sz, C.c_int, vp, vp, vp, vp, vp, vp]
        L.mi_outgate_download.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.mi_outgate_state_size.argtypes = [vp]
        L.mi_outgate_state_size.restype = sz
        L.mi_outgate_get_state.argtypes = [vp, vp, sz]
        L.mi_outgate_set_state.argtypes = [vp, vp, sz]
        L.mi_outgate_set_timing.argtypes = [vp, C.c_int]
        L.mi_outgate_last_launch_ms.argtypes = [vp, vp]
        L.mi_gate_plan_host.argtypes = [vp, C.c_int, vp, sz, C.c_int, vp, vp, vp, vp]
        L.mi_txsplit_create.argtypes = [C.POINTER(TxCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_txsplit_destroy.argtypes = [vp]
        L.mi_txsplit_destroy.restype = None
        L.mi_txsplit_set_rows.argtypes = [vp, vp]
        L.mi_txsplit_process_device.argtypes = [vp, vp, sz, vp, sz, C.c_int, vp, vp, vp, vp]
        L.mi_txsplit_download.argtypes = [vp, vp, vp, vp, vp]
        L.mi_txsplit_state_size.argtypes = [vp]
        L.mi_txsplit_state_size.restype = sz
        L.mi_txsplit_get_state.argtypes = [vp, vp, sz]
        L.mi_txsplit_set_state.argtypes = [vp, vp, sz]
        L.mi_txsplit_set_timing.argtypes = [vp, C.c_int]
        L.mi_txsplit_last_launch_ms.argtypes = [vp, vp]
        L.mi_tx_plan_host.argtypes = [C.POINTER(TxCfg), vp, C.c_int, vp, sz, C.c_int, vp, sz, vp, vp, sz, vp, vp]
        L.mi_tones_create.argtypes = [C.POINTER(TonesCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_tones_destroy.argtypes = [vp]
        L.mi_tones_destroy.restype = None
        L.mi_tones_set_rows.argtypes = [vp, vp]
        L.mi_tones_process_device.argtypes = [vp, vp, sz, vp, sz, C.c_int, vp, vp, vp, vp, vp]
        L.mi_tones_download.argtypes = [vp, vp, vp, vp, vp, vp]
        L.mi_tones_state_size.argtypes = [vp]
        L.mi_tones_state_size.restype = sz
        L.mi_tones_get_state.argtypes = [vp, vp, sz]
        L.mi_tones_set_state.argtypes = [vp, vp, sz]
        L.mi_tones_set_timing.argtypes = [vp, C.c_int]
        L.mi_tones_last_launch_ms.argtypes = [vp, vp]
        L.mi_tones_plan_host.argtypes = [C.POINTER(TonesCfg), vp, C.c_int, vp, sz, C.c_int, vp, sz, vp, vp, vp, sz, vp, vp]
        L.mi_tones_table.argtypes = [C.c_uint32, vp, vp, vp]
        L.mi_tones_vote_host.argtypes = [vp, sz, C.POINTER(TonesRule), C.POINTER(TonesVote)]
        L.mi_pcm_create.argtypes = [C.POINTER(PcmCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_pcm_destroy.argtypes = [vp]
        L.mi_pcm_destroy.restype = None
        L.mi_pcm_set_rows.argtypes = [vp, vp]
        L.mi_pcm_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp]
        L.mi_pcm_download.argtypes = [vp, vp, vp, vp]
        L.mi_pcm_state_size.argtypes = [vp]
        L.mi_pcm_state_size.restype = sz
        L.mi_pcm_get_state.argtypes = [vp, vp, sz]
        L.mi_pcm_set_state.argtypes = [vp, vp, sz]
        L.mi_pcm_set_timing.argtypes = [vp, C.c_int]
        L.mi_pcm_last_launch_ms.argtypes = [vp, vp]
        L.mi_pcm_block_bytes.argtypes = [C.POINTER(PcmCfg)]
        L.mi_pcm_block_bytes.restype = sz
        L.mi_pcm_taps.argtypes = [vp]
        L.mi_pcm_plan_host.argtypes = [C.POINTER(PcmCfg), vp, C.c_int, C.c_int, vp, sz, vp, sz, vp, vp]
        L.mi_pcm_wav_header.argtypes = [C.POINTER(PcmCfg), C.c_uint64, vp, sz, C.POINTER(sz)]
        L.mi_vband_default_row.argtypes = []
        L.mi_vband_default_row.restype = VbandRow
        L.mi_vband_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_vband_destroy.argtypes = [vp]
        L.mi_vband_destroy.restype = None
        L.mi_vband_set_rows.argtypes = [vp, vp, vp]
        L.mi_vband_process_device.argtypes = [vp, vp, sz, C.c_int, vp, sz, vp]
        L.mi_vband_state_size.argtypes = [vp]
        L.mi_vband_state_size.restype = sz
        L.mi_vband_get_state.argtypes = [vp, vp, sz]
        L.mi_vband_set_state.argtypes = [vp, vp, sz]
        L.mi_vband_set_timing.argtypes = [vp, C.c_int]
        L.mi_vband_last_launch_ms.argtypes = [vp, vp]
        L.mi_vband_taps.argtypes = [C.c_uint32, C.c_uint32, vp]
        L.mi_vband_plan_host.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, vp, vp, sz]
        L.mi_denoise_default_row.argtypes = []
        L.mi_denoise_default_row.restype = DenoiseRow
        L.mi_denoise_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_denoise_destroy.argtypes = [vp]
        L.mi_denoise_destroy.restype = None
        L.mi_denoise_set_rows.argtypes = [vp, vp, vp]
        L.mi_denoise_process_device.argtypes = [vp, vp, sz, C.c_int, vp, sz, vp]
        L.mi_denoise_state_size.argtypes = [vp]
        L.mi_denoise_state_size.restype = sz
        L.mi_denoise_get_state.argtypes = [vp, vp, sz]
        L.mi_denoise_set_state.argtypes = [vp, vp, sz]
        L.mi_denoise_set_timing.argtypes = [vp, C.c_int]
        L.mi_denoise_last_launch_ms.argtypes = [vp, vp]
        L.mi_denoise_window.argtypes = [vp]
        L.mi_denoise_plan_host.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, vp, vp, sz]
        L.mi_selcal_create.argtypes = [C.POINTER(SelcalCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_selcal_destroy.argtypes = [vp]
        L.mi_selcal_destroy.restype = None
        L.mi_selcal_set_rows.argtypes = [vp, vp]
        L.mi_selcal_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp, vp]
        L.mi_selcal_download.argtypes = [vp, vp, vp, vp, vp, vp]
        L.mi_selcal_state_size.argtypes = [vp]
        L.mi_selcal_state_size.restype = sz
        L.mi_selcal_get_state.argtypes = [vp, vp, sz]
        L.mi_selcal_set_state.argtypes = [vp, vp, sz]
        L.mi_selcal_set_timing.argtypes = [vp, C.c_int]
        L.mi_selcal_last_launch_ms.argtypes = [vp, vp]
        L.mi_selcal_plan_host.argtypes = [C.POINTER(SelcalCfg), vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, sz, vp, vp]
        L.mi_selcal_table.argtypes = [C.POINTER(SelcalCfg), C.POINTER(C.c_uint32), vp, vp, vp]
        L.mi_selcal_settings.argtypes = [C.POINTER(SelcalCfg), C.POINTER(SelcalCfg), C.POINTER(C.c_float)]
        L.mi_selcal_window.argtypes = [vp]
        L.mi_selcal_code_text.argtypes = [C.c_uint32, vp, vp]
        L.mi_acars_create.argtypes = [C.POINTER(AcarsCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_acars_destroy.argtypes = [vp]
        L.mi_acars_destroy.restype = None
        L.mi_acars_set_rows.argtypes = [vp, vp]
        L.mi_acars_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp, vp, vp]
        L.mi_acars_download.argtypes = [vp, vp, vp, vp, vp]
        L.mi_acars_state_size.argtypes = [vp]
        L.mi_acars_state_size.restype = sz
        L.mi_acars_get_state.argtypes = [vp, vp, sz]
        L.mi_acars_set_state.argtypes = [vp, vp, sz]
        L.mi_acars_set_timing.argtypes = [vp, C.c_int]
        L.mi_acars_last_launch_ms.argtypes = [vp, vp]
        L.mi_acars_plan_host.argtypes = [C.POINTER(AcarsCfg), vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, vp, sz, vp, vp]
        L.mi_acars_settings.argtypes = [C.POINTER(AcarsCfg), C.POINTER(AcarsCfg)]
        L.mi_acars_templates.argtypes = [vp, vp]
        L.mi_acars_crc.argtypes = [vp, sz]
        L.mi_acars_crc.restype = C.c_uint32
        L.mi_acars_frame_text.argtypes = [vp, C.POINTER(AcarsText)]
        L.mi_ax25_create.argtypes = [C.POINTER(Ax25Cfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_ax25_destroy.argtypes = [vp]
        L.mi_ax25_destroy.restype = None
        L.mi_ax25_set_rows.argtypes = [vp, vp]
        L.mi_ax25_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp, vp]
        L.mi_ax25_download.argtypes = [vp, vp, vp, vp, vp]
        L.mi_ax25_state_size.argtypes = [vp]
        L.mi_ax25_state_size.restype = sz
        L.mi_ax25_get_state.argtypes = [vp, vp, sz]
        L.mi_ax25_set_state.argtypes = [vp, vp, sz]
        L.mi_ax25_set_timing.argtypes = [vp, C.c_int]
        L.mi_ax25_last_launch_ms.argtypes = [vp, vp]
        L.mi_ax25_plan_host.argtypes = [C.POINTER(Ax25Cfg), vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, sz, vp, vp]
        L.mi_ax25_settings.argtypes = [C.POINTER(Ax25Cfg), C.POINTER(Ax25Cfg)]
        L.mi_ax25_templates.argtypes = [vp]
        L.mi_ax25_crc.argtypes = [vp, sz]
        L.mi_ax25_crc.restype = C.c_uint32
        L.mi_ax25_frame_text.argtypes = [vp, C.c_char_p, sz]
        L.mi_pocsag_create.argtypes = [C.POINTER(PocsagCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_pocsag_destroy.argtypes = [vp]
        L.mi_pocsag_destroy.restype = None
        L.mi_pocsag_set_rows.argtypes = [vp, vp]
        L.mi_pocsag_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp, vp, vp]
        L.mi_pocsag_download.argtypes = [vp, vp, vp, vp, vp]
        L.mi_pocsag_state_size.argtypes = [vp]
        L.mi_pocsag_state_size.restype = sz
        L.mi_pocsag_get_state.argtypes = [vp, vp, sz]
        L.mi_pocsag_set_state.argtypes = [vp, vp, sz]
        L.mi_pocsag_set_timing.argtypes = [vp, C.c_int]
        L.mi_pocsag_last_launch_ms.argtypes = [vp, vp]
        L.mi_pocsag_plan_host.argtypes = [C.POINTER(PocsagCfg), vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, vp, sz, vp, vp]
        L.mi_pocsag_settings.argtypes = [C.POINTER(PocsagCfg), C.POINTER(PocsagCfg)]
        L.mi_pocsag_geometry.argtypes = [C.c_uint32, vp, vp, vp]
        L.mi_pocsag_max_messages.argtypes = [C.c_uint32, C.c_uint64]
        L.mi_pocsag_max_messages.restype = C.c_uint32
        L.mi_pocsag_encode.argtypes = [C.c_uint32]
        L.mi_pocsag_encode.restype = C.c_uint32
        L.mi_pocsag_decode.argtypes = [C.c_uint32, C.c_uint32, vp, vp]
        L.mi_pocsag_message_text.argtypes = [vp, C.c_int, C.c_char_p, sz]
        L.mi_elt_create.argtypes = [C.POINTER(EltCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_elt_destroy.argtypes = [vp]
        L.mi_elt_destroy.restype = None
        L.mi_elt_set_rows.argtypes = [vp, vp]
        L.mi_elt_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp, vp]
        L.mi_elt_download.argtypes = [vp, vp, vp, vp, vp, vp]
        L.mi_elt_state_size.argtypes = [vp]
        L.mi_elt_state_size.restype = sz
        L.mi_elt_get_state.argtypes = [vp, vp, sz]
        L.mi_elt_set_state.argtypes = [vp, vp, sz]
        L.mi_elt_set_timing.argtypes = [vp, C.c_int]
        L.mi_elt_last_launch_ms.argtypes = [vp, vp]
        L.mi_elt_plan_host.argtypes = [C.POINTER(EltCfg), vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, sz, vp, vp]
        L.mi_elt_settings.argtypes = [C.POINTER(EltCfg), C.POINTER(EltCfg), C.POINTER(C.c_float)]
        L.mi_elt_window.argtypes = [vp]
        L.mi_elt_coeffs.argtypes = [vp]
        L.mi_elt_event_text.argtypes = [vp, vp]
        L.mi_same_create.argtypes = [C.POINTER(SameCfg), vp, C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_same_destroy.argtypes = [vp]
        L.mi_same_destroy.restype = None
        L.mi_same_set_rows.argtypes = [vp, vp]
        L.mi_same_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp, vp, vp]
        L.mi_same_download.argtypes = [vp, vp, vp, vp, vp]
        L.mi_same_state_size.argtypes = [vp]
        L.mi_same_state_size.restype = sz
        L.mi_same_get_state.argtypes = [vp, vp, sz]
        L.mi_same_set_state.argtypes = [vp, vp, sz]
        L.mi_same_set_timing.argtypes = [vp, C.c_int]
        L.mi_same_last_launch_ms.argtypes = [vp, vp]
        L.mi_same_plan_host.argtypes = [C.POINTER(SameCfg), vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, vp, sz, vp, vp]
        L.mi_same_settings.argtypes = [C.POINTER(SameCfg), C.POINTER(SameCfg)]
        L.mi_same_templates.argtypes = [vp]
        L.mi_same_message_text.argtypes = [vp, C.POINTER(SameText)]
        L.mi_limit_default_row.argtypes = []
        L.mi_limit_default_row.restype = LimitRow
        L.mi_limit_create.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_limit_destroy.argtypes = [vp]
        L.mi_limit_destroy.restype = None
        L.mi_limit_set_rows.argtypes = [vp, vp, vp]
        L.mi_limit_process_device.argtypes = [vp, vp, sz, C.c_int, vp, sz, vp]
        L.mi_limit_state_size.argtypes = [vp]
        L.mi_limit_state_size.restype = sz
        L.mi_limit_get_state.argtypes = [vp, vp, sz]
        L.mi_limit_set_state.argtypes = [vp, vp, sz]
        L.mi_limit_set_timing.argtypes = [vp, C.c_int]
        L.mi_limit_last_launch_ms.argtypes = [vp, vp]
        L.mi_limit_plan_host.argtypes = [vp, vp, C.c_int, C.c_int, vp, sz, vp, vp, sz]
        L.mi_limit_pregain_host.argtypes = [vp, sz, C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        L.mi_aspec_create.argtypes = [C.POINTER(AspecCfg), C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_aspec_destroy.argtypes = [vp]
        L.mi_aspec_destroy.restype = None
        L.mi_aspec_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mi_aspec_download.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.mi_aspec_set_timing.argtypes = [vp, C.c_int]
        L.mi_aspec_last_launch_ms.argtypes = [vp, vp]
        L.mi_aspec_window.argtypes = [vp]
        L.mi_aspec_band.argtypes = [C.POINTER(AspecCfg), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.mi_aspec_plan_host.argtypes = [C.POINTER(AspecCfg), C.c_int, C.c_int, vp, sz, vp, sz, vp, vp, vp, vp, vp]
        L.mi_aspec_notch_host.argtypes = [vp, C.c_uint32, vp, sz, C.POINTER(AspecCfg), C.POINTER(AspecRule), C.POINTER(AspecNotch)]
        L.mi_survey_create.argtypes = [C.POINTER(DeviceCfg), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_survey_destroy.argtypes = [vp]
        L.mi_survey_destroy.restype = None
        L.mi_survey_set_streams.argtypes = [vp, vp]
        L.mi_survey_bytes_needed.argtypes = [vp, C.c_int]
        L.mi_survey_bytes_needed.restype = sz
        L.mi_survey_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp, vp]
        L.mi_survey_set_timing.argtypes = [vp, C.c_int]
        L.mi_survey_last_launch_ms.argtypes = [vp, vp]
        L.mi_survey_bin_range.argtypes = [C.POINTER(DeviceCfg), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mi_occupancy_create.argtypes = [C.POINTER(DeviceCfg), C.POINTER(OccCfg), C.c_int, C.c_int, sz, C.c_int, C.POINTER(vp)]
        L.mi_occupancy_destroy.argtypes = [vp]
        L.mi_occupancy_destroy.restype = None
        L.mi_occupancy_set_streams.argtypes = [vp, vp]
        L.mi_occupancy_process_device.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
        L.mi_occupancy_download.argtypes = [vp, vp, vp, vp, vp, vp]
        L.mi_occupancy_set_timing.argtypes = [vp, C.c_int]
        L.mi_occupancy_last_launch_ms.argtypes = [vp, vp]
        L.mi_occupancy_plan_host.argtypes = [C.POINTER(DeviceCfg), C.POINTER(OccCfg), vp, C.c_int, vp, vp, C.c_int, vp, vp, sz, vp, vp]
        L.mi_probe_create.argtypes = [C.POINTER(DeviceCfg), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.mi_probe_destroy.argtypes = [vp]
        L.mi_probe_destroy.restype = None
        L.mi_probe_set_targets.argtypes = [vp, vp, C.c_int]
        L.mi_probe_bytes_needed.argtypes = [vp, C.c_int]
        L.mi_probe_bytes_needed.restype = sz
        L.mi_probe_process_device.argtypes = [vp, vp, sz, C.c_int, vp, vp]
        L.mi_probe_download.argtypes = [vp, vp, vp]
        L.mi_probe_set_timing.argtypes = [vp, C.c_int]
        L.mi_probe_last_launch_ms.argtypes = [vp, vp]
        L.mi_probe_targets_from_candidates.argtypes = [vp, sz, vp]
        L.mi_probe_features_host.argtypes = [C.POINTER(DeviceCfg), C.c_int, vp, C.c_int, vp, C.POINTER(ProbeFeatures)]
        L.mi_probe_classify_host.argtypes = [C.POINTER(ProbeFeatures), C.POINTER(ProbeRule), C.POINTER(C.c_int)]
        L.mi_plan_create.argtypes = [C.POINTER(DeviceCfg), C.POINTER(ChannelCfg), C.c_int, C.POINTER(vp)]
        L.mi_plan_destroy.argtypes = [vp]
        L.mi_plan_destroy.restype = None
        L.mi_plan_fft_size.argtypes = [vp]
        for f in (L.mi_plan_window, L.mi_plan_twiddles, L.mi_plan_levels):
            f.argtypes = [vp, vp]
        L.mi_plan_sincos_lut.argtypes = [vp, vp, vp]
        L.mi_plan_channel.argtypes = [vp, C.c_int, C.POINTER(ChannelDerived)]
        L.mi_plan_lane_fft.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int), vp, vp]
        L.mi_plan_ctcss_coeffs.argtypes = [vp, C.c_int, C.c_int, vp]
        L.mi_iqgen_host.argtypes = [C.POINTER(IqGenCfg), C.c_uint32, C.c_uint64, C.c_uint64, vp]
        L.mi_iqgen_device.argtypes = [C.POINTER(IqGenCfg), C.c_uint32, C.c_uint32, sz, C.c_uint64, C.c_uint64, vp, vp]
        _lib = L
    return _lib


def _check(rc):
    if rc != MI_OK:
        raise MiError(rc, lib().mi_last_error().decode())


def device_count():
    return lib().mi_device_count()


def device_cfg(sample_rate=2560000, centerfreq=120000000, fft_size_log=9, sfmt=SFMT_U8, fullscale=127.5, tau=-1, fm_quadri=0):
    return DeviceCfg(sample_rate, centerfreq, fft_size_log, sfmt, fullscale, tau, fm_quadri)


def channel_cfg(freq, modulation=MOD_AM, squelch_threshold_dbfs=0, squelch_snr_db=None, notch=0.0, notch_q=0.0, ctcss=0.0, bandwidth=0,
                ampfactor=1.0, tau=-1, afc=0, has_iq_outputs=0):
    return ChannelCfg(freq, modulation, squelch_threshold_dbfs, 0 if squelch_snr_db is None else 1,
                      -1.0 if squelch_snr_db is None else squelch_snr_db, notch, notch_q, ctcss, bandwidth, ampfactor, tau, afc,
                      has_iq_outputs)


def _chan_array(chans):
    return (ChannelCfg * len(chans))(*chans)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _flags(x):
    """truth values as 0 / 1 bytes"""
    return np.array([1 if v else 0 for v in x], np.uint8)


class _Handle:
    """A library handle in `_h` (None once closed), released by the function `_destroy` names."""
    _destroy = None
    _h = None

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TimedStage(_Handle):
    """The handle of a stage with per-launch timing: the calls `_prefix`_* over its `_launches` launches."""
    _prefix = None
    _launches = 0

    def _call(self, name, *args):
        _check(getattr(lib(), f"{self._prefix}_{name}")(self._h, *args))

    def set_timing(self, on=True):
        self._call("set_timing", 1 if on else 0)

    def last_launch_ms(self):
        """(diagnostic) ms of each launch of the last call made with set_timing(True): the gate's rank pass, scan and block copy;
        the splitter's walk, scan, block statistics and combine pass; the tone finder's walk, scan and bank; the PCM stage's encoder and tail copy; the audio spectrum stage's blocks and row means; the voice band stage's filter and tail copy; the limiter stage's limiter and tail copy; the noise reduction stage's floor, apply and tails; the SELCAL stage's bank, walk, scan, store and tails; the ACARS stage's bits, walk, scan, store and tails; the SAME stage's bits, walk, scan, store and tails; the ELT stage's bank, walk, scan, store and tails; the packet and the pager stage's bits, walk, scan, store and tails;
        the survey's windows and fold; the channel finder's bin records, run starts, scan and candidates; the probe's windows and reduction"""
        ms = (C.c_float * self._launches)()
        self._call("last_launch_ms", C.cast(ms, C.c_void_p))
        return tuple(ms)


class _PostStage(_TimedStage):
    """... with a state blob."""

    def state(self):
        """The state blob as bytes (*_get_state): the gate's carried flags, one per row; the splitter's rows * 32 bytes, whose
        fields .view(TX_STATE_DTYPE) names; the tone finder's rows * 520 bytes, .view(TONES_STATE_DTYPE); the PCM stage's rows * 248,
        .view(PCM_STATE_DTYPE); the voice band stage's rows * 2040, .view(VBAND_STATE_DTYPE); the limiter stage's rows * 4344, .view(LIMIT_STATE_DTYPE); the noise reduction stage's rows * 9196, .view(DENOISE_STATE_DTYPE); the SELCAL stage's rows * 4048,
        .view(SELCAL_STATE_DTYPE); the ACARS stage's rows * 496, .view(ACARS_STATE_DTYPE); the SAME stage's rows * 1160, .view(SAME_STATE_DTYPE); the ELT stage's rows * 776, .view(ELT_STATE_DTYPE); the packet stage's rows * 10544, .view(AX25_STATE_DTYPE); the pager stage's rows * 800, .view(POCSAG_STATE_DTYPE).  The audio spectrum stage has none."""
        n = getattr(lib(), f"{self._prefix}_state_size")(self._h)
        buf = np.zeros(n, np.uint8)
        self._call("get_state", _ptr(buf), n)
        return buf

    def set_state(self, buf):
        """The state blob back in (*_set_state): bytes as state() gave them, or an array of the stage's *_STATE_DTYPE."""
        buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        self._call("set_state", _ptr(buf), buf.size)


class Plan(_Handle):
    """Host-only derived parameters (no GPU needed)."""
    _destroy = "mi_plan_destroy"

    def __init__(self, dev, chans):
        self._h = C.c_void_p()
        self.nch = len(chans)
        _check(lib().mi_plan_create(C.byref(dev), _chan_array(chans), self.nch, C.byref(self._h)))
        self.fft_size = lib().mi_plan_fft_size(self._h)

    def _vec(self, fn, n):
        out = np.zeros(n, np.float32)
        _check(fn(self._h, _ptr(out)))
        return out

    def window(self):
        return self._vec(lib().mi_plan_window, self.fft_size)

    def twiddles(self):
        return self._vec(lib().mi_plan_twiddles, self.fft_size).reshape(-1, 2)

    def levels(self):
        return self._vec(lib().mi_plan_levels, 256)

    def sincos_lut(self):
        s, c = np.zeros(257, np.float32), np.zeros(257, np.float32)
        _check(lib().mi_plan_sincos_lut(self._h, _ptr(s), _ptr(c)))
        return s, c

    def channel(self, i):
        d = ChannelDerived()
        _check(lib().mi_plan_channel(self._h, i, C.byref(d)))
        return d

    def lane_fft(self):
        """The lane-resident stage 1 as the plan derives it: (enabled, need[6] residue masks of the in-lane stages, lanes per
        window, slots[nch] among the live classes mod 64, stage_tw[nch][log2n - 6][2] twiddles of the combining stages)."""
        nst = max(self.fft_size.bit_length() - 1 - 6, 0)
        enabled, lanes = C.c_int(0), C.c_int(0)
        need = (C.c_uint64 * 6)()
        slots = np.zeros(self.nch, np.int32)
        tw = np.zeros((self.nch, nst, 2), np.float32)
        _check(lib().mi_plan_lane_fft(self._h, C.byref(enabled), need, C.byref(lanes), _ptr(slots),
                                      _ptr(tw)))
        return bool(enabled.value), [int(x) for x in need], lanes.value, slots, tw

    def ctcss_coeffs(self, i, slow):
        d = self.channel(i)
        n = d.ctcss_slow_ndet if slow else d.ctcss_fast_ndet
        out = np.zeros(n, np.float32)
        _check(lib().mi_plan_ctcss_coeffs(self._h, i, 1 if slow else 0, _ptr(out)))
        return out


class Demod(_Handle):
    """nstreams x nch channels of demodulate() state resident on one GPU."""
    _destroy = "mi_demod_destroy"

    def __init__(self, dev, chans, nstreams=1, max_batches=1, gpu=0):
        self._h = C.c_void_p()
        self.nch, self.nstreams, self.max_batches = len(chans), nstreams, max_batches
        self.chans = list(chans)
        _check(lib().mi_demod_create(C.byref(dev), _chan_array(chans), self.nch, nstreams, max_batches, gpu, C.byref(self._h)))

    @property
    def hop_bytes(self):
        return lib().mi_demod_hop_bytes(self._h)

    def bytes_needed(self, nbatches):
        return lib().mi_demod_bytes_needed(self._h, nbatches)

    def bytes_consumed(self, nbatches):
        return lib().mi_demod_bytes_consumed(self._h, nbatches)

    def process(self, iq_streams, nbatches, want_iq=False, want_stats=True):
        """Host-buffer entry.  iq_streams: list of uint8 arrays, one per stream, each starting at the stream's
        current position.  Returns (waveout[ns][nch][nb*2000+100], axc[ns][nch][nb], iq_out or None, stats or None)."""
        assert len(iq_streams) == self.nstreams
        need = self.bytes_needed(nbatches)
        keep = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8) for a in iq_streams]  # (None: a stream that sits the call out)
        for a in keep:
            if a is not None and a.size < need:
                raise ValueError(f"stream shorter than bytes_needed ({a.size} < {need})")
        ptrs = (C.c_void_p * self.nstreams)(*[None if a is None else a.ctypes.data for a in keep])
        # the library completes whatever was submitted before it runs this call: those results are ready for wait()
        self._done = getattr(self, "_done", []) + getattr(self, "_tickets", [])
        self._tickets = []
        n = nbatches * WAVE_BATCH
        wo = np.zeros((self.nstreams, self.nch, n + AGC_EXTRA), np.float32)
        axc = np.zeros((self.nstreams, self.nch, nbatches), np.uint8)
        iqo = np.zeros((self.nstreams, self.nch, n, 2), np.float32) if want_iq else None
        stats = (ChannelStats * (self.nstreams * self.nch))() if want_stats else None
        _check(lib().mi_demod_process(self._h, ptrs, nbatches, _ptr(wo),
                                      None if iqo is None else _ptr(iqo), _ptr(axc),
                                      None if stats is None else C.cast(stats, C.c_void_p)))
        return wo, axc, iqo, stats

    def submit(self, iq_streams, nbatches, want_iq=False, want_stats=True, waveout=None):
        """mi_demod_submit: starts a call and returns a ticket; wait() completes the oldest ticket and returns its results
        like process().  The numpy arrays of a ticket stay referenced until it has been waited for."""
        assert len(iq_streams) == self.nstreams
        need = self.bytes_needed(nbatches)
        keep = [a if a is None or isinstance(a, PinnedBuffer) else np.ascontiguousarray(a, dtype=np.uint8) for a in iq_streams]
        addr = [None if a is None else (a.ptr if isinstance(a, PinnedBuffer) else a.ctypes.data) for a in keep]
        ptrs = (C.c_void_p * self.nstreams)(*addr)
        n = nbatches * WAVE_BATCH
        # waveout: an optional caller-owned float32 array [nstreams][nch][n + AGC_EXTRA] (e.g. a view of a PinnedBuffer)
        wo = waveout if waveout is not None else np.empty((self.nstreams, self.nch, n + AGC_EXTRA), np.float32)
        assert wo.dtype == np.float32 and wo.size == self.nstreams * self.nch * (n + AGC_EXTRA) and wo.flags["C_CONTIGUOUS"]
        axc = np.zeros((self.nstreams, self.nch, nbatches), np.uint8)
        iqo = np.zeros((self.nstreams, self.nch, n, 2), np.float32) if want_iq else None
        stats = (ChannelStats * (self.nstreams * self.nch))() if want_stats else None
        _check(lib().mi_demod_submit(self._h, ptrs, nbatches, _ptr(wo),
                                     None if iqo is None else _ptr(iqo), _ptr(axc),
                                     None if stats is None else C.cast(stats, C.c_void_p)))
        if not hasattr(self, "_tickets"):
            self._tickets = []
        self._tickets.append((keep, ptrs, wo, axc, iqo, stats))
        while len(self._tickets) > MAX_IN_FLIGHT:  # a further submit completed the oldest call inside the library
            self._done = getattr(self, "_done", []) + [self._tickets.pop(0)]

    def wait(self):
        """Results (waveout, axc, iq_out, stats) of the oldest submitted call."""
        done = getattr(self, "_done", [])
        if done:
            t = done.pop(0)
            return t[2], t[3], t[4], t[5]
        _check(lib().mi_demod_wait(self._h))
        t = self._tickets.pop(0)
        return t[2], t[3], t[4], t[5]

    def process_device(self, d_iq_ptr, stream_stride, nbatches, d_waveout_ptr, d_axc_ptr, d_iq_out_ptr=None, hip_stream=None):
        """Device-resident entry: raw device pointers (ints), asynchronous on hip_stream."""
        _check(lib().mi_demod_process_device(self._h, d_iq_ptr, stream_stride, nbatches, d_waveout_ptr, d_iq_out_ptr, d_axc_ptr, hip_stream))

    def set_active_streams(self, active=None):
        """mi_demod_set_active_streams: `active` = one truth value per stream, or None for all.  Streams that are not active sit the
        following calls out: their IQ is not read (pass None for them), their output regions and their state are left untouched."""
        # the library completes whatever was submitted before it changes the mask: those results are ready for wait()
        self._done = getattr(self, "_done", []) + getattr(self, "_tickets", [])
        self._tickets = []
        if active is None:
            _check(lib().mi_demod_set_active_streams(self._h, None))
            return
        assert len(active) == self.nstreams
        m = _flags(active)
        _check(lib().mi_demod_set_active_streams(self._h, _ptr(m)))

    def get_active_streams(self):
        m = np.zeros(self.nstreams, np.uint8)
        _check(lib().mi_demod_get_active_streams(self._h, _ptr(m)))
        return [bool(x) for x in m]

    def stats(self):
        st = (ChannelStats * (self.nstreams * self.nch))()
        _check(lib().mi_demod_get_stats(self._h, C.cast(st, C.c_void_p)))
        return st

    def get_state(self):
        n = lib().mi_demod_state_size(self._h)
        buf = np.zeros(n, np.uint8)
        _check(lib().mi_demod_get_state(self._h, _ptr(buf), n))
        return buf

    def set_state(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        _check(lib().mi_demod_set_state(self._h, _ptr(buf), buf.size))

    def last_path(self):
        """(1 if the last call ran the time-parallel stage 2 else 0, rows left unverified -- always 0)."""
        a, b = C.c_int(0), C.c_int(0)
        _check(lib().mi_demod_last_path(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def process_planes(self, mag, nbatches, cplx=None, want_iq=False):
        """mi_demod_process_planes (test entry): stage 2 over caller-supplied planes.  mag: [rows][count] float32; cplx:
        [iq rows][count][2] or None.  Returns (waveout [nstreams][nch][n + AGC_EXTRA], axc, iq_out or None, stats)."""
        n = nbatches * WAVE_BATCH
        mag = np.ascontiguousarray(mag, dtype=np.float32)
        wo = np.zeros((self.nstreams, self.nch, n + AGC_EXTRA), np.float32)
        axc = np.zeros((self.nstreams, self.nch, nbatches), np.uint8)
        iqo = np.zeros((self.nstreams, self.nch, n, 2), np.float32) if want_iq else None
        stats = (ChannelStats * (self.nstreams * self.nch))()
        zc = None if cplx is None else np.ascontiguousarray(cplx, dtype=np.float32)
        f = lib().mi_demod_process_planes
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(f(self._h, _ptr(mag), None if zc is None else _ptr(zc), nbatches,
                 _ptr(wo), None if iqo is None else _ptr(iqo), _ptr(axc),
                 C.cast(stats, C.c_void_p)))
        return wo, axc, iqo, list(stats)

    def prepare(self, host_slots=1):
        """mi_demod_prepare: stage-1 kernel of the plan + the staging of `host_slots` host-buffer calls, before the first batch."""
        _check(lib().mi_demod_prepare(self._h, host_slots))

    def pre_wave_timeouts(self):
        n = C.c_uint(0)
        f = lib().mi_demod_pre_wave_timeouts
        f.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        _check(f(self._h, C.byref(n)))
        return n.value

    def last_stage1(self):
        """MI_STAGE1_* of the last call: 0 / 1 exchange kernels (full / pruned), 2 / 3 lane-resident (full graph / plan-compiled)."""
        k = C.c_int(-1)
        _check(lib().mi_demod_last_stage1(self._h, C.byref(k)))
        return k.value

    def tp_debug(self, row):
        """(core[nseg+1][4], diag[4]) of the last time-parallel call for one row."""
        nseg = C.c_int(0)
        _check(lib().mi_demod_tp_debug(self._h, row, None, 0, None, C.byref(nseg)))
        core = np.zeros((nseg.value + 1, 4), np.float32)
        diag = np.zeros(8, np.int32)
        _check(lib().mi_demod_tp_debug(self._h, row, _ptr(core), nseg.value + 1, _ptr(diag),
                                       C.byref(nseg)))
        return core, diag

    def read_planes(self, stream, ch, first, count, want_iq=False):
        mag = np.zeros(count, np.float32)
        iq = np.zeros((count, 2), np.float32) if want_iq else None
        _check(lib().mi_demod_read_planes(self._h, stream, ch, first, count, _ptr(mag),
                                          None if iq is None else _ptr(iq)))
        return mag, iq

    def set_option(self, option, value):
        _check(lib().mi_demod_set_option(self._h, option, value))

    def kernel_times(self, age=0):
        """[(kernel name, total ms, launches)] of the last call (age 0) or of the call `age` calls before it, from HIP events
        on the launch streams."""
        out = []
        i = 0
        while True:
            name, ms, n = C.c_char_p(), C.c_float(0), C.c_int(0)
            if lib().mi_demod_kernel_time_prev(self._h, age, i, C.byref(name), C.byref(ms), C.byref(n)) != MI_OK:
                break
            out.append((name.value.decode(), ms.value, n.value))
            i += 1
        return out

    def event_ms(self, ref_age, age, chunk, event):
        """(diagnostic) ms from the core chain start of the call `ref_age` back to an event of the call `age` back, or None"""
        ms = C.c_float(0)
        if lib().mi_demod_event_ms(self._h, ref_age, age, chunk, event, C.byref(ms)) != MI_OK:
            return None
        return ms.value

    def last_kernel_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        _check(lib().mi_demod_last_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


def iqgen_cfg(sample_rate=2560000, seed=0xA1B2C3D4, noise_q8_mul=111, gate_samples=None, carriers=()):
    cfg = IqGenCfg()
    cfg.sample_rate = sample_rate
    cfg.seed = seed
    cfg.noise_q8_mul = noise_q8_mul
    cfg.gate_samples = sample_rate if gate_samples is None else gate_samples
    cfg.ncarriers = len(carriers)
    for i, (off, kind, amp_q8, gate_phase) in enumerate(carriers):
        cfg.carriers[i] = IqGenCarrier(off, kind, amp_q8, gate_phase)
    return cfg


def iqgen_host(cfg, stream_id, first, count):
    out = np.zeros(2 * count, np.uint8)
    _check(lib().mi_iqgen_host(C.byref(cfg), stream_id, first, count, _ptr(out)))
    return out


def iqgen_device(cfg, first_stream_id, nstreams, stream_stride, first, count, d_out_ptr, hip_stream=None):
    _check(lib().mi_iqgen_device(C.byref(cfg), first_stream_id, nstreams, stream_stride, first, count, d_out_ptr, hip_stream))


def set_cache_dir(path):
    """mi_set_cache_dir: where compiled stage-1 kernels are kept between process starts (None / "" = nowhere)."""
    _check(lib().mi_set_cache_dir(None if path is None else os.fsencode(path)))


def jit_counts():
    """(kernels compiled by this process, kernels loaded from the cache directory)"""
    a, b = C.c_int(0), C.c_int(0)
    _check(lib().mi_jit_counts(C.byref(a), C.byref(b)))
    return a.value, b.value


class Gather(_Handle):
    """mi_gather_*: audio + flags of every rank to rank 0 over RCCL (the C-ABI twin of shard.AudioGather)."""
    _destroy = "mi_gather_destroy"

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        _check(lib().mi_gather_unique_id(C.byref(buf)))
        return bytes(buf)

    @staticmethod
    def loopback_id(job):
        """mi_gather_loopback_id (test transport): ranks of job `job` are threads of this process."""
        buf = (C.c_char * 128)()
        f = lib().mi_gather_loopback_id
        f.argtypes = [C.c_void_p, C.c_uint64]
        _check(f(C.byref(buf), job))
        return bytes(buf)

    def __init__(self, uid, rank, world, gpu, streams_per_rank, nch, max_batches):
        self._h = C.c_void_p()
        idbuf = (C.c_char * 128).from_buffer_copy(uid) if uid is not None else None
        arr = (C.c_int * world)(*streams_per_rank)
        _check(lib().mi_gather_create(None if idbuf is None else C.byref(idbuf), rank, world, gpu, arr, nch, max_batches, C.byref(self._h)))

    def audio(self, d_waveout, d_axc, nbatches, d_all_waveout=None, d_all_axc=None, open_only=False, hip_stream=None):
        _check(lib().mi_gather_audio(self._h, d_waveout, d_axc, nbatches, 1 if open_only else 0, d_all_waveout, d_all_axc, hip_stream))

    def stream_wait(self, hip_stream=None):
        _check(lib().mi_gather_stream_wait(self._h, hip_stream))

    def sync(self):
        _check(lib().mi_gather_sync(self._h))


class PinnedBuffer:
    """Page-locked host memory from mi_host_alloc, viewed as a uint8 numpy array (.array); .ptr is its address."""

    def __init__(self, nbytes, _root=None, _ptr=None):
        self._root = _root
        if _root is None:
            self._mem = lib().mi_host_alloc(nbytes)
            if not self._mem:
                raise MemoryError("mi_host_alloc failed")
            self.ptr = self._mem
        else:
            self._mem = None
            self.ptr = _ptr
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array((C.c_ubyte * nbytes).from_address(self.ptr))

    def view(self, offset):
        """The same memory from `offset` on (a stream position inside a pinned capture)."""
        return PinnedBuffer(self.nbytes - offset, self._root or self, self.ptr + offset)

    def free(self):
        if self._mem:
            lib().mi_host_free(self._mem)
            self._mem = None


class Mixer(_Handle):
    """One mixer_t (src/mixer.cpp) over device-resident audio: inputs = [(row, ampfactor, balance), ...]."""
    _destroy = "mi_mixer_destroy"

    def __init__(self, inputs, gpu=0):
        arr = (MixInput * len(inputs))(*[MixInput(int(r), float(a), float(b)) for r, a, b in inputs])
        self._h = C.c_void_p()
        _check(lib().mi_mixer_create(arr, len(inputs), gpu, C.byref(self._h)))
        self.stereo = bool(lib().mi_mixer_is_stereo(self._h))

    def process_device(self, d_waveout, row_stride, d_axc, axc_stride, nbatches, d_left, d_right, d_axc_out, hip_stream=None):
        _check(lib().mi_mixer_process_device(self._h, d_waveout, row_stride, d_axc, axc_stride, nbatches, d_left, d_right, d_axc_out, hip_stream))


class OutputGate(_PostStage):
    """mi_outgate: the (row, batch) blocks the reference's outputs consume, packed on the device.  row_rule: one GATE_* per row
    (row = stream * nch + channel); row_has_iq: truth value per row or None; max_blocks: capacity of the destination buffers in
    blocks, 0 = rows * max_batches."""
    _destroy, _prefix, _launches = "mi_outgate_destroy", "mi_outgate", 3

    def __init__(self, row_rule, row_has_iq=None, max_batches=1, max_blocks=0, gpu=0):
        rule = np.ascontiguousarray(row_rule, dtype=np.uint8)
        self.rows, self.max_batches = rule.size, max_batches
        self.max_blocks = min(max_blocks, self.rows * max_batches) if max_blocks else self.rows * max_batches
        has_iq = None if row_has_iq is None else _flags(row_has_iq)
        assert has_iq is None or has_iq.size == self.rows
        self._h = C.c_void_p()
        _check(lib().mi_outgate_create(_ptr(rule), None if has_iq is None else _ptr(has_iq),
                                       self.rows, max_batches, max_blocks, gpu, C.byref(self._h)))

    def set_rules(self, row_rule):
        rule = np.ascontiguousarray(row_rule, dtype=np.uint8)
        assert rule.size == self.rows
        _check(lib().mi_outgate_set_rules(self._h, _ptr(rule)))

    def process_device(self, d_waveout, row_stride, d_axc, axc_stride, nbatches, d_blocks, d_index, d_row_first, d_count, d_iq_out=None,
                       iq_row_stride=0, d_iq_blocks=None, hip_stream=None):
        """Raw device pointers (ints), strides in floats (audio, raw I/Q) and bytes (flags); asynchronous on hip_stream."""
        _check(lib().mi_outgate_process_device(self._h, d_waveout, row_stride, d_iq_out, iq_row_stride, d_axc, axc_stride, nbatches, d_blocks,
                                               d_iq_blocks, d_index, d_row_first, d_count, hip_stream))

    def download(self, hip_stream=None, want_iq=False):
        """Results of the last process_device (enqueued on hip_stream): (blocks [k][WAVE_BATCH], iq_blocks [k][WAVE_BATCH][2] or None,
        index [k][2] = (row, batch), row_first [rows + 1], count [2]) with k = count[1], the number of blocks stored."""
        blocks = np.empty((self.max_blocks, WAVE_BATCH), np.float32)
        iq = np.empty((self.max_blocks, WAVE_BATCH, 2), np.float32) if want_iq else None
        index = np.empty((self.max_blocks, 2), np.uint32)
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_outgate_download(self._h, hip_stream, _ptr(blocks), None if iq is None else _ptr(iq),
                                         _ptr(index), _ptr(row_first), _ptr(count)))
        k = int(count[1])
        return blocks[:k], None if iq is None else iq[:k], index[:k], row_first, count

    def set_state(self, buf):  # (its own: truth values, converted to bytes and not viewed as them)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._call("set_state", _ptr(buf), buf.size)


def gate_plan_host(row_rule, axc, carried=None):
    """mi_gate_plan_host: the gate's index from flags on the host, no GPU.  axc: uint8 [rows][nbatches]; carried: uint8 [rows] or
    None (all false).  Returns (index [k][2] = (row, batch), row_first [rows + 1], count [2], carried after the call)."""
    rule = np.ascontiguousarray(row_rule, dtype=np.uint8)
    axc = np.ascontiguousarray(axc, dtype=np.uint8)
    assert axc.ndim == 2 and axc.shape[0] == rule.size
    rows, nb = axc.shape
    carried = np.zeros(rows, np.uint8) if carried is None else np.array(carried, dtype=np.uint8)
    assert carried.size == rows
    index = np.empty((rows * nb, 2), np.uint32)
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_gate_plan_host(_ptr(rule), rows, _ptr(axc), nb, nb, _ptr(carried),
                                   _ptr(index), _ptr(row_first), _ptr(count)))
    return index[:int(count[0])], row_first, count, carried


def _tx_cfg(cfg):
    """None, a TxCfg or (min_batches, idle_batches, max_batches) -> TxCfg"""
    if cfg is None:
        return TxCfg(0, 0, 0)
    return cfg if isinstance(cfg, TxCfg) else TxCfg(*[int(x) for x in cfg])


class TxSplit(_PostStage):
    """mi_txsplit: one recording per transmission in signal time (split_on_transmission, src/output.cpp:353-376) on the device.
    row_enabled: truth value per row (row = stream * nch + channel); cfg: (min, idle, max) in batches, 0 = the reference's 8 / 4 /
    28800; max_records: capacity of the record buffer, 0 = rows * (max_batches + 1)."""
    _destroy, _prefix, _launches = "mi_txsplit_destroy", "mi_txsplit", 4

    def __init__(self, row_enabled, max_batches=1, cfg=None, max_records=0, gpu=0):
        en = _flags(row_enabled)
        self.rows, self.max_batches = en.size, max_batches
        slots = self.rows * (max_batches + 1)
        self.max_records = min(max_records, slots) if max_records else slots
        self._h = C.c_void_p()
        _check(lib().mi_txsplit_create(C.byref(_tx_cfg(cfg)), _ptr(en), self.rows, max_batches, max_records, gpu, C.byref(self._h)))

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_txsplit_set_rows(self._h, _ptr(en)))

    def process_device(self, d_waveout, row_stride, d_axc, axc_stride, nbatches, d_records, d_row_first_record, d_count, hip_stream=None):
        """Raw device pointers (ints; d_waveout may be None), strides in floats (audio) and bytes (flags); asynchronous on hip_stream."""
        _check(lib().mi_txsplit_process_device(self._h, d_waveout, row_stride, d_axc, axc_stride, nbatches, d_records, d_row_first_record, d_count,
                                               hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (records [k] of TX_RECORD_DTYPE, row_first_record [rows + 1],
        count [2]) with k = count[1], the number of records stored."""
        records = np.zeros(self.max_records, TX_RECORD_DTYPE)
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_txsplit_download(self._h, hip_stream, _ptr(records), _ptr(row_first),
                                         _ptr(count)))
        return records[:int(count[1])], row_first, count


def tx_plan_host(row_enabled, axc, state=None, waveout=None, cfg=None, max_records=0, nbatches=None):
    """mi_tx_plan_host: the splitter's records from flags (and audio) on the host, no GPU.  axc: uint8 [rows][axc_stride]; waveout:
    float32 [rows][row_stride] or None; state: the blob (rows * 32 bytes) or None (a fresh one); nbatches: batches of the call, default
    axc's width; max_records: 0 = rows * (nbatches + 1).  Returns (records [count[1]], row_first_record [rows + 1], count [2], state
    after the call)."""
    en = _flags(row_enabled)
    axc = np.ascontiguousarray(axc, dtype=np.uint8)
    assert axc.ndim == 2 and axc.shape[0] == en.size
    rows, axc_stride = axc.shape
    nb = axc_stride if nbatches is None else nbatches
    state = np.zeros(rows * TX_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * TX_STATE_DTYPE.itemsize
    row_stride = 0
    if waveout is not None:
        waveout = np.ascontiguousarray(waveout, dtype=np.float32)
        assert waveout.ndim == 2 and waveout.shape[0] == rows
        row_stride = waveout.shape[1]
    cap = max_records or rows * (nb + 1)
    records = np.zeros(cap, TX_RECORD_DTYPE)
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_tx_plan_host(C.byref(_tx_cfg(cfg)), _ptr(en), rows, _ptr(axc), axc_stride, nb,
                                 None if waveout is None else _ptr(waveout), row_stride, _ptr(state),
                                 _ptr(records), cap, _ptr(row_first), _ptr(count)))
    return records[:int(count[1])], row_first, count, state


def _tones_cfg(window):
    """None or 0 (the default 6400), a window in samples or a TonesCfg -> TonesCfg"""
    return window if isinstance(window, TonesCfg) else TonesCfg(int(window or 0))


def tones_max_windows(window, nbatches):
    """the most windows one row completes in a call of nbatches batches"""
    w = window or 6400
    return (w - 1 + WAVE_BATCH * nbatches) // w


class Tones(_PostStage):
    """mi_tones: the CTCSS tone finder -- the reference's 51 standard tones (src/ctcss.cpp:101-103), one Goertzel detector each, over
    every window of `window` samples (0 = 6400, 800 .. 64000) of the rows' audio; a MI_NO_SIGNAL batch resets a row's window.
    row_enabled: truth value per row (row = stream * nch + channel); max_records: capacity of the record buffer, 0 = rows * the most
    windows a row completes in max_batches batches.  state() gives rows * 520 bytes, whose fields .view(TONES_STATE_DTYPE) names."""
    _destroy, _prefix, _launches = "mi_tones_destroy", "mi_tones", 3

    def __init__(self, row_enabled, max_batches=1, window=0, max_records=0, gpu=0):
        en = _flags(row_enabled)
        self.rows, self.max_batches, self.window = en.size, max_batches, _tones_cfg(window).window_samples or 6400
        most = self.rows * tones_max_windows(self.window, max_batches)
        self.max_records = min(max_records, most) if max_records else most
        self._h = C.c_void_p()
        _check(lib().mi_tones_create(C.byref(_tones_cfg(window)), _ptr(en), self.rows, max_batches, max_records, gpu, C.byref(self._h)))

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_tones_set_rows(self._h, _ptr(en)))

    def process_device(self, d_waveout, row_stride, d_axc, axc_stride, nbatches, d_records, d_row_first_record, d_count, d_powers=None,
                       hip_stream=None):
        """Raw device pointers (ints; d_powers may be None), strides in floats (audio) and bytes (flags); asynchronous on hip_stream."""
        self._with_powers = d_powers is not None
        _check(lib().mi_tones_process_device(self._h, d_waveout, row_stride, d_axc, axc_stride, nbatches, d_records, d_powers, d_row_first_record,
                                             d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (records [k] of TONE_RECORD_DTYPE, powers [k][64] or None where
        the call stored none, row_first_record [rows + 1], count [2]) with k = count[1], the number of records stored."""
        records = np.zeros(self.max_records, TONE_RECORD_DTYPE)
        powers = np.zeros((self.max_records, TONES_LANES), np.float32) if getattr(self, "_with_powers", False) else None
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_tones_download(self._h, hip_stream, _ptr(records), None if powers is None else _ptr(powers), _ptr(row_first), _ptr(count)))
        k = int(count[1])
        return records[:k], None if powers is None else powers[:k], row_first, count


def tones_plan_host(row_enabled, axc, waveout, state=None, window=0, max_records=0, nbatches=None, want_powers=True):
    """mi_tones_plan_host: the tone finder's records (and powers) from flags and audio on the host, no GPU.  axc: uint8 [rows][axc_stride];
    waveout: float32 [rows][row_stride]; state: the blob (rows * 520 bytes) or None (a fresh one); nbatches: batches of the call, default
    axc's width; max_records: 0 = every record of the call.  Returns (records [count[1]], powers [count[1]][64] or None,
    row_first_record [rows + 1], count [2], state after the call)."""
    en = _flags(row_enabled)
    axc = np.ascontiguousarray(axc, dtype=np.uint8)
    waveout = np.ascontiguousarray(waveout, dtype=np.float32)
    assert axc.ndim == 2 and axc.shape[0] == en.size and waveout.ndim == 2 and waveout.shape[0] == en.size
    rows, axc_stride = axc.shape
    nb = axc_stride if nbatches is None else nbatches
    cfg = _tones_cfg(window)
    state = np.zeros(rows * TONES_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * TONES_STATE_DTYPE.itemsize
    cap = max_records or max(1, rows * tones_max_windows(cfg.window_samples, nb))
    records = np.zeros(cap, TONE_RECORD_DTYPE)
    powers = np.zeros((cap, TONES_LANES), np.float32) if want_powers else None
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_tones_plan_host(C.byref(cfg), _ptr(en), rows, _ptr(axc), axc_stride, nb, _ptr(waveout), waveout.shape[1], _ptr(state),
                                    _ptr(records), None if powers is None else _ptr(powers), cap, _ptr(row_first), _ptr(count)))
    k = int(count[1])
    return records[:k], None if powers is None else powers[:k], row_first, count, state


def _pcm_cfg(rate=0, fmt=0):
    """a rate (0 = 8000) and a format (0 = PCM_S16), or a PcmCfg -> PcmCfg"""
    return rate if isinstance(rate, PcmCfg) else PcmCfg(int(rate or 0), int(fmt or 0))


def pcm_block_bytes(rate=0, fmt=0):
    """mi_pcm_block_bytes: bytes of one encoded block -- 2000 / 4000 as PCM_S16, 640 / 1280 as PCM_IMA4 at 8000 / 16000"""
    n = lib().mi_pcm_block_bytes(C.byref(_pcm_cfg(rate, fmt)))
    if not n:
        raise MiError(MI_ERR_INVALID, lib().mi_last_error().decode())
    return n


class Pcm(_PostStage):
    """mi_pcm: the blocks the output gate lets travel as int16 or WAV-container IMA ADPCM at 8000 (through the 63-tap decimating
    filter) or 16000 samples a second, encoded on the device from the gate's index and counts where it left them.  row_enabled: truth
    value per row (a disabled row's carried samples stay); max_blocks: capacity of the destination in blocks, 0 = rows * max_batches.
    state() gives rows * 248 bytes, .view(PCM_STATE_DTYPE): the 62 samples a row carries into its next call."""
    _destroy, _prefix, _launches = "mi_pcm_destroy", "mi_pcm", 2

    def __init__(self, row_enabled, max_batches=1, rate=0, fmt=0, max_blocks=0, gpu=0):
        en = _flags(row_enabled)
        cfg = _pcm_cfg(rate, fmt)
        self.rows, self.max_batches, self.block_bytes = en.size, max_batches, pcm_block_bytes(cfg)
        self.max_blocks = min(max_blocks, self.rows * max_batches) if max_blocks else self.rows * max_batches
        self._h = C.c_void_p()
        _check(lib().mi_pcm_create(C.byref(cfg), _ptr(en), self.rows, max_batches, max_blocks, gpu, C.byref(self._h)))

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_pcm_set_rows(self._h, _ptr(en)))

    def process_device(self, d_waveout, row_stride, nbatches, d_index, d_count, d_out, hip_stream=None):
        """Raw device pointers (ints), the stride in floats; d_index and d_count as OutputGate.process_device left them; asynchronous
        on hip_stream."""
        _check(lib().mi_pcm_process_device(self._h, d_waveout, row_stride, nbatches, d_index, d_count, d_out, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (blocks [k][block_bytes] uint8, count [2]) with k = count[1],
        the number of blocks stored; count[0] is the gate's number of travelling blocks."""
        blocks = np.empty((self.max_blocks, self.block_bytes), np.uint8)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_pcm_download(self._h, hip_stream, _ptr(blocks), _ptr(count)))
        return blocks[:int(count[1])], count


def pcm_plan_host(row_enabled, waveout, index, state=None, rate=0, fmt=0, nbatches=None):
    """mi_pcm_plan_host: the PCM stage's blocks from audio and an index on the host, no GPU.  waveout: float32 [rows][row_stride];
    index: [k][2] = (row, batch), as gate_plan_host gives it; state: the blob (rows * 248 bytes) or None (a fresh one); nbatches:
    batches of the call, default row_stride // WAVE_BATCH.  Returns (blocks [k][block_bytes] uint8, state after the call)."""
    en = _flags(row_enabled)
    waveout = np.ascontiguousarray(waveout, dtype=np.float32)
    assert waveout.ndim == 2 and waveout.shape[0] == en.size
    rows, row_stride = waveout.shape
    nb = row_stride // WAVE_BATCH if nbatches is None else nbatches
    index = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1, 2)
    cfg = _pcm_cfg(rate, fmt)
    state = np.zeros(rows * PCM_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * PCM_STATE_DTYPE.itemsize
    blocks = np.zeros((len(index), pcm_block_bytes(cfg)), np.uint8)
    _check(lib().mi_pcm_plan_host(C.byref(cfg), _ptr(en), rows, nb, _ptr(waveout), row_stride, _ptr(index) if len(index) else None, len(index),
                                  _ptr(state), _ptr(blocks) if len(index) else None))
    return blocks, state


def pcm_taps():
    """mi_pcm_taps: the 63 float32 taps of the 2:1 decimating filter"""
    h = np.zeros(PCM_TAPS, np.float32)
    _check(lib().mi_pcm_taps(_ptr(h)))
    return h


def pcm_wav_header(nblocks, rate=0, fmt=0):
    """mi_pcm_wav_header: the bytes that, in front of `nblocks` encoded blocks, make a complete WAV file (44 as PCM_S16, 60 as PCM_IMA4)"""
    buf = np.zeros(64, np.uint8)
    n = C.c_size_t(0)
    _check(lib().mi_pcm_wav_header(C.byref(_pcm_cfg(rate, fmt)), int(nblocks), _ptr(buf), buf.size, C.byref(n)))
    return buf[:n.value].tobytes()


def _row_settings(rows_cfg, rows, dtype, scalar, default):
    """None (default() everywhere), one pair of `scalar`s for every row, or a pair per row -> [rows] of `dtype`"""
    if rows_cfg is None:
        rows_cfg = default()
    a = np.asarray(rows_cfg)
    if a.dtype != dtype:
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(rows_cfg, scalar).reshape(-1, 2), (rows, 2))).view(dtype).reshape(-1)
    a = np.ascontiguousarray(a)
    assert a.shape == (rows,)
    return a


class _PlaneStage(_PostStage):
    """A post-stage that reads a plane [rows][row_stride] and writes one of the same layout under per-row settings (Vband, Limit, Denoise):
    `_rows_of`(rows_cfg, rows) gives the settings as the library takes them.  A subclass adds process_device under its own argument names."""
    _launches = 2
    _rows_of = None

    def __init__(self, row_enabled, rows_cfg=None, max_batches=1, gpu=0):
        en = _flags(row_enabled)
        self.rows, self.max_batches = en.size, max_batches
        cfg = type(self)._rows_of(rows_cfg, self.rows)
        self._h = C.c_void_p()
        _check(getattr(lib(), f"{self._prefix}_create")(_ptr(cfg), _ptr(en), self.rows, max_batches, gpu, C.byref(self._h)))

    def set_rows(self, row_enabled=None, rows_cfg=None):
        """other rows and / or other settings from the next call on (None = keep); the carried samples stay (and, in the limiter,
        count under the new pregain)"""
        en = None if row_enabled is None else _flags(row_enabled)
        cfg = None if rows_cfg is None else type(self)._rows_of(rows_cfg, self.rows)
        assert en is None or en.size == self.rows
        self._call("set_rows", None if cfg is None else _ptr(cfg), None if en is None else _ptr(en))


def _plane_plan_host(fn, rows_of, state_dtype, row_enabled, plane, rows_cfg, state, nbatches, out):
    """the host twin `fn` of a _PlaneStage: (out, state after the call)"""
    en = _flags(row_enabled)
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    assert plane.ndim == 2 and plane.shape[0] == en.size
    rows, row_stride = plane.shape
    nb = row_stride // WAVE_BATCH if nbatches is None else nbatches
    cfg = rows_of(rows_cfg, rows)
    state = np.zeros(rows * state_dtype.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * state_dtype.itemsize
    out = np.zeros((rows, nb * WAVE_BATCH), np.float32) if out is None else out
    assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == rows and out.flags.c_contiguous
    _check(fn(_ptr(cfg), _ptr(en), rows, nb, _ptr(plane), row_stride, _ptr(state), _ptr(out), out.shape[1]))
    return out, state


def vband_default_row():
    """mi_vband_default_row: (100, 2500), the reference's highpass / lowpass defaults"""
    r = lib().mi_vband_default_row()
    return r.hp_hz, r.lp_hz


def _vband_rows(rows_cfg, rows):
    """None (the default row everywhere), one (hp_hz, lp_hz) pair for every row, or a pair per row -> [rows] of VBAND_ROW_DTYPE"""
    return _row_settings(rows_cfg, rows, VBAND_ROW_DTYPE, np.uint32, vband_default_row)


class Vband(_PlaneStage):
    """mi_vband: the voice band stage -- the reference's `highpass` / `lowpass` keys as a 511-tap linear-phase FIR per row over the
    demodulator's audio, written as a plane of the same layout (delayed by 255 samples, clamped to [-1, 1]) that the gate, the
    splitter, the PCM stage and the mixer take in its place.  row_enabled: truth value per row (a disabled row's output is not
    written and its carried samples stay); rows_cfg: (hp_hz, lp_hz) for every row or one pair per row, 0 = no edge on that side,
    None = the defaults 100 / 2500.  state() gives rows * 2040 bytes, .view(VBAND_STATE_DTYPE): the 510 input samples a row carries
    into its next call."""
    _destroy, _prefix, _rows_of = "mi_vband_destroy", "mi_vband", _vband_rows

    def process_device(self, d_waveout, row_stride, nbatches, d_out, out_stride, hip_stream=None):
        """Raw device pointers (ints), the strides in floats; d_out [rows][out_stride] must not overlap d_waveout; asynchronous on
        hip_stream."""
        self._call("process_device", d_waveout, row_stride, nbatches, d_out, out_stride, hip_stream)


def vband_plan_host(row_enabled, waveout, rows_cfg=None, state=None, nbatches=None, out=None):
    """mi_vband_plan_host: the voice band stage's plane from audio on the host, no GPU.  waveout: float32 [rows][row_stride];
    rows_cfg as for Vband; state: the blob (rows * 2040 bytes) or None (a fresh one); nbatches: batches of the call, default
    row_stride // WAVE_BATCH; out: float32 [rows][out_stride] to write into (a disabled row's floats stay), default zeros
    [rows][nbatches * WAVE_BATCH].  Returns (out, state after the call)."""
    return _plane_plan_host(lib().mi_vband_plan_host, _vband_rows, VBAND_STATE_DTYPE, row_enabled, waveout, rows_cfg, state, nbatches, out)


def vband_taps(hp_hz, lp_hz):
    """mi_vband_taps: the 511 float32 taps of a row with these settings (0 = no edge on that side)"""
    h = np.zeros(VBAND_TAPS, np.float32)
    _check(lib().mi_vband_taps(int(hp_hz), int(lp_hz), _ptr(h)))
    return h


def limit_default_row():
    """mi_limit_default_row: (1.0, 0.89125094): no gain in front, a ceiling of -1 dBFS"""
    r = lib().mi_limit_default_row()
    return r.pregain, r.ceiling


def _limit_rows(rows_cfg, rows):
    """None (the default row everywhere), one (pregain, ceiling) pair for every row, or a pair per row -> [rows] of LIMIT_ROW_DTYPE"""
    return _row_settings(rows_cfg, rows, LIMIT_ROW_DTYPE, np.float32, limit_default_row)


class Limit(_PlaneStage):
    """mi_limit: the peak limiter stage -- a look-ahead gain per row that keeps a plane of audio (the demodulator's, the voice band
    stage's, a mixer's sum) inside a ceiling without clipping it, written as a plane of the same layout (delayed by 63 samples) that
    the gate, the splitter, the PCM stage and the mixer take in its place.  row_enabled: truth value per row (a disabled row's output
    is not written and its carried samples stay); rows_cfg: (pregain, ceiling) for every row or one pair per row, None = the defaults
    1.0 / 0.89125094.  Rows are independent: no stereo link.  state() gives rows * 4344 bytes, .view(LIMIT_STATE_DTYPE): the 1086
    input samples a row carries into its next call."""
    _destroy, _prefix, _rows_of = "mi_limit_destroy", "mi_limit", _limit_rows

    def process_device(self, d_in, row_stride, nbatches, d_out, out_stride, hip_stream=None):
        """Raw device pointers (ints), the strides in floats; d_out [rows][out_stride] must not overlap d_in; asynchronous on
        hip_stream."""
        self._call("process_device", d_in, row_stride, nbatches, d_out, out_stride, hip_stream)


def limit_plan_host(row_enabled, plane, rows_cfg=None, state=None, nbatches=None, out=None):
    """mi_limit_plan_host: the limiter stage's plane from audio on the host, no GPU.  plane: float32 [rows][row_stride]; rows_cfg as
    for Limit; state: the blob (rows * 4344 bytes) or None (a fresh one); nbatches: batches of the call, default row_stride //
    WAVE_BATCH; out: float32 [rows][out_stride] to write into (a disabled row's floats stay), default zeros [rows][nbatches *
    WAVE_BATCH].  Returns (out, state after the call)."""
    return _plane_plan_host(lib().mi_limit_plan_host, _limit_rows, LIMIT_STATE_DTYPE, row_enabled, plane, rows_cfg, state, nbatches, out)


def limit_pregain_host(records, row, ceiling=None, percentile=0):
    """mi_limit_pregain_host: a pregain for `row` from the splitter's records (TX_RECORD_DTYPE): the ceiling (None = the default row's)
    over the peak at `percentile` (1 .. 100, 0 = 90) of the row's records with blocks, clamped into [2^-10, 2^10]; 1.0 without such
    records.  Returns (pregain, used).  Tried on synthetic signals only."""
    records = np.ascontiguousarray(records, dtype=TX_RECORD_DTYPE).reshape(-1)
    ceiling = limit_default_row()[1] if ceiling is None else ceiling
    pregain, used = C.c_float(0.0), C.c_uint32(0)
    _check(lib().mi_limit_pregain_host(_ptr(records) if records.size else None, records.size, int(row), float(ceiling), int(percentile), C.byref(pregain),
                                       C.byref(used)))
    return np.float32(pregain.value), used.value


def denoise_default_row():
    """mi_denoise_default_row: (reduction_db, over) = (12.0, 4.5)"""
    r = lib().mi_denoise_default_row()
    return r.reduction_db, r.over


def _denoise_rows(rows_cfg, rows):
    """None (the default row everywhere), one (reduction_db, over) pair for every row, or a pair per row -> [rows] of DENOISE_ROW_DTYPE"""
    return _row_settings(rows_cfg, rows, DENOISE_ROW_DTYPE, np.float32, denoise_default_row)


def denoise_fresh_state(rows):
    """the blob of a new handle: zeros in the carried samples, +Inf in the seven carried minima"""
    s = np.zeros(rows, DENOISE_STATE_DTYPE)
    s["m"] = np.inf
    return s.view(np.uint8).reshape(-1)


class Denoise(_PlaneStage):
    """mi_denoise: the noise reduction stage -- a spectral gate per row over a plane of audio: 512-point spectra of 500-sample frames
    at a hop of 250, a noise floor per bin from the minima of the last eight batches, every bin turned down that does not stand above
    `over` times the floor, by `reduction_db` at the most, and the overlap-add of the inverse transforms, written as a plane of the same
    layout (delayed by 250 samples, clamped to [-1, 1]) that the voice band stage, the limiter, the gate, the splitter, the PCM stage
    and the mixer take in its place.  row_enabled: truth value per row (a disabled row's output is not written and its state stays);
    rows_cfg: (reduction_db, over) for every row or one pair per row, None = the defaults 12 / 4.5; either one 0 gives a pure delay.
    state() gives rows * 9196 bytes, .view(DENOISE_STATE_DTYPE): the 500 input samples and the seven minima a row carries into its
    next call."""
    _destroy, _prefix, _rows_of, _launches = "mi_denoise_destroy", "mi_denoise", _denoise_rows, 3

    def process_device(self, d_in, row_stride, nbatches, d_out, out_stride, hip_stream=None):
        """Raw device pointers (ints), the strides in floats; d_out [rows][out_stride] must not overlap d_in; asynchronous on
        hip_stream."""
        self._call("process_device", d_in, row_stride, nbatches, d_out, out_stride, hip_stream)


def denoise_plan_host(row_enabled, plane, rows_cfg=None, state=None, nbatches=None, out=None):
    """mi_denoise_plan_host: the noise reduction stage's plane from audio on the host, no GPU.  plane: float32 [rows][row_stride];
    rows_cfg as for Denoise; state: the blob (rows * 9196 bytes) or None (denoise_fresh_state); nbatches: batches of the call, default
    row_stride // WAVE_BATCH; out: float32 [rows][out_stride] to write into (a disabled row's floats stay), default zeros
    [rows][nbatches * WAVE_BATCH].  Returns (out, state after the call)."""
    state = denoise_fresh_state(len(_flags(row_enabled))) if state is None else state
    return _plane_plan_host(lib().mi_denoise_plan_host, _denoise_rows, DENOISE_STATE_DTYPE, row_enabled, plane, rows_cfg, state, nbatches, out)


def denoise_window():
    """mi_denoise_window: the 500 float32 coefficients of the stage's sine window"""
    w = np.zeros(DENOISE_FRAME, np.float32)
    _check(lib().mi_denoise_window(_ptr(w)))
    return w


def selcal_cfg(mode=SELCAL_16, freq=None, min_energy=0.0, min_tonality=0.0, max_twist=0.0, min_separation=0.0, min_run=0, max_run=0, max_gap=0):
    """mi_selcal_cfg: a table mode (freq: the 2 .. 32 tones of SELCAL_CUSTOM in Hz) and the settings, 0 = the default; a SelcalCfg or
    None (all defaults) passes through"""
    if isinstance(mode, SelcalCfg):
        return mode
    c = SelcalCfg()
    c.mode = int(mode or 0)
    if freq is not None:
        c.ntones = len(freq)
        for i, f in enumerate(list(freq)[:SELCAL_MAX_TONES]):
            c.freq[i] = f
    c.min_energy, c.min_tonality, c.max_twist, c.min_separation = min_energy, min_tonality, max_twist, min_separation
    c.min_run, c.max_run, c.max_gap = min_run, max_run, max_gap
    return c


def selcal_settings(cfg=None):
    """mi_selcal_settings: (the settings with every default filled in, as a SelcalCfg; the constant c of the tonality condition)"""
    out, c = SelcalCfg(), C.c_float()
    _check(lib().mi_selcal_settings(C.byref(selcal_cfg(cfg)), C.byref(out), C.byref(c)))
    return out, np.float32(c.value)


def selcal_max_codes(nbatches, cfg=None):
    """the most codes one row can emit in a call of nbatches batches"""
    return 1 + (2 * nbatches - 1) // (2 * selcal_settings(cfg)[0].min_run)


def selcal_table(cfg=None):
    """mi_selcal_table: (freq [n], coeff [n], letters, a str of n) of the tone table of cfg (None = SELCAL_16)"""
    n = C.c_uint32()
    freq, coeff, letter = np.zeros(SELCAL_MAX_TONES, np.float32), np.zeros(SELCAL_MAX_TONES, np.float32), np.zeros(SELCAL_MAX_TONES, np.uint8)
    _check(lib().mi_selcal_table(C.byref(selcal_cfg(cfg)), C.byref(n), _ptr(freq), _ptr(coeff), _ptr(letter)))
    return freq[:n.value], coeff[:n.value], bytes(letter[:n.value]).decode()


def selcal_window():
    """mi_selcal_window: the 2000 float32 coefficients of the stage's Hann window"""
    w = np.zeros(SELCAL_WINDOW, np.float32)
    _check(lib().mi_selcal_window(_ptr(w)))
    return w


def selcal_code_text(tones, mode=SELCAL_16):
    """mi_selcal_code_text: "AB-CD" from a code record's four tone indices"""
    t = np.ascontiguousarray(tones, dtype=np.uint8)
    assert t.size == 4
    out = np.zeros(6, np.uint8)
    _check(lib().mi_selcal_code_text(int(mode), _ptr(t), _ptr(out)))
    return bytes(out[:5]).decode()


class Selcal(_PostStage):
    """mi_selcal: the SELCAL decoder stage -- per row, which aircraft was called: a Goertzel bank over the SELCAL tone table per window of
    2000 samples at a hop of 1000, the decision whether a window names a pair of tones, and a decoder over the windows that emits one
    code record per call (two pulses of two tones).  It reads a plane of audio (the demodulator's, or what the noise reduction, the
    voice band stage, the limiter or a mixer wrote) and needs no flags.  row_enabled: truth value per row; cfg: selcal_cfg(...) or
    None; max_codes: capacity of the code buffer, 0 = rows * selcal_max_codes(max_batches).  state() gives rows * 4048 bytes, whose
    fields .view(SELCAL_STATE_DTYPE) names."""
    _destroy, _prefix, _launches = "mi_selcal_destroy", "mi_selcal", 5

    def __init__(self, row_enabled, max_batches=1, cfg=None, max_codes=0, gpu=0):
        en = _flags(row_enabled)
        self.cfg = selcal_cfg(cfg)
        self.rows, self.max_batches = en.size, max_batches
        self._h = C.c_void_p()
        _check(lib().mi_selcal_create(C.byref(self.cfg), _ptr(en), self.rows, max_batches, max_codes, gpu, C.byref(self._h)))
        most = self.rows * selcal_max_codes(max_batches, self.cfg)
        self.max_codes = min(max_codes, most) if max_codes else most

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_selcal_set_rows(self._h, _ptr(en)))

    def process_device(self, d_plane, row_stride, nbatches, d_codes, d_row_first_code, d_count, d_windows=None, hip_stream=None):
        """Raw device pointers (ints; d_windows may be None), the stride in floats; asynchronous on hip_stream."""
        self._nwin = 2 * nbatches if d_windows is not None else 0
        _check(lib().mi_selcal_process_device(self._h, d_plane, row_stride, nbatches, d_windows, d_codes, d_row_first_code, d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (codes [k] of SELCAL_CODE_DTYPE, windows [rows][2 * nbatches] of
        SELCAL_WINDOW_DTYPE or None where the call stored none, row_first_code [rows + 1], count [2]) with k = count[1]."""
        codes = np.zeros(self.max_codes, SELCAL_CODE_DTYPE)
        nwin = getattr(self, "_nwin", 0)
        windows = np.zeros((self.rows, nwin), SELCAL_WINDOW_DTYPE) if nwin else None
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_selcal_download(self._h, hip_stream, _ptr(codes), None if windows is None else _ptr(windows), _ptr(row_first), _ptr(count)))
        return codes[:int(count[1])], windows, row_first, count


def selcal_plan_host(row_enabled, plane, cfg=None, state=None, max_codes=0, nbatches=None, want_windows=True):
    """mi_selcal_plan_host: the SELCAL stage's windows and codes from audio on the host, no GPU.  plane: float32 [rows][row_stride];
    state: the blob (rows * 4048 bytes) or None (a fresh one, zeros); nbatches: batches of the call, default row_stride // 2000;
    max_codes: 0 = every code of the call.  Returns (codes [count[1]], windows [rows][2 * nbatches] or None, row_first_code
    [rows + 1], count [2], state after the call)."""
    en = _flags(row_enabled)
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    assert plane.ndim == 2 and plane.shape[0] == en.size
    rows = en.size
    nb = plane.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    c = selcal_cfg(cfg)
    state = np.zeros(rows * SELCAL_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * SELCAL_STATE_DTYPE.itemsize
    cap = max_codes or max(1, rows * selcal_max_codes(max(nb, 1), c))
    codes = np.zeros(cap, SELCAL_CODE_DTYPE)
    windows = np.zeros((rows, 2 * max(nb, 0)), SELCAL_WINDOW_DTYPE) if want_windows else None
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_selcal_plan_host(C.byref(c), _ptr(en), rows, nb, _ptr(plane), plane.shape[1], _ptr(state), None if windows is None else _ptr(windows),
                                     _ptr(codes), cap, _ptr(row_first), _ptr(count)))
    return codes[:int(count[1])], windows, row_first, count, state


def elt_cfg(min_energy=0.0, min_tonality=0.0, band_lo=0, band_hi=0, min_span=0, min_len=0, max_len=0, max_step=0, max_drop=0, max_gap=0, min_sweeps=0):
    """mi_elt_cfg: the settings, 0 = the default; an EltCfg or None (all defaults) passes through"""
    if isinstance(min_energy, EltCfg):
        return min_energy
    c = EltCfg()
    c.min_energy, c.min_tonality = min_energy or 0.0, min_tonality
    c.band_lo, c.band_hi, c.min_span, c.min_len, c.max_len = band_lo, band_hi, min_span, min_len, max_len
    c.max_step, c.max_drop, c.max_gap, c.min_sweeps = max_step, max_drop, max_gap, min_sweeps
    return c


def elt_settings(cfg=None):
    """mi_elt_settings: (the settings with every default filled in, as an EltCfg; the constant c of the tonality condition)"""
    out, c = EltCfg(), C.c_float()
    _check(lib().mi_elt_settings(C.byref(elt_cfg(cfg)), C.byref(out), C.byref(c)))
    return out, np.float32(c.value)


def elt_max_events(nbatches, cfg=None):
    """the most events one row can emit in a call of nbatches batches"""
    s = elt_settings(cfg)[0]
    return 2 * (1 + (ELT_FRAMES * nbatches - 1) // (s.min_sweeps * s.min_len)) + 1


def elt_window():
    """mi_elt_window: the 256 float32 coefficients of the stage's Hann window"""
    w = np.zeros(ELT_FRAME, np.float32)
    _check(lib().mi_elt_window(_ptr(w)))
    return w


def elt_coeffs():
    """mi_elt_coeffs: the 32 float32 recurrence coefficients of bins 2 .. 33"""
    c = np.zeros(ELT_BINS, np.float32)
    _check(lib().mi_elt_coeffs(_ptr(c)))
    return c


def elt_event_text(event):
    """mi_elt_event_text: one printable line from an event record (one element of ELT_EVENT_DTYPE)"""
    e = np.array(event, dtype=ELT_EVENT_DTYPE).reshape(1)
    out = np.zeros(96, np.uint8)
    _check(lib().mi_elt_event_text(_ptr(e), _ptr(out)))
    return bytes(out).split(b"\0")[0].decode()


class Elt(_PostStage):
    """mi_elt: the ELT detector stage -- per row, whether a distress beacon's swept tone is on it and since when: a Goertzel bank over
    the bins 2 .. 33 of 256-sample frames at a hop of 80, the decision whether a frame is tonal and on which bin, and a walker over the
    frames that follows sweeps, chains valid ones and emits one ONSET and one END record per beacon.  It reads a plane of audio as
    Selcal does and needs no flags.  row_enabled: truth value per row; cfg: elt_cfg(...) or None; max_events: capacity of the event
    buffer, 0 = rows * elt_max_events(max_batches).  state() gives rows * 776 bytes, whose fields .view(ELT_STATE_DTYPE) names."""
    _destroy, _prefix, _launches = "mi_elt_destroy", "mi_elt", 5

    def __init__(self, row_enabled, max_batches=1, cfg=None, max_events=0, gpu=0):
        en = _flags(row_enabled)
        self.cfg = elt_cfg(cfg)
        self.rows, self.max_batches = en.size, max_batches
        self._h = C.c_void_p()
        _check(lib().mi_elt_create(C.byref(self.cfg), _ptr(en), self.rows, max_batches, max_events, gpu, C.byref(self._h)))
        most = self.rows * elt_max_events(max_batches, self.cfg)
        self.max_events = min(max_events, most) if max_events else most

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_elt_set_rows(self._h, _ptr(en)))

    def process_device(self, d_plane, row_stride, nbatches, d_events, d_row_first_event, d_count, d_frames=None, hip_stream=None):
        """Raw device pointers (ints; d_frames may be None), the stride in floats; asynchronous on hip_stream."""
        self._nframes = ELT_FRAMES * nbatches if d_frames is not None else 0
        _check(lib().mi_elt_process_device(self._h, d_plane, row_stride, nbatches, d_frames, d_events, d_row_first_event, d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (events [k] of ELT_EVENT_DTYPE, frames [rows][25 * nbatches] of
        ELT_FRAME_DTYPE or None where the call stored none, row_first_event [rows + 1], count [2]) with k = count[1]."""
        events = np.zeros(self.max_events, ELT_EVENT_DTYPE)
        nf = getattr(self, "_nframes", 0)
        frames = np.zeros((self.rows, nf), ELT_FRAME_DTYPE) if nf else None
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_elt_download(self._h, hip_stream, _ptr(events), None if frames is None else _ptr(frames), _ptr(row_first), _ptr(count)))
        return events[:int(count[1])], frames, row_first, count


def elt_plan_host(row_enabled, plane, cfg=None, state=None, max_events=0, nbatches=None, want_frames=True):
    """mi_elt_plan_host: the ELT stage's frame records and events from audio on the host, no GPU.  plane: float32 [rows][row_stride];
    state: the blob (rows * 776 bytes) or None (a fresh one, zeros); nbatches: batches of the call, default row_stride // 2000;
    max_events: 0 = every event of the call.  Returns (events [count[1]], frames [rows][25 * nbatches] or None, row_first_event
    [rows + 1], count [2], state after the call)."""
    en = _flags(row_enabled)
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    assert plane.ndim == 2 and plane.shape[0] == en.size
    rows = en.size
    nb = plane.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    c = elt_cfg(cfg)
    state = np.zeros(rows * ELT_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * ELT_STATE_DTYPE.itemsize
    cap = max_events or max(1, rows * elt_max_events(max(nb, 1), c))
    events = np.zeros(cap, ELT_EVENT_DTYPE)
    frames = np.zeros((rows, ELT_FRAMES * max(nb, 0)), ELT_FRAME_DTYPE) if want_frames else None
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_elt_plan_host(C.byref(c), _ptr(en), rows, nb, _ptr(plane), plane.shape[1], _ptr(state), None if frames is None else _ptr(frames),
                                  _ptr(events), cap, _ptr(row_first), _ptr(count)))
    return events[:int(count[1])], frames, row_first, count, state


def acars_cfg(sync_errors=0, keep_bad=False, min_quality=0.0, hold_timing=False):
    """mi_acars_cfg, field for field as the C struct takes it: sync_errors 1 .. 4 mismatches a sync may have, 0 (or None) = the
    default, 2, and ACARS_SYNC_EXACT for none; keep_bad: frames whose checksum fails are records too; min_quality: floor on Q of a
    sync's batch; hold_timing: no timing moves.  An AcarsCfg passes through."""
    if isinstance(sync_errors, AcarsCfg):
        return sync_errors
    c = AcarsCfg()
    c.sync_errors = int(sync_errors or 0)
    c.keep_bad, c.min_quality, c.hold_timing = int(keep_bad), min_quality, int(hold_timing)
    return c


def acars_settings(cfg=None):
    """mi_acars_settings: the settings with every default filled in, as an AcarsCfg"""
    out = AcarsCfg()
    _check(lib().mi_acars_settings(C.byref(acars_cfg(cfg)), C.byref(out)))
    return out


def acars_max_frames(nbatches):
    """the most frames one row can end in a call of nbatches batches"""
    return 1 + ACARS_BITS * nbatches // 119


def acars_templates():
    """mi_acars_templates: (h1 [20], h2 [20]), the half cycle of 1200 Hz and the full cycle of 2400 Hz over a bit's 20 thirds"""
    h1, h2 = np.zeros(20, np.float32), np.zeros(20, np.float32)
    _check(lib().mi_acars_templates(_ptr(h1), _ptr(h2)))
    return h1, h2


def acars_crc(data):
    """mi_acars_crc: CRC-16/KERMIT of bytes"""
    b = np.frombuffer(bytes(data), np.uint8)
    return int(lib().mi_acars_crc(_ptr(b) if b.size else None, b.size))


def acars_frame_text(frame):
    """mi_acars_frame_text: a record's printable fields, parity stripped, as a dict of str: mode, address, ack, label, block_id, text"""
    f = np.array(frame, ACARS_FRAME_DTYPE).reshape(1)
    out = AcarsText()
    _check(lib().mi_acars_frame_text(_ptr(f), C.byref(out)))
    return {n: getattr(out, n).decode("ascii") for n, _ in AcarsText._fields_}


class Acars(_PostStage):
    """mi_acars: the ACARS decoder stage -- per row, the blocks its 2400 bit/s MSK bursts carried: a bank of coherent bit detectors
    under 20 timing hypotheses per batch, a sync compare on every hypothesis while the row is idle, and a walker that reads the frame's
    bytes, checks parity and the BCS and follows the timing.  It reads a plane of audio as Selcal does and needs no flags.
    row_enabled: truth value per row; cfg: acars_cfg(...) or None; max_frames: capacity of the frame buffer, 0 = rows *
    acars_max_frames(max_batches).  state() gives rows * 496 bytes, whose fields .view(ACARS_STATE_DTYPE) names."""
    _destroy, _prefix, _launches = "mi_acars_destroy", "mi_acars", 5

    def __init__(self, row_enabled, max_batches=1, cfg=None, max_frames=0, gpu=0):
        en = _flags(row_enabled)
        self.cfg = acars_cfg(cfg)
        self.rows, self.max_batches = en.size, max_batches
        self._h = C.c_void_p()
        _check(lib().mi_acars_create(C.byref(self.cfg), _ptr(en), self.rows, max_batches, max_frames, gpu, C.byref(self._h)))
        most = self.rows * acars_max_frames(max_batches)
        self.max_frames = min(max_frames, most) if max_frames else most

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_acars_set_rows(self._h, _ptr(en)))

    def process_device(self, d_plane, row_stride, nbatches, d_frames, d_row_first_frame, d_count, d_bits=None, d_q=None, hip_stream=None):
        """Raw device pointers (ints; d_bits and d_q may be None), the stride in floats; asynchronous on hip_stream."""
        _check(lib().mi_acars_process_device(self._h, d_plane, row_stride, nbatches, d_bits, d_q, d_frames, d_row_first_frame, d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (frames [k] of ACARS_FRAME_DTYPE, row_first_frame [rows + 1],
        count [2]) with k = count[1]."""
        frames = np.zeros(self.max_frames, ACARS_FRAME_DTYPE)
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_acars_download(self._h, hip_stream, _ptr(frames), _ptr(row_first), _ptr(count)))
        return frames[:int(count[1])], row_first, count


def acars_plan_host(row_enabled, plane, cfg=None, state=None, max_frames=0, nbatches=None):
    """mi_acars_plan_host: the ACARS stage's bits, Q and frames from audio on the host, no GPU.  plane: float32 [rows][row_stride];
    state: the blob (rows * 496 bytes) or None (a fresh one, zeros); nbatches: batches of the call, default row_stride // 2000;
    max_frames: 0 = every frame of the call.  Returns (frames [count[1]], bits [rows][nbatches][20][10], q [rows][nbatches][20],
    row_first_frame [rows + 1], count [2], state after the call).  A disabled row's bits and q stay zero."""
    en = _flags(row_enabled)
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    assert plane.ndim == 2 and plane.shape[0] == en.size
    rows = en.size
    nb = plane.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    c = acars_cfg(cfg)
    state = np.zeros(rows * ACARS_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * ACARS_STATE_DTYPE.itemsize
    cap = max_frames or max(1, rows * acars_max_frames(max(nb, 1)))
    frames = np.zeros(cap, ACARS_FRAME_DTYPE)
    bits = np.zeros((rows, max(nb, 0), ACARS_HYPOTHESES, ACARS_BIT_WORDS), np.uint32)
    q = np.zeros((rows, max(nb, 0), ACARS_HYPOTHESES), np.float32)
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_acars_plan_host(C.byref(c), _ptr(en), rows, nb, _ptr(plane), plane.shape[1], _ptr(state), _ptr(bits), _ptr(q), _ptr(frames), cap,
                                    _ptr(row_first), _ptr(count)))
    return frames[:int(count[1])], bits, q, row_first, count, state


def ax25_cfg(gain=None, strict=True):
    """mi_ax25_cfg, field for field as the C struct takes it: gain: the three slicers' weights of the space power, each 0 (or the
    whole None) = its default; strict: False = frames whose address field is not well formed are records too.  An Ax25Cfg passes
    through."""
    if isinstance(gain, Ax25Cfg):
        return gain
    c = Ax25Cfg()
    for g, v in enumerate(gain or (0.0, 0.0, 0.0)):
        c.gain[g] = v
    c.strict = 0 if strict else AX25_STRICT_OFF
    return c


def ax25_settings(cfg=None):
    """mi_ax25_settings: the settings with every default filled in, as an Ax25Cfg"""
    out = Ax25Cfg()
    _check(lib().mi_ax25_settings(C.byref(ax25_cfg(cfg)), C.byref(out)))
    return out


def ax25_max_frames(nbatches):
    """the most records one row can have in a call of nbatches batches"""
    return 1 + AX25_BITS * nbatches // 143


def ax25_templates():
    """mi_ax25_templates: [4][40], cos and sin of 1200 Hz, cos and sin of 2200 Hz over a bit's 40 thirds"""
    t = np.zeros((4, 40), np.float32)
    _check(lib().mi_ax25_templates(_ptr(t)))
    return t


def ax25_crc(data):
    """mi_ax25_crc: CRC-16/X.25 of bytes, complemented as it is sent"""
    b = np.frombuffer(bytes(data), np.uint8)
    return int(lib().mi_ax25_crc(_ptr(b) if b.size else None, b.size))


def ax25_frame_text(frame):
    """mi_ax25_frame_text: a record's TNC2 line SRC-S>DST-S,DIGI-S*,..:info as a str"""
    f = np.array(frame, AX25_FRAME_DTYPE).reshape(1)
    out = C.create_string_buffer(AX25_TEXT_BYTES)
    _check(lib().mi_ax25_frame_text(_ptr(f), out, AX25_TEXT_BYTES))
    return out.value.decode("ascii")


class Ax25(_PostStage):
    """mi_ax25: the packet decoder stage -- per row, the AX.25 frames its 1200 bit/s Bell 202 bursts carried: a bank of tone detectors
    under 10 timing hypotheses and three slicers per batch, and 30 HDLC deframers side by side, whose frames the frame check admits
    and a rule on their positions keeps to one record each.  It reads a plane of audio as Acars does and needs no flags.
    row_enabled: truth value per row; cfg: ax25_cfg(...) or None; max_frames: capacity of the frame buffer, 0 = rows *
    ax25_max_frames(max_batches).  state() gives rows * 10544 bytes, whose fields .view(AX25_STATE_DTYPE) names."""
    _destroy, _prefix, _launches = "mi_ax25_destroy", "mi_ax25", 5

    def __init__(self, row_enabled, max_batches=1, cfg=None, max_frames=0, gpu=0):
        en = _flags(row_enabled)
        self.cfg = ax25_cfg(cfg)
        self.rows, self.max_batches = en.size, max_batches
        self._h = C.c_void_p()
        _check(lib().mi_ax25_create(C.byref(self.cfg), _ptr(en), self.rows, max_batches, max_frames, gpu, C.byref(self._h)))
        most = self.rows * ax25_max_frames(max_batches)
        self.max_frames = min(max_frames, most) if max_frames else most

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_ax25_set_rows(self._h, _ptr(en)))

    def process_device(self, d_plane, row_stride, nbatches, d_frames, d_row_first_frame, d_count, d_bits=None, hip_stream=None):
        """Raw device pointers (ints; d_bits may be None), the stride in floats; asynchronous on hip_stream."""
        _check(lib().mi_ax25_process_device(self._h, d_plane, row_stride, nbatches, d_bits, d_frames, d_row_first_frame, d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (frames [k] of AX25_FRAME_DTYPE, row_first_frame [rows + 1],
        count [2]) with k = count[1]."""
        frames = np.zeros(self.max_frames, AX25_FRAME_DTYPE)
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_ax25_download(self._h, hip_stream, _ptr(frames), _ptr(row_first), _ptr(count)))
        return frames[:int(count[1])], row_first, count


def ax25_plan_host(row_enabled, plane, cfg=None, state=None, max_frames=0, nbatches=None):
    """mi_ax25_plan_host: the packet stage's tone bits and frames from audio on the host, no GPU.  plane: float32 [rows][row_stride];
    state: the blob (rows * 10544 bytes) or None (a fresh one, zeros); nbatches: batches of the call, default row_stride // 2000;
    max_frames: 0 = every frame of the call.  Returns (frames [count[1]], bits [rows][nbatches][3][10][5], row_first_frame [rows + 1],
    count [2], state after the call).  A disabled row's bits stay zero."""
    en = _flags(row_enabled)
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    assert plane.ndim == 2 and plane.shape[0] == en.size
    rows = en.size
    nb = plane.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    c = ax25_cfg(cfg)
    state = np.zeros(rows * AX25_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * AX25_STATE_DTYPE.itemsize
    cap = max_frames or max(1, rows * ax25_max_frames(max(nb, 1)))
    frames = np.zeros(cap, AX25_FRAME_DTYPE)
    bits = np.zeros((rows, max(nb, 0), AX25_SLICERS, AX25_HYPOTHESES, AX25_BIT_WORDS), np.uint32)
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_ax25_plan_host(C.byref(c), _ptr(en), rows, nb, _ptr(plane), plane.shape[1], _ptr(state), _ptr(bits), _ptr(frames), cap,
                                   _ptr(row_first), _ptr(count)))
    return frames[:int(count[1])], bits, row_first, count, state


def pocsag_cfg(baud=0, sync_errors=0, preamble_errors=0, correct=0, hold_timing=False):
    """mi_pocsag_cfg, field for field as the C struct takes it: baud 512, 1200 or 2400, 0 (or None) = 1200; sync_errors 1 .. 4
    mismatches a sync may have, 0 = the default, 2, and POCSAG_SYNC_EXACT for none; preamble_errors 1 .. 8 mismatches of the 32 bits
    before it, 0 = the default, 4, POCSAG_PREAMBLE_EXACT for none, POCSAG_PREAMBLE_OFF to drop the condition; correct: the bits a
    word may have repaired, 1 (0 = the default) or 2, POCSAG_CORRECT_NONE for none; hold_timing: no timing moves.  A PocsagCfg passes
    through."""
    if isinstance(baud, PocsagCfg):
        return baud
    c = PocsagCfg()
    c.baud, c.sync_errors, c.preamble_errors, c.correct, c.hold_timing = int(baud or 0), int(sync_errors or 0), int(preamble_errors or 0), int(correct or 0), int(hold_timing)
    return c


def pocsag_settings(cfg=None):
    """mi_pocsag_settings: the settings with every default filled in, as a PocsagCfg"""
    out = PocsagCfg()
    _check(lib().mi_pocsag_settings(C.byref(pocsag_cfg(cfg)), C.byref(out)))
    return out


def pocsag_geometry(baud=0):
    """mi_pocsag_geometry: (hypotheses H, bits of a batch and hypothesis B, words W) of a baud"""
    h, b, w = C.c_int(), C.c_int(), C.c_int()
    _check(lib().mi_pocsag_geometry(int(baud or 0), C.byref(h), C.byref(b), C.byref(w)))
    return h.value, b.value, w.value


def pocsag_max_messages(nbatches, baud=0):
    """mi_pocsag_max_messages: the most messages one row can close in a call of nbatches batches, 1 + (nbatches (B + 1) - 1) // 32"""
    pocsag_geometry(baud)  # (the refusal of a baud the stage does not have)
    return int(lib().mi_pocsag_max_messages(int(baud or 0), int(nbatches)))


def pocsag_encode(data21):
    """mi_pocsag_encode: the codeword of 21 data bits"""
    return int(lib().mi_pocsag_encode(int(data21)))


def pocsag_decode(word, correct=0):
    """mi_pocsag_decode: (good, the word as stored, e) by the walker's rule for one word under the setting `correct`"""
    fixed, errors = C.c_uint32(), C.c_uint32()
    rc = lib().mi_pocsag_decode(int(word), int(correct), C.byref(fixed), C.byref(errors))
    if rc < 0:
        _check(rc)
    return bool(rc), fixed.value, errors.value


def pocsag_message_text(message, mode=POCSAG_TEXT_AUTO):
    """mi_pocsag_message_text: a record's text as a str: POCSAG_TEXT_NUMERIC, POCSAG_TEXT_ALPHA, or by its function (AUTO)"""
    m = np.array(message, POCSAG_MESSAGE_DTYPE).reshape(1)
    out = C.create_string_buffer(POCSAG_TEXT_BYTES)
    _check(lib().mi_pocsag_message_text(_ptr(m), mode, out, POCSAG_TEXT_BYTES))
    return out.value.decode("ascii")


class Pocsag(_PostStage):
    """mi_pocsag: the pager decoder stage -- per row, the pages its 512 / 1200 / 2400 bit/s POCSAG transmissions carried: a bank of
    bit sums under H timing hypotheses and two slicers per batch, a sync compare of both polarities on every lane while the row is
    idle, and a walker that reads the codewords, repairs them by BCH(31,21), assembles the messages and follows the timing.  It reads
    a plane of audio as Acars does and needs no flags.  row_enabled: truth value per row; cfg: pocsag_cfg(...) or None;
    max_messages: capacity of the message buffer, 0 = rows * pocsag_max_messages(max_batches, baud).  state() gives rows * 800 bytes,
    whose fields .view(POCSAG_STATE_DTYPE) names."""
    _destroy, _prefix, _launches = "mi_pocsag_destroy", "mi_pocsag", 5

    def __init__(self, row_enabled, max_batches=1, cfg=None, max_messages=0, gpu=0):
        en = _flags(row_enabled)
        self.cfg = pocsag_cfg(cfg)
        self.rows, self.max_batches = en.size, max_batches
        self._h = C.c_void_p()
        _check(lib().mi_pocsag_create(C.byref(self.cfg), _ptr(en), self.rows, max_batches, max_messages, gpu, C.byref(self._h)))
        self.hypotheses, self.bits, self.words = pocsag_geometry(self.cfg.baud)
        most = self.rows * pocsag_max_messages(max_batches, self.cfg.baud)
        self.max_messages = min(max_messages, most) if max_messages else most

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_pocsag_set_rows(self._h, _ptr(en)))

    def process_device(self, d_plane, row_stride, nbatches, d_messages, d_row_first_message, d_count, d_bits=None, d_q=None, hip_stream=None):
        """Raw device pointers (ints; d_bits and d_q may be None), the stride in floats; asynchronous on hip_stream."""
        _check(lib().mi_pocsag_process_device(self._h, d_plane, row_stride, nbatches, d_bits, d_q, d_messages, d_row_first_message, d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (messages [k] of POCSAG_MESSAGE_DTYPE, row_first_message
        [rows + 1], count [2]) with k = count[1]."""
        messages = np.zeros(self.max_messages, POCSAG_MESSAGE_DTYPE)
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_pocsag_download(self._h, hip_stream, _ptr(messages), _ptr(row_first), _ptr(count)))
        return messages[:int(count[1])], row_first, count


def pocsag_plan_host(row_enabled, plane, cfg=None, state=None, max_messages=0, nbatches=None):
    """mi_pocsag_plan_host: the pager stage's bits, Q and messages from audio on the host, no GPU.  plane: float32 [rows][row_stride];
    state: the blob (rows * 800 bytes) or None (a fresh one, zeros); nbatches: batches of the call, default row_stride // 2000;
    max_messages: 0 = every message of the call.  Returns (messages [count[1]], bits [rows][nbatches][2][H][W], q [rows][nbatches][2][H],
    row_first_message [rows + 1], count [2], state after the call).  A disabled row's bits and q stay zero."""
    en = _flags(row_enabled)
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    assert plane.ndim == 2 and plane.shape[0] == en.size
    rows = en.size
    nb = plane.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    c = pocsag_cfg(cfg)
    H, _, W = pocsag_geometry(c.baud)
    state = np.zeros(rows * POCSAG_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * POCSAG_STATE_DTYPE.itemsize
    cap = max_messages or max(1, rows * pocsag_max_messages(max(nb, 1), c.baud))
    messages = np.zeros(cap, POCSAG_MESSAGE_DTYPE)
    bits = np.zeros((rows, max(nb, 0), 2, H, W), np.uint32)
    q = np.zeros((rows, max(nb, 0), 2, H), np.float32)
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_pocsag_plan_host(C.byref(c), _ptr(en), rows, nb, _ptr(plane), plane.shape[1], _ptr(state), _ptr(bits), _ptr(q), _ptr(messages), cap,
                                     _ptr(row_first), _ptr(count)))
    return messages[:int(count[1])], bits, q, row_first, count, state


def same_cfg(sync_errors=0, max_bad=0, gap_batches=0, min_quality=0.0, space_gain=0.0, hold_timing=False):
    """mi_same_cfg, field for field as the C struct takes it: sync_errors 1 .. 4 mismatches a sync may have, 0 (or None) = the
    default, 4, and SAME_SYNC_EXACT for none; max_bad: the consecutive bad bytes that end a burst (0 = 4); gap_batches: batches behind
    the last burst that close a message (0 = 20); min_quality: floor on Q of a sync's batch; space_gain: weight of the space power in
    the bit decision (0 = 1); hold_timing: no timing moves.  A SameCfg passes through."""
    if isinstance(sync_errors, SameCfg):
        return sync_errors
    c = SameCfg()
    c.sync_errors, c.max_bad, c.gap_batches = int(sync_errors or 0), int(max_bad), int(gap_batches)
    c.min_quality, c.space_gain, c.hold_timing = min_quality, space_gain, int(hold_timing)
    return c


def same_settings(cfg=None):
    """mi_same_settings: the settings with every default filled in, as a SameCfg"""
    out = SameCfg()
    _check(lib().mi_same_settings(C.byref(same_cfg(cfg)), C.byref(out)))
    return out


def same_max_messages(nbatches):
    """the most messages one row can close in a call of nbatches batches (MI_SAME_MAX_MESSAGES)"""
    return 2 * (2 + 66 * nbatches // 65) + 1


def same_templates():
    """mi_same_templates: [4][768], cos and sin of 4 cycles a bit (mark), cos and sin of 3 (space)"""
    t = np.zeros((4, SAME_BIT_UNITS), np.float32)
    _check(lib().mi_same_templates(_ptr(t)))
    return t


def same_message_text(message):
    """mi_same_message_text: a header record's fields as a dict: originator, event, locations (list of str), purge, issue, station"""
    m = np.array(message, SAME_MESSAGE_DTYPE).reshape(1)
    out = SameText()
    _check(lib().mi_same_message_text(_ptr(m), C.byref(out)))
    d = {n: getattr(out, n).decode("ascii") for n in ("originator", "event", "purge", "issue", "station")}
    d["locations"] = [out.locations[i].value.decode("ascii") for i in range(out.nlocations)]
    return d


class Same(_PostStage):
    """mi_same: the SAME decoder stage -- per row, the weather-alert headers and end-of-message marks its 520.83 bit/s AFSK bursts
    carried: a bank of mark / space detectors under 16 timing hypotheses per batch, a sync compare on every hypothesis while the row
    is idle, a walker that reads the burst's bytes and follows the timing, and an assembler that votes three bursts into a message.
    It reads a plane of audio as Acars does and needs no flags.  row_enabled: truth value per row; cfg: same_cfg(...) or None;
    max_messages: capacity of the message buffer, 0 = rows * same_max_messages(max_batches).  state() gives rows * 1160 bytes, whose
    fields .view(SAME_STATE_DTYPE) names."""
    _destroy, _prefix, _launches = "mi_same_destroy", "mi_same", 5

    def __init__(self, row_enabled, max_batches=1, cfg=None, max_messages=0, gpu=0):
        en = _flags(row_enabled)
        self.cfg = same_cfg(cfg)
        self.rows, self.max_batches = en.size, max_batches
        self._h = C.c_void_p()
        _check(lib().mi_same_create(C.byref(self.cfg), _ptr(en), self.rows, max_batches, max_messages, gpu, C.byref(self._h)))
        most = self.rows * same_max_messages(max_batches)
        self.max_messages = min(max_messages, most) if max_messages else most

    def set_rows(self, row_enabled):
        en = _flags(row_enabled)
        assert en.size == self.rows
        _check(lib().mi_same_set_rows(self._h, _ptr(en)))

    def process_device(self, d_plane, row_stride, nbatches, d_messages, d_row_first_message, d_count, d_bits=None, d_q=None, hip_stream=None):
        """Raw device pointers (ints; d_bits and d_q may be None), the stride in floats; asynchronous on hip_stream."""
        _check(lib().mi_same_process_device(self._h, d_plane, row_stride, nbatches, d_bits, d_q, d_messages, d_row_first_message, d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (messages [k] of SAME_MESSAGE_DTYPE, row_first_message
        [rows + 1], count [2]) with k = count[1]."""
        messages = np.zeros(self.max_messages, SAME_MESSAGE_DTYPE)
        row_first = np.empty(self.rows + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_same_download(self._h, hip_stream, _ptr(messages), _ptr(row_first), _ptr(count)))
        return messages[:int(count[1])], row_first, count


def same_plan_host(row_enabled, plane, cfg=None, state=None, max_messages=0, nbatches=None):
    """mi_same_plan_host: the SAME stage's bits, Q and messages from audio on the host, no GPU.  plane: float32 [rows][row_stride];
    state: the blob (rows * 1160 bytes) or None (a fresh one, zeros); nbatches: batches of the call, default row_stride // 2000;
    max_messages: 0 = every message of the call.  Returns (messages [count[1]], bits [rows][nbatches][16][4], q [rows][nbatches][16],
    row_first_message [rows + 1], count [2], state after the call).  A disabled row's bits and q stay zero."""
    en = _flags(row_enabled)
    plane = np.ascontiguousarray(plane, dtype=np.float32)
    assert plane.ndim == 2 and plane.shape[0] == en.size
    rows = en.size
    nb = plane.shape[1] // WAVE_BATCH if nbatches is None else nbatches
    c = same_cfg(cfg)
    state = np.zeros(rows * SAME_STATE_DTYPE.itemsize, np.uint8) if state is None else np.array(state, copy=True).view(np.uint8).reshape(-1)
    assert state.size == rows * SAME_STATE_DTYPE.itemsize
    cap = max_messages or max(1, rows * same_max_messages(max(nb, 1)))
    messages = np.zeros(cap, SAME_MESSAGE_DTYPE)
    bits = np.zeros((rows, max(nb, 0), SAME_HYPOTHESES, SAME_BIT_WORDS), np.uint32)
    q = np.zeros((rows, max(nb, 0), SAME_HYPOTHESES), np.float32)
    row_first = np.empty(rows + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_same_plan_host(C.byref(c), _ptr(en), rows, nb, _ptr(plane), plane.shape[1], _ptr(state), _ptr(bits), _ptr(q), _ptr(messages), cap,
                                   _ptr(row_first), _ptr(count)))
    return messages[:int(count[1])], bits, q, row_first, count, state


def _aspec_cfg(lo_hz=0, hi_hz=0):
    """a band in Hz (0 = 60 / 3800), or an AspecCfg -> AspecCfg"""
    return lo_hz if isinstance(lo_hz, AspecCfg) else AspecCfg(int(lo_hz or 0), int(hi_hz or 0))


def aspec_band(lo_hz=0, hi_hz=0):
    """mi_aspec_band: (lo_bin, hi_bin) of the band, 8 and 486 at the defaults; bin j is j * 7.8125 Hz"""
    lo, hi = C.c_uint32(0), C.c_uint32(0)
    _check(lib().mi_aspec_band(C.byref(_aspec_cfg(lo_hz, hi_hz)), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def aspec_window():
    """mi_aspec_window: the 2000 float32 coefficients of the stage's Hann window"""
    w = np.zeros(WAVE_BATCH, np.float32)
    _check(lib().mi_aspec_window(_ptr(w)))
    return w


class Aspec(_PostStage):
    """mi_aspec: the audio spectrum stage -- a 2048-point power spectrum (1024 bins of 7.8125 Hz) of every block the output gate lets
    travel, one ASPEC_RECORD_DTYPE record per block (strongest band bin, band and line power), optionally the power rows and one mean
    spectrum per row, from which aspec_notch_host reads a notch frequency.  Stateless: there is no state blob and no row mask.
    max_blocks: capacity of the destinations in blocks, 0 = rows * max_batches."""
    _destroy, _prefix, _launches = "mi_aspec_destroy", "mi_aspec", 2

    def __init__(self, rows, max_batches=1, lo_hz=0, hi_hz=0, max_blocks=0, gpu=0):
        self.rows, self.max_batches = int(rows), max_batches
        self.max_blocks = min(max_blocks, self.rows * max_batches) if max_blocks else self.rows * max_batches
        self._h = C.c_void_p()
        self._wrote = (False, False)
        _check(lib().mi_aspec_create(C.byref(_aspec_cfg(lo_hz, hi_hz)), self.rows, max_batches, max_blocks, gpu, C.byref(self._h)))

    def process_device(self, d_waveout, row_stride, nbatches, d_index, d_row_first, d_count, d_records, d_power=None, d_row_mean=None,
                       d_row_blocks=None, hip_stream=None):
        """Raw device pointers (ints; d_power, d_row_mean with d_row_blocks, and d_row_first without a row mean may be None), the
        stride in floats; d_index, d_row_first and d_count as OutputGate.process_device left them; asynchronous on hip_stream."""
        _check(lib().mi_aspec_process_device(self._h, d_waveout, row_stride, nbatches, d_index, d_row_first, d_count, d_records, d_power, d_row_mean,
                                             d_row_blocks, hip_stream))
        self._wrote = (d_power is not None, d_row_mean is not None)

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (records [k] of ASPEC_RECORD_DTYPE, power [k][1024] or None,
        row_mean [rows][1024] or None, row_blocks [rows] or None, count [2]) with k = count[1], the number of blocks stored; None
        where the call wrote none."""
        records = np.zeros(self.max_blocks, ASPEC_RECORD_DTYPE)
        power = np.zeros((self.max_blocks, ASPEC_BINS), np.float32) if self._wrote[0] else None
        mean = np.zeros((self.rows, ASPEC_BINS), np.float32) if self._wrote[1] else None
        blocks = np.zeros(self.rows, np.uint32) if self._wrote[1] else None
        count = np.zeros(2, np.uint32)
        _check(lib().mi_aspec_download(self._h, hip_stream, _ptr(records), None if power is None else _ptr(power), None if mean is None else _ptr(mean),
                                       None if blocks is None else _ptr(blocks), _ptr(count)))
        k = int(count[1])
        return records[:k], None if power is None else power[:k], mean, blocks, count


def aspec_plan_host(rows, waveout, index, row_first=None, lo_hz=0, hi_hz=0, nbatches=None, want_power=True):
    """mi_aspec_plan_host: the stage's records, power rows and row means from audio and an index on the host, no GPU.  waveout:
    float32 [rows][row_stride]; index: [k][2] = (row, batch), any order; row_first: [rows + 1] as gate_plan_host gives it, or None (no
    row mean); nbatches: batches of the call, default row_stride // WAVE_BATCH.  Returns (records [k], power [k][1024] or None,
    row_mean [rows][1024] or None, row_blocks [rows] or None)."""
    waveout = np.ascontiguousarray(waveout, dtype=np.float32)
    assert waveout.ndim == 2 and waveout.shape[0] == rows
    row_stride = waveout.shape[1]
    nb = row_stride // WAVE_BATCH if nbatches is None else nbatches
    index = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1, 2)
    k = len(index)
    records = np.zeros(k, ASPEC_RECORD_DTYPE)
    power = np.zeros((k, ASPEC_BINS), np.float32) if want_power else None
    first = None if row_first is None else np.ascontiguousarray(row_first, dtype=np.uint32)
    assert first is None or first.size == rows + 1
    mean = None if first is None else np.zeros((rows, ASPEC_BINS), np.float32)
    blocks = None if first is None else np.zeros(rows, np.uint32)
    _check(lib().mi_aspec_plan_host(C.byref(_aspec_cfg(lo_hz, hi_hz)), rows, nb, _ptr(waveout), row_stride, _ptr(index) if k else None, k,
                                    None if first is None else _ptr(first), _ptr(records) if k else None, _ptr(power) if want_power and k else None,
                                    None if mean is None else _ptr(mean), None if blocks is None else _ptr(blocks)))
    return records, power, mean, blocks


def aspec_notch_host(row_mean, row_blocks, records=None, lo_hz=0, hi_hz=0, min_blocks=0, ratio=0.0):
    """mi_aspec_notch_host: an AspecNotch (found, bin, freq_hz, peak, floor, votes, blocks) from one row's mean spectrum [1024], its
    block count and its records (or None); min_blocks 0 = 8, ratio 0 = 16.0.  freq_hz is what a channel's notch takes when found."""
    mean = np.ascontiguousarray(row_mean, dtype=np.float32)
    assert mean.shape == (ASPEC_BINS,)
    recs = np.zeros(0, ASPEC_RECORD_DTYPE) if records is None else np.ascontiguousarray(records, dtype=ASPEC_RECORD_DTYPE)
    out = AspecNotch()
    _check(lib().mi_aspec_notch_host(_ptr(mean), int(row_blocks), _ptr(recs) if len(recs) else None, len(recs), C.byref(_aspec_cfg(lo_hz, hi_hz)),
                                     C.byref(AspecRule(int(min_blocks or 0), float(ratio or 0.0))), C.byref(out)))
    return out


def tones_table(window=0):
    """mi_tones_table: (freq [51], coeff [51], alias_of [51]) of the tone table at `window` samples (0 = 6400)"""
    freq, coeff, alias = np.zeros(TONES_STANDARD, np.float32), np.zeros(TONES_STANDARD, np.float32), np.zeros(TONES_STANDARD, np.uint32)
    _check(lib().mi_tones_table(int(window or 0), _ptr(freq), _ptr(coeff), _ptr(alias)))
    return freq, coeff, alias


def tones_vote_host(records, min_windows=0, min_share_permille=0):
    """mi_tones_vote_host: one row's records (TONE_RECORD_DTYPE) -> TonesVote; 0 = the defaults, 2 windows and 500 permille"""
    records = np.ascontiguousarray(records, dtype=TONE_RECORD_DTYPE)
    out = TonesVote()
    _check(lib().mi_tones_vote_host(_ptr(records) if records.size else None, records.size, C.byref(TonesRule(min_windows, min_share_permille)),
                                    C.byref(out)))
    return out


class Survey(_TimedStage):
    """mi_survey: per-bin mean and peak magnitude of every cell of windows_per_cell consecutive windows (0 = WAVE_BATCH), over the full
    FFT of the windows stage 1 runs -- the pass that comes before a channel plan.  Stateless between calls; no state blob."""
    _destroy, _prefix, _launches = "mi_survey_destroy", "mi_survey", 2

    def __init__(self, dev, nstreams=1, max_cells=1, windows_per_cell=0, gpu=0):
        self.nstreams, self.max_cells = nstreams, max_cells
        self.windows_per_cell = windows_per_cell or WAVE_BATCH
        self.fft_size = 1 << dev.fft_size_log
        self._h = C.c_void_p()
        _check(lib().mi_survey_create(C.byref(dev), nstreams, max_cells, windows_per_cell, gpu, C.byref(self._h)))

    def set_streams(self, enabled=None):
        """enabled: truth value per stream, or None = all.  A disabled stream is neither read nor written."""
        en = None if enabled is None else _flags(enabled)
        assert en is None or en.size == self.nstreams
        _check(lib().mi_survey_set_streams(self._h, None if en is None else _ptr(en)))

    def bytes_needed(self, ncells):
        return lib().mi_survey_bytes_needed(self._h, ncells)

    def process_device(self, d_iq, stream_stride, ncells, d_mean, d_peak, hip_stream=None):
        """Raw device pointers (ints): d_mean and d_peak float32 [nstreams][ncells][fft_size]; asynchronous on hip_stream."""
        _check(lib().mi_survey_process_device(self._h, d_iq, stream_stride, ncells, d_mean, d_peak, hip_stream))


def survey_bin_range(dev, bin):
    """mi_survey_bin_range: (lo_hz, hi_hz), a closed range of integer frequencies inside the band that the plan's bin rule maps to
    `bin` (the bin's longest piece; see include/mi_airband.h).  No GPU."""
    lo, hi = C.c_int(), C.c_int()
    _check(lib().mi_survey_bin_range(C.byref(dev), bin, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def _occ_cfg(cfg):
    """None, an OccCfg or (floor_permille, ratio, min_cells) -> a pointer to an OccCfg, or None (all defaults)"""
    if cfg is None:
        return None
    return C.byref(cfg if isinstance(cfg, OccCfg) else OccCfg(int(cfg[0]), float(cfg[1]), int(cfg[2])))


class Occupancy(_TimedStage):
    """mi_occupancy: the channel finder -- from the survey's planes to one OCC_BIN_DTYPE record per (stream, bin) and to channel
    candidates (OCC_CAND_DTYPE), the maximal runs of occupied bins in frequency order.  cfg: (floor_permille, ratio, min_cells), 0 = the
    default 250 / 3.0 / 1; max_candidates: capacity of the candidate buffer, 0 = nstreams * fft_size / 2.  Stateless between calls."""
    _destroy, _prefix, _launches = "mi_occupancy_destroy", "mi_occupancy", 4

    def __init__(self, dev, nstreams=1, max_cells=1, cfg=None, max_candidates=0, gpu=0):
        self.nstreams, self.max_cells = nstreams, max_cells
        self.fft_size = 1 << dev.fft_size_log
        most = nstreams * self.fft_size // 2
        self.max_candidates = min(max_candidates, most) if max_candidates else most
        self._h = C.c_void_p()
        _check(lib().mi_occupancy_create(C.byref(dev), _occ_cfg(cfg), nstreams, max_cells, max_candidates, gpu, C.byref(self._h)))

    def set_streams(self, enabled=None):
        """enabled: truth value per stream, or None = all.  A disabled stream is not read, gets no bin record and no candidate."""
        en = None if enabled is None else _flags(enabled)
        assert en is None or en.size == self.nstreams
        _check(lib().mi_occupancy_set_streams(self._h, None if en is None else _ptr(en)))

    def process_device(self, d_mean, d_peak, ncells, d_bins, d_cands, d_stream_first, d_count, hip_stream=None):
        """Raw device pointers (ints): d_mean and d_peak float32 [nstreams][ncells][fft_size] as Survey.process_device wrote them;
        asynchronous on hip_stream."""
        _check(lib().mi_occupancy_process_device(self._h, d_mean, d_peak, ncells, d_bins, d_cands, d_stream_first, d_count, hip_stream))

    def download(self, hip_stream=None):
        """Results of the last process_device (enqueued on hip_stream): (bins [nstreams][fft_size] of OCC_BIN_DTYPE, candidates [k] of
        OCC_CAND_DTYPE, stream_first [nstreams + 1], count [2]) with k = count[1], the number of candidates stored."""
        bins = np.zeros((self.nstreams, self.fft_size), OCC_BIN_DTYPE)
        cands = np.zeros(self.max_candidates, OCC_CAND_DTYPE)
        first = np.empty(self.nstreams + 1, np.uint32)
        count = np.zeros(2, np.uint32)
        _check(lib().mi_occupancy_download(self._h, hip_stream, _ptr(bins), _ptr(cands), _ptr(first), _ptr(count)))
        return bins, cands[:int(count[1])], first, count


def occupancy_plan_host(dev, mean, peak, cfg=None, enabled=None, max_candidates=0, bins=None, cands=None):
    """mi_occupancy_plan_host: the finder on the host, no GPU.  mean, peak: float32 [nstreams][ncells][fft_size]; enabled: truth value per
    stream or None = all.  bins / cands: arrays to write into (a test's sentinel-filled ones), default fresh zeros.  Returns (bins
    [nstreams][fft_size], cands -- the whole buffer if one was given, else the count[1] stored --, stream_first [nstreams + 1], count [2])."""
    mean = np.ascontiguousarray(mean, dtype=np.float32)
    peak = np.ascontiguousarray(peak, dtype=np.float32)
    n = 1 << dev.fft_size_log
    assert mean.ndim == 3 and mean.shape == peak.shape
    ns, ncells = mean.shape[0], mean.shape[1]
    en = None if enabled is None else _flags(enabled)
    assert en is None or en.size == ns
    cap = max_candidates or ns * n // 2
    given = cands is not None
    bins = np.zeros((ns, n), OCC_BIN_DTYPE) if bins is None else bins
    cands = np.zeros(cap, OCC_CAND_DTYPE) if cands is None else cands
    assert bins.dtype == OCC_BIN_DTYPE and bins.size >= ns * n and cands.dtype == OCC_CAND_DTYPE and cands.size >= min(cap, ns * n // 2)
    first = np.empty(ns + 1, np.uint32)
    count = np.zeros(2, np.uint32)
    _check(lib().mi_occupancy_plan_host(C.byref(dev), _occ_cfg(cfg), None if en is None else _ptr(en), ns, _ptr(mean), _ptr(peak), ncells, _ptr(bins),
                                        _ptr(cands), max_candidates, _ptr(first), _ptr(count)))
    return bins, (cands if given else cands[:int(count[1])]), first, count


def _probe_targets(targets):
    """a PROBE_TARGET_DTYPE array, or (stream, bin) pairs -> a contiguous PROBE_TARGET_DTYPE array"""
    if isinstance(targets, np.ndarray) and targets.dtype == PROBE_TARGET_DTYPE:
        return np.ascontiguousarray(targets)
    return np.array([(int(s), int(b)) for s, b in targets], PROBE_TARGET_DTYPE)


class Probe(_TimedStage):
    """mi_probe: the channel probe -- for a list of targets (stream, bin), one PROBE_CELL_DTYPE record per (target, cell) with the
    float64 sums of the bin's envelope and of z_w * conj(z_(w-1)) over the cell's windows.  The windows are the survey's.  Stateless
    between calls; the target list stays until it is replaced."""
    _destroy, _prefix, _launches = "mi_probe_destroy", "mi_probe", 2

    def __init__(self, dev, nstreams=1, max_cells=1, windows_per_cell=0, max_targets=1, gpu=0):
        self.nstreams, self.max_cells, self.max_targets = nstreams, max_cells, max_targets
        self.windows_per_cell = windows_per_cell or WAVE_BATCH
        self.fft_size = 1 << dev.fft_size_log
        self.ntargets = self._last = 0
        self._h = C.c_void_p()
        _check(lib().mi_probe_create(C.byref(dev), nstreams, max_cells, windows_per_cell, max_targets, gpu, C.byref(self._h)))

    def set_targets(self, targets):
        """targets: (stream, bin) pairs or a PROBE_TARGET_DTYPE array, strictly ascending.  A refused list leaves the old one."""
        t = _probe_targets(targets)
        _check(lib().mi_probe_set_targets(self._h, _ptr(t), t.size))
        self.ntargets = t.size

    def bytes_needed(self, ncells):
        return lib().mi_probe_bytes_needed(self._h, ncells)

    def process_device(self, d_iq, stream_stride, ncells, d_cells, hip_stream=None):
        """Raw device pointers (ints): d_cells [ntargets][ncells] of 40-byte records; asynchronous on hip_stream."""
        _check(lib().mi_probe_process_device(self._h, d_iq, stream_stride, ncells, d_cells, hip_stream))
        self._last = (self.ntargets, ncells)

    def download(self, hip_stream=None):
        """The records of the last process_device (enqueued on hip_stream): PROBE_CELL_DTYPE [ntargets][ncells]."""
        cells = np.zeros(self._last or (0, 0), PROBE_CELL_DTYPE)
        _check(lib().mi_probe_download(self._h, hip_stream, _ptr(cells)))
        return cells


def probe_targets_from_candidates(cands):
    """mi_probe_targets_from_candidates: OCC_CAND_DTYPE [n] -> PROBE_TARGET_DTYPE [n], best_bin of each, sorted by (stream, bin).  No GPU."""
    cands = np.ascontiguousarray(cands, dtype=OCC_CAND_DTYPE)
    out = np.zeros(cands.size, PROBE_TARGET_DTYPE)
    _check(lib().mi_probe_targets_from_candidates(_ptr(cands), cands.size, _ptr(out)))
    return out


def probe_features_host(dev, bin, cells, mask=None):
    """mi_probe_features_host: the ProbeFeatures of one target from its PROBE_CELL_DTYPE [ncells] records; mask: truth value per cell or
    None = all.  No GPU."""
    cells = np.ascontiguousarray(cells, dtype=PROBE_CELL_DTYPE)
    assert cells.ndim == 1
    m = None if mask is None else _flags(mask)
    assert m is None or m.size == cells.size
    f = ProbeFeatures()
    _check(lib().mi_probe_features_host(C.byref(dev), bin, _ptr(cells), cells.size, None if m is None else _ptr(m), C.byref(f)))
    return f


def probe_classify_host(features, rule=None):
    """mi_probe_classify_host: MOD_AM or MOD_NFM; rule: None, a ProbeRule or (coherence_max, cv2_min), 0 = the default.  No GPU."""
    r = None if rule is None else C.byref(rule if isinstance(rule, ProbeRule) else ProbeRule(float(rule[0]), float(rule[1])))
    mod = C.c_int(-1)
    _check(lib().mi_probe_classify_host(C.byref(features), r, C.byref(mod)))
    return mod.value


# ---- the BASELINE.json channel plans ----

def config2_channels():
    """8 AM channels at centre -1.0 MHz + 25 kHz + k*250 kHz (bins 316,366,416,466,4,54,104,154 at fft 512)."""
    centre = 120000000
    return centre, [channel_cfg(centre - 1000000 + 25000 + k * 250000) for k in range(8)]


def config3_channels():
    """32 channels spaced 70 kHz, even = AM, odd = NFM with bandwidth 12500; every 4th NFM has ctcss 100.0,
    one has notch 100.0; fft 2048."""
    centre = 120000000
    chans = []
    nfm_idx = 0
    for k in range(32):
        f = centre - 1120000 + 35000 + k * 70000
        if k % 2 == 0:
            chans.append(channel_cfg(f))
        else:
            ct = 100.0 if nfm_idx % 4 == 0 else 0.0
            notch = 100.0 if nfm_idx == 0 else 0.0
            chans.append(channel_cfg(f, modulation=MOD_NFM, bandwidth=12500, ctcss=ct, notch=notch))
            nfm_idx += 1
    return centre, chans


def carriers_for(centre, chans, amp_q8=3072, active=lambda k: k % 2 == 0):
    """One synthetic carrier per active channel: AM for AM channels, NFM (+CTCSS where configured) otherwise."""
    out = []
    for k, c in enumerate(chans):
        if not active(k):
            continue
        kind = 0 if c.modulation == MOD_AM else (2 if c.ctcss_freq > 0 else 1)
        out.append((c.freq - centre, kind, amp_q8, 0))
    return out
