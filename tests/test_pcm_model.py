"""The PCM stage's definition, pinned without a GPU: the taps and their response, mi_pcm_plan_host (csrc/poststage_host.cpp) against
the numpy model of pcm_model.py as bytes -- blocks and the state blob --, the IMA encoder against the standard library's and against a
separately written decoder, the WAV containers through the `wave` module and `struct`, the exported symbols and every refusal."""
import ctypes as C
import io
import os
import re
import struct
import wave as wavefile

import numpy as np
import pytest

import pcm_model as pm
from pcm_model import CONFIGS, HISTORY, IMA4, IMA_BYTES, IMA_SAMPLES, S16, WAVE_BATCH, audio, pcm_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCM_SYMBOLS = {"mi_pcm_create", "mi_pcm_destroy", "mi_pcm_set_rows", "mi_pcm_process_device", "mi_pcm_download", "mi_pcm_state_size",
               "mi_pcm_get_state", "mi_pcm_set_state", "mi_pcm_set_timing", "mi_pcm_last_launch_ms", "mi_pcm_block_bytes", "mi_pcm_taps",
               "mi_pcm_plan_host", "mi_pcm_wav_header"}
SENT = 0xA5
INVALID, NO_DEVICE = -1, -2


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------- taps ----------------

def test_taps_against_the_model(pkg):
    h, want = pkg.pcm_taps(), pm.taps()
    assert h.dtype == np.float32 and h.shape == (63,)
    assert (np.abs(h.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all(), "more than one float32 step"
    assert h.tobytes() == h[::-1].tobytes(), "not symmetric bit for bit"
    c = np.arange(63) - 31
    zero = (c % 2 == 0) & (c != 0)
    assert (h[zero].view(np.uint32) == 0).all() and zero.sum() == 30 and (h[~zero & (np.arange(63) % 62 != 0)] != 0).all()
    assert abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6


def test_response_of_the_returned_taps(pkg):
    """conditions on the design, not tolerances of the device: +-0.01 dB up to 3 kHz, below -70 dB from 4.7 kHz (what folds back under
    3.3 kHz after the decimation).  The float64 design gives +-0.0015 dB and -71.7 dB."""
    h = pkg.pcm_taps()
    low, high = np.arange(0.0, 3000.5, 5.0), np.arange(4700.0, 8000.5, 5.0)
    for name, taps in (("float64 design", pm.design64()), ("returned float32 taps", h)):
        ripple, stop = np.abs(pm.response_db(taps, low)).max(), pm.response_db(taps, high).max()
        print(f"{name}: passband ripple {ripple:.5f} dB up to 3 kHz, stopband {stop:.2f} dB from 4.7 kHz")
        assert ripple <= 0.01 and stop <= -70.0
    assert np.abs(pm.response_db(pm.design64(), low)).max() <= 0.0016 and pm.response_db(pm.design64(), high).max() <= -71.6


def test_tie_builder_finds_even_and_odd(pkg):
    ns, xs = pm.tie_values()
    q = pm.quantise(xs)
    assert (q % 2 == 0).all() and (np.abs(q - (ns + 0.5)) == 0.5).all()  # half to even, whichever side that is
    assert (pm.quantise(-xs) == -q).all()


# ---------------- the twin against the model ----------------

def twin(pkg, wave, index, state, enabled, rate, fmt, nbatches=None):
    rows = wave.shape[0]
    en = np.ones(rows, np.uint8) if enabled is None else enabled
    return pkg.pcm_plan_host(en, wave, index, None if state is None else state, rate, fmt, nbatches=nbatches)


@pytest.mark.parametrize("rate,fmt", CONFIGS)
@pytest.mark.parametrize("rows", [1, 5])
def test_twin_equals_model_on_every_builder(pkg, rows, rate, fmt):
    nb = 3
    for name in pm.BUILDERS:
        wave = audio(name, rows, nb)
        index = pm.drawn_index(rows, nb, seed=rows)
        want, after = pcm_model(wave, index, rate=rate, fmt=fmt)
        got, state = twin(pkg, wave, index, None, None, rate, fmt)
        assert got.shape == (len(index), pkg.pcm_block_bytes(rate, fmt)) == (len(index), pm.block_bytes(rate, fmt))
        assert got.tobytes() == want.tobytes(), f"{name}: blocks"
        assert state.tobytes() == after.tobytes(), f"{name}: state"
        assert state.view(np.float32).reshape(rows, HISTORY).tobytes() == wave[:, -HISTORY:].tobytes()


def test_builders_reach_what_they_are_for():
    """the square wave: index0's fallback, index 88 and the predictor clamp at 16000, the quantiser clamp at 8000; the ties: both
    parities; silence and the subnormal values: all-zero samples"""
    sq = audio("square", 5, 2)
    s16k, _ = pm.block_samples(sq, pm.full_index(5, 2), pm.fresh_state(5), 16000, 2)
    sub = s16k[0].reshape(-1, IMA_SAMPLES)
    assert (np.abs(sub[:, 0]) == 32767).all() and (sub[:, 0] == -sub[:, 1]).all()
    blocks, preds, indices, clamps = pm.ima_encode(s16k.reshape(-1, IMA_SAMPLES), trace=True)
    assert (blocks[:len(sub), 2] == 88).all() and (indices == 88).any() and (indices == 0).any() and clamps.any()
    s8k, _ = pm.block_samples(sq, pm.full_index(5, 2), pm.fresh_state(5), 8000, 2)
    y = pm.fir(np.concatenate([np.zeros((5, HISTORY), np.float32), sq[:, :WAVE_BATCH]], axis=1))
    assert (np.abs(y) > 1.0).any() and np.abs(s8k).max() == 32767
    t = pm.quantise(audio("ties", 1, 1))
    assert (t % 2 == 0).all() and len(np.unique(t)) > 30
    for name in ("silence", "subnormal"):
        for rate in (8000, 16000):
            assert not pm.block_samples(audio(name, 2, 2), pm.full_index(2, 2), pm.fresh_state(2), rate, 2)[0].any()


@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_call_cuts_give_identical_blocks(pkg, rate, fmt):
    """the same 4 batches as one call, as four calls and as 1 + 3: a block's 62 samples of history come from the row's previous batch
    or from the carried state, and the bytes do not depend on which"""
    rows, nb = 3, 4
    for name in ("voice", "noise", "square"):
        wave = audio(name, rows, nb)
        whole, whole_state = twin(pkg, wave, pm.full_index(rows, nb), None, None, rate, fmt)
        whole = whole.reshape(rows, nb, -1)
        for cuts in ((1, 1, 1, 1), (1, 3)):
            state, done = None, 0
            for n in cuts:
                part = np.ascontiguousarray(wave[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH])
                got, state = twin(pkg, part, pm.full_index(rows, n), state, None, rate, fmt)
                want, want_state = pcm_model(part, pm.full_index(rows, n), state=None if done == 0 else prev, rate=rate, fmt=fmt)
                assert got.tobytes() == want.tobytes() and state.tobytes() == want_state.tobytes()
                assert got.reshape(rows, n, -1).tobytes() == whole[:, done:done + n].tobytes(), f"{name}, cuts {cuts}, batch {done}"
                prev, done = state, done + n
            assert state.tobytes() == whole_state.tobytes()


@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_a_disabled_row_keeps_its_samples(pkg, rate, fmt):
    """row 1 sits the second of three calls out: its carried samples keep their bytes, so the third call's batch 0 continues from
    the first call's tail; its blocks in the second call's index are encoded from what is there"""
    rows = 3
    wave = audio("noise", rows, 3)
    masks = [np.ones(rows, np.uint8), np.array([1, 0, 1], np.uint8), np.ones(rows, np.uint8)]
    state, model_state = None, None
    for i in range(3):
        part = np.ascontiguousarray(wave[:, i * WAVE_BATCH:(i + 1) * WAVE_BATCH])
        got, state = twin(pkg, part, pm.full_index(rows, 1), state, masks[i], rate, fmt)
        want, model_state = pcm_model(part, pm.full_index(rows, 1), model_state, masks[i], rate, fmt)
        assert got.tobytes() == want.tobytes() and state.tobytes() == model_state.tobytes(), f"call {i}"
        tails = state.view(np.float32).reshape(rows, HISTORY)
        assert tails[0].tobytes() == part[0, -HISTORY:].tobytes()
        assert tails[1].tobytes() == wave[1, (1 if i == 1 else i + 1) * WAVE_BATCH - HISTORY:(1 if i == 1 else i + 1) * WAVE_BATCH].tobytes()


@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_unsorted_repeated_and_out_of_range_entries(pkg, rate, fmt):
    rows, nb = 3, 3
    wave = audio("voice", rows, nb)
    index = np.array([[2, 1], [0, 2], [0, 0], [2, 1], [1, 0], [rows, 0], [0, nb], [0xFFFFFFFF, 0xFFFFFFFF], [1, 2]], np.uint32)
    got, state = twin(pkg, wave, index, None, None, rate, fmt)
    want, after = pcm_model(wave, index, rate=rate, fmt=fmt)
    assert got.tobytes() == want.tobytes() and state.tobytes() == after.tobytes()
    assert got[0].tobytes() == got[3].tobytes() and got[0].any()
    assert not got[5:8].any() and got[8].any()
    # batch >= nbatches is out of range even where the buffer is longer than the call
    got2, _ = twin(pkg, wave, np.array([[0, 1], [0, 2]], np.uint32), None, None, rate, fmt, nbatches=2)
    assert got2[0].any() and not got2[1].any()


@pytest.mark.parametrize("rate,fmt", CONFIGS)
def test_capped_nblocks_leaves_the_rest_alone(pkg, rate, fmt):
    rows, nb = 2, 2
    wave = audio("noise", rows, nb)
    index = pm.full_index(rows, nb)
    bb = pm.block_bytes(rate, fmt)
    want, after = pcm_model(wave, index[:3], rate=rate, fmt=fmt)
    out = np.full((len(index) + 1) * bb, SENT, np.uint8)
    state = np.zeros(rows * 248 + 16, np.uint8)
    state[rows * 248:] = SENT
    en = np.ones(rows, np.uint8)
    cfg = pkg.PcmCfg(rate, fmt)
    rc = pkg.lib().mi_pcm_plan_host(C.byref(cfg), ptr(en), rows, nb, ptr(wave), wave.shape[1], ptr(index), 3, ptr(state), ptr(out))
    assert rc == 0
    assert out[:3 * bb].tobytes() == want.tobytes() and (out[3 * bb:] == SENT).all()
    assert state[:rows * 248].tobytes() == after.tobytes() and (state[rows * 248:] == SENT).all()
    # no block at all: the state still moves on
    state[:rows * 248] = 0
    assert pkg.lib().mi_pcm_plan_host(C.byref(cfg), ptr(en), rows, nb, ptr(wave), wave.shape[1], None, 0, ptr(state), None) == 0
    assert state[:rows * 248].tobytes() == after.tobytes()
    none, model_state = pcm_model(wave, index[:0], rate=rate, fmt=fmt)
    assert none.shape == (0, bb) and model_state.tobytes() == after.tobytes()


# ---------------- a foreign index: entries no gate writes, more of them than the call's grid ----------------

GUARD = 2  # blocks behind the capacity that must keep the sentinel


def test_foreign_index_is_what_it_is_built_for():
    """the properties on the index alone, at the shape the builder is drawn for and at each of the three cases; the three row
    slices; and that the zero entries of kinds B and D point at audio: with the input laid out for the handle's batches, a stage
    that took them for entries of the call would encode FOREIGN_FILL, not fault and not write zeros"""
    rows, nb, mb = pm.FOREIGN_SHAPE
    index, count, row_first = pm.foreign_index(rows, nb, mb)
    assert index.shape == (20, 2) and index.dtype == np.uint32 and count.tolist() == [20, 20] and row_first.tolist() == [5, 2, 21, 22]
    kinds = pm.assert_foreign_properties(index, row_first, rows, nb, mb, 20, grid=rows * nb)
    assert kinds == "VCVVBV" "ABVDVC" "VVDAVV" "DV"
    for name in pm.FOREIGN_CASES:
        index, count, row_first, cap, stored = pm.foreign_case(name)
        assert (len(index), count.tolist(), cap, stored) == {"20 entries": (20, [20, 20], 24, 20), "capacity 13": (20, [20, 20], 13, 13),
                                                            "count 40": (24, [40, 40], 24, 24)}[name]
        # entries k, k + 6, k + 12, k + 18 of a grid of 6 go to one workgroup: workgroup 0 makes the most trips
        assert [len(range(g, stored, 6)) for g in range(6)] == {20: [4, 4, 3, 3, 3, 3], 13: [3, 2, 2, 2, 2, 2], 24: [4] * 6}[stored]
    wave = pm.foreign_wave(audio("noise", rows, nb), nb, mb)
    assert wave.shape == (rows, mb * WAVE_BATCH) and (wave[:, nb * WAVE_BATCH:] == pm.FOREIGN_FILL).all()
    index = pm.foreign_index(rows, nb, mb, 24)[0]
    kinds = pm.foreign_kinds(index, rows, nb, mb)
    for rate, fmt in CONFIGS:
        as_call, _ = pcm_model(wave, index, rate=rate, fmt=fmt, nbatches=nb)
        as_handle, _ = pcm_model(wave, index, rate=rate, fmt=fmt, nbatches=mb)
        for k, kind in enumerate(kinds):
            assert as_call[k].any() == (kind == "V"), (k, kind)
            assert as_handle[k].any() == (kind in "VBD"), (k, kind)


@pytest.mark.parametrize("rate,fmt", CONFIGS)
@pytest.mark.parametrize("case", pm.FOREIGN_CASES)
def test_twin_equals_model_on_the_foreign_index(pkg, case, rate, fmt):
    """Two calls of 2 batches over buffers laid out for 8, fresh and then from the first call's tails, through the C entry point into
    a sentinel-filled destination with a guard behind the capacity: exactly min(count[1], max_blocks) blocks are written, the zero
    entries are zero blocks, the entry that occurs twice has the same bytes twice, and batch 0 entries read the carried samples."""
    rows, nb, mb = pm.FOREIGN_SHAPE
    index, count, _, cap, stored = pm.foreign_case(case)
    kinds = pm.foreign_kinds(index[:stored], rows, nb, mb)
    bb = pm.block_bytes(rate, fmt)
    en, cfg = np.ones(rows, np.uint8), pkg.PcmCfg(rate, fmt)
    for name in ("voice", "noise"):
        long = audio(name, rows, 2 * nb)
        state = pm.fresh_state(rows)
        for call in range(2):
            wave = pm.foreign_wave(long[:, call * nb * WAVE_BATCH:], nb, mb)
            want, after = pcm_model(wave, index[:stored], state, rate=rate, fmt=fmt, nbatches=nb)
            out = np.full((cap + GUARD) * bb, SENT, np.uint8)
            blob = np.concatenate([state.view(np.uint8).reshape(-1), np.full(16, SENT, np.uint8)])
            n = pm.stored_blocks(count, cap)
            assert pkg.lib().mi_pcm_plan_host(C.byref(cfg), ptr(en), rows, nb, ptr(wave), wave.shape[1], ptr(index), n, ptr(blob), ptr(out)) == 0
            what = f"{case}, {name}, call {call}"
            assert out[:stored * bb].tobytes() == want.tobytes(), f"{what}: blocks"
            assert (out[stored * bb:] == SENT).all(), f"{what}: something was written behind block {stored}"
            assert blob[:rows * 248].tobytes() == after.tobytes() and (blob[rows * 248:] == SENT).all(), f"{what}: state"
            got = out[:stored * bb].reshape(stored, bb)
            assert [bool(b.any()) for b in got] == [k == "V" for k in kinds], what
            twice = [k for k in range(stored) if tuple(index[k]) == (2, 1)]
            assert len(twice) >= 2 and all(got[k].tobytes() == got[twice[0]].tobytes() for k in twice)
            if call and rate == 8000:  # the carried samples are in the bytes: the same entries from a fresh state differ at batch 0 alone
                fresh, _ = pcm_model(wave, index[:stored], None, rate=rate, fmt=fmt, nbatches=nb)
                differ = [k for k in range(stored) if fresh[k].tobytes() != want[k].tobytes()]
                assert differ == [k for k in range(stored) if kinds[k] == "V" and index[k][1] == 0] and any(k >= rows * nb for k in differ)
            state = after
        assert state["x"].tobytes() == long[:, -HISTORY:].tobytes()


# ---------------- the IMA encoder ----------------

def ima_blocks(pkg, name, rate, rows=2, nb=2):
    wave = audio(name, rows, nb)
    index = pm.full_index(rows, nb)
    blocks, _ = twin(pkg, wave, index, None, None, rate, IMA4)
    s16, _ = twin(pkg, wave, index, None, None, rate, S16)
    return blocks.reshape(-1, IMA_BYTES), s16.view("<i2").reshape(-1, IMA_SAMPLES)


@pytest.mark.parametrize("rate", [8000, 16000])
def test_ima4_equals_the_standard_library_encoder(pkg, rate):
    """audioop.lin2adpcm started from (s[0], index0) gives the same 24 codes for every sub-block, once its high-nibble-first packing is
    swapped"""
    audioop = pytest.importorskip("audioop")
    checked = 0
    for name in pm.BUILDERS:
        blocks, samples = ima_blocks(pkg, name, rate)
        for blk, s in zip(blocks, samples):
            assert int(blk[0]) | (int(blk[1]) << 8) == int(s[0]) & 0xFFFF and blk[3] == 0
            assert blk[2] == pm.ima_index0(s[:1], s[1:2])[0]
            codes, _ = audioop.lin2adpcm(s[1:].astype("<i2").tobytes(), 2, (int(s[0]), int(blk[2])))
            theirs = np.frombuffer(codes, np.uint8)
            assert len(theirs) == 12
            assert (((theirs >> 4) | (theirs << 4)) & 0xFF).astype(np.uint8).tobytes() == blk[4:].tobytes(), f"{name}: sub-block {checked}"
            checked += 1
    assert checked == len(pm.BUILDERS) * 2 * 2 * pm.samples_per_block(rate) // IMA_SAMPLES


@pytest.mark.parametrize("rate", [8000, 16000])
def test_ima4_decoder_keeps_step_with_the_encoder(pkg, rate):
    """the separately written decoder reproduces the model encoder's predictor after every sample, on the twin's bytes"""
    for name in pm.BUILDERS:
        blocks, samples = ima_blocks(pkg, name, rate)
        mine, preds, _, _ = pm.ima_encode(samples, trace=True)
        assert mine.tobytes() == blocks.tobytes()
        assert np.array_equal(pm.ima_decode(blocks), preds), name
        assert np.array_equal(pm.ima_decode(blocks)[:, 0], samples[:, 0])


def test_decode_snr_is_reported(pkg):
    """(a figure for DESIGN.md, nothing asserted about its value) the SNR of the decoded IMA4 blocks against the S16 samples"""
    for name in pm.TONE_BUILDERS + ("noise", "ramp"):
        for rate in (8000, 16000):
            blocks, samples = ima_blocks(pkg, name, rate, rows=5, nb=4)
            print(f"decode SNR, {name} at {rate}: {pm.snr_db(samples, pm.ima_decode(blocks)):.2f} dB")


# ---------------- the containers ----------------

@pytest.mark.parametrize("rate", [8000, 16000])
def test_s16_file_opens_with_the_wave_module(pkg, rate):
    wave = audio("voice", 1, 3)
    blocks, _ = twin(pkg, wave, pm.full_index(1, 3), None, None, rate, S16)
    header = pkg.pcm_wav_header(len(blocks), rate, S16)
    assert len(header) == 44
    with wavefile.open(io.BytesIO(header + blocks.tobytes()), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, rate, 3 * pm.samples_per_block(rate))
        assert f.readframes(f.getnframes()) == blocks.tobytes()


@pytest.mark.parametrize("rate", [8000, 16000])
def test_ima4_file_fields_and_decode(pkg, rate):
    wave = audio("voice", 1, 3)
    blocks, _ = twin(pkg, wave, pm.full_index(1, 3), None, None, rate, IMA4)
    s16, _ = twin(pkg, wave, pm.full_index(1, 3), None, None, rate, S16)
    header = pkg.pcm_wav_header(len(blocks), rate, IMA4)
    data = header + blocks.tobytes()
    assert len(header) == 60
    riff, size, wav, fmt_id, fmt_len = struct.unpack_from("<4sI4s4sI", data, 0)
    assert (riff, size, wav, fmt_id, fmt_len) == (b"RIFF", len(data) - 8, b"WAVE", b"fmt ", 20)
    tag, channels, srate, avg, align, bits, cb, spb = struct.unpack_from("<HHIIHHHH", data, 20)
    assert (tag, channels, srate, avg, align, bits, cb, spb) == (0x0011, 1, rate, rate * 16 // 25, 16, 4, 2, 25)
    fact, fact_len, nsamples, did, dlen = struct.unpack_from("<4sII4sI", data, 40)
    assert (fact, fact_len, nsamples, did, dlen) == (b"fact", 4, 3 * pm.samples_per_block(rate), b"data", blocks.size)
    body = np.frombuffer(data[60:], np.uint8).reshape(-1, align)
    decoded = pm.ima_decode(body).reshape(-1)
    assert len(decoded) == nsamples
    want = s16.view("<i2").reshape(-1)
    assert np.array_equal(decoded[::IMA_SAMPLES], want[::IMA_SAMPLES]) and pm.snr_db(want, decoded) > 0


# ---------------- sizes, symbols, refusals ----------------

def test_sizes_and_symbols(pkg):
    assert [pkg.pcm_block_bytes(r, f) for r, f in CONFIGS] == [2000, 640, 4000, 1280]
    assert pkg.pcm_block_bytes() == 2000 and pkg.pcm_block_bytes(0, IMA4) == 640 and pkg.pcm_block_bytes(16000, 0) == 4000
    assert pkg.lib().mi_pcm_block_bytes(None) == 2000
    assert C.sizeof(pkg.PcmCfg) == 8 and pkg.PCM_STATE_DTYPE.itemsize == 248 and (pkg.PCM_S16, pkg.PCM_IMA4) == (S16, IMA4)
    header = open(os.path.join(ROOT, "include", "mi_airband.h")).read()
    assert "MI_PCM_STATE_ROW_BYTES = 248" in header and "MI_PCM_S16 = 1" in header and "MI_PCM_IMA4 = 2" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = {s for s in re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header) if s.startswith("mi_pcm")}
    assert declared == PCM_SYMBOLS and PCM_SYMBOLS <= set(pkg.ABI_SYMBOLS)
    assert all(hasattr(pkg.lib(), s) for s in PCM_SYMBOLS)


def test_refusals(pkg):
    L = pkg.lib()
    null = b"NULL argument"

    def refused(rc, code=INVALID, text=None):
        assert rc == code
        if text is not None:
            assert L.mi_last_error() == text

    out = C.c_void_p()
    en, some = np.ones(4, np.uint8), np.zeros(4096, np.uint8)
    good = pkg.PcmCfg(0, 0)
    refused(L.mi_pcm_create(C.byref(good), None, 4, 1, 0, 0, C.byref(out)), text=null)
    refused(L.mi_pcm_create(C.byref(good), ptr(en), 4, 1, 0, 0, None), text=null)
    rate_text = b"PCM stage: rate must be 8000 or 16000 (0 = 8000)"
    format_text = b"PCM stage: format must be MI_PCM_S16 or MI_PCM_IMA4 (0 = MI_PCM_S16)"
    bad_cfgs = [(pkg.PcmCfg(r, 0), rate_text) for r in (1, 7999, 8001, 11025, 44100, 0xFFFFFFFF)] + [(pkg.PcmCfg(0, f), format_text) for f in (3, 4, 0x11)]
    for cfg, text in bad_cfgs:  # (the argument alone decides: before a device is looked for)
        refused(L.mi_pcm_create(C.byref(cfg), ptr(en), 4, 1, 0, 0, C.byref(out)), text=text)
        assert L.mi_pcm_block_bytes(C.byref(cfg)) == 0
        n = C.c_size_t(0)
        refused(L.mi_pcm_wav_header(C.byref(cfg), 1, ptr(some), 64, C.byref(n)), text=text)
    geometry = b"PCM stage needs 1 <= rows < 2^20, max_batches >= 1 and rows * max_batches < 2^24"
    for rows, max_batches in ((0, 1), (-1, 1), (1 << 20, 1), (4, 0), (4, -1), (1 << 12, 1 << 12), ((1 << 20) - 1, 17)):
        refused(L.mi_pcm_create(None, ptr(en), rows, max_batches, 0, 0, C.byref(out)), text=geometry)
    assert not out.value
    if pkg.device_count() < 1:
        refused(L.mi_pcm_create(None, ptr(en), 4, 1, 0, 0, C.byref(out)), NO_DEVICE, b"no HIP device: the PCM stage runs on the GPU only")
        assert not out.value
        with pytest.raises(pkg.MiError) as e:
            pkg.Pcm(np.ones(3), max_batches=2)
        assert e.value.code == pkg.MI_ERR_NO_DEVICE
    # a NULL handle, before anything else
    refused(L.mi_pcm_set_rows(None, ptr(en)), text=null)
    refused(L.mi_pcm_process_device(None, ptr(some), 0, 1, ptr(some), ptr(some), ptr(some), None), text=null)
    refused(L.mi_pcm_download(None, None, ptr(some), ptr(some)), text=null)
    refused(L.mi_pcm_set_timing(None, 1), text=null)
    refused(L.mi_pcm_last_launch_ms(None, ptr(some)), text=null)
    refused(L.mi_pcm_get_state(None, ptr(some), 248), text=b"PCM stage state: NULL argument or wrong length")
    refused(L.mi_pcm_set_state(None, ptr(some), 248), text=b"PCM stage state: NULL argument or wrong length")
    assert L.mi_pcm_state_size(None) == 0
    L.mi_pcm_destroy(None)
    refused(L.mi_pcm_taps(None), text=null)
    # the twin
    rows, nb = 2, 2
    wave, index = np.zeros((rows, nb * WAVE_BATCH), np.float32), pm.full_index(rows, nb)
    state, blocks = np.zeros(rows * 248, np.uint8), np.zeros(rows * nb * 4000, np.uint8)

    def plan(**over):
        a = dict(cfg=None, en=ptr(en), rows=rows, nb=nb, wave=ptr(wave), row_stride=nb * WAVE_BATCH, index=ptr(index), n=len(index), state=ptr(state),
                 out=ptr(blocks))
        a.update(over)
        return L.mi_pcm_plan_host(*a.values())

    assert plan() == 0
    for name in ("en", "wave", "index", "state", "out"):
        refused(plan(**{name: None}), text=null)
    for cfg, text in bad_cfgs:
        refused(plan(cfg=C.byref(cfg)), text=text)
    for over in (dict(rows=0), dict(rows=-1), dict(nb=0), dict(nb=-1)):
        refused(plan(**over), text=b"pcm plan needs rows >= 1 and nbatches >= 1")
    refused(plan(row_stride=nb * WAVE_BATCH - 1), text=b"a row stride is shorter than the call")
    # the header
    n = C.c_size_t(0)
    ima = pkg.PcmCfg(0, IMA4)
    refused(L.mi_pcm_wav_header(None, 1, None, 64, C.byref(n)), text=null)
    refused(L.mi_pcm_wav_header(None, 1, ptr(some), 64, None), text=null)
    refused(L.mi_pcm_wav_header(None, 1, ptr(some), 43, C.byref(n)))
    refused(L.mi_pcm_wav_header(C.byref(ima), 1, ptr(some), 59, C.byref(n)))
    refused(L.mi_pcm_wav_header(None, (1 << 32) // 2000 + 1, ptr(some), 64, C.byref(n)))
    refused(L.mi_pcm_wav_header(C.byref(ima), (1 << 32) // 1000 + 1, ptr(some), 64, C.byref(n)))
    assert L.mi_pcm_wav_header(None, 0, ptr(some), 44, C.byref(n)) == 0 and n.value == 44
    assert L.mi_pcm_wav_header(C.byref(ima), (1 << 32) // 1000 - 1, ptr(some), 60, C.byref(n)) == 0 and n.value == 60
