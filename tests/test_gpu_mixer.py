"""The mixer on the GPU (mi_mixer_*, csrc/mixer.hip) against the oracle's ao_mixer_run over the planes and input lists of mixer_model.py.

Every comparison is of bytes.  The planes hold NaN wherever the reference copies nothing -- NO_SIGNAL batches of a listed row, a row no
input lists, the padding behind the call -- and +Inf on a row whose multiplier is 0.0f in one channel, so a kernel that reads or
multiplies what it should skip puts a NaN into its output.  Every destination is 16 floats (8 flags) longer than the call and holds a
sentinel beforehand; a mono mixer is handed a right-channel buffer, which it must leave alone."""
import functools

import numpy as np
import pytest

import libs
from mixer_model import LISTS, ROWS, WAVE_BATCH, assert_mix_conditions, mixer_planes

gpu = pytest.mark.gpu
SENT_BYTE = 0xA5
SENT32 = int(np.uint32(0xA5A5A5A5).view(np.int32))
GUARD_FLOATS, GUARD_FLAGS = 16, 8
NB = [1, 2, 65, 129]  # 500, 1000, 32500 and 64500 four-sample groups: each ends inside a 256-thread workgroup
PAD = [0, 3]


@functools.lru_cache(maxsize=None)
def planes(nb, pad):
    wave, axc = mixer_planes(ROWS, nb, pad)
    wave.setflags(write=False)
    axc.setflags(write=False)
    return wave, axc


@functools.lru_cache(maxsize=None)
def expected(name, nb, pad):
    """ao_mixer_run's bytes, computed once per case, with the conditions the planes are built for checked on them"""
    wave, axc = planes(nb, pad)
    left, right, out = libs.oracle_mixer(LISTS[name], wave, axc, nb)
    assert_mix_conditions(name, axc, nb, left, right, out)
    return left.tobytes(), None if right is None else right.tobytes(), out.tobytes()


class Dest:
    """left, right and flags for a call of nb batches, the guard behind each, all holding the sentinel"""

    def __init__(self, nb):
        import torch
        self.nb = nb
        self.left = torch.full((nb * WAVE_BATCH + GUARD_FLOATS,), SENT32, dtype=torch.int32, device="cuda")
        self.right = torch.full((nb * WAVE_BATCH + GUARD_FLOATS,), SENT32, dtype=torch.int32, device="cuda")
        self.out = torch.full((nb + GUARD_FLAGS,), SENT_BYTE, dtype=torch.uint8, device="cuda")

    def check(self, what, want_left, want_right, want_out):
        n = self.nb * WAVE_BATCH * 4
        left, right, out = (t.cpu().numpy().view(np.uint8) for t in (self.left, self.right, self.out))
        assert (left[n:] == SENT_BYTE).all() and (right[n:] == SENT_BYTE).all() and (out[self.nb:] == SENT_BYTE).all(), f"{what}: written behind the call"
        assert out[:self.nb].tobytes() == want_out, f"{what}: axc_out {bytes(out[:self.nb])} vs {want_out}"
        assert left[:n].tobytes() == want_left, f"{what}: left differs in {diff(left[:n], want_left)}"
        if want_right is None:
            assert (right == SENT_BYTE).all(), f"{what}: a mono mixer wrote its right channel"
        else:
            assert right[:n].tobytes() == want_right, f"{what}: right differs in {diff(right[:n], want_right)}"


def diff(got, want):
    bad = np.flatnonzero(got.view(np.uint32) != np.frombuffer(want, np.uint32))
    return f"{len(bad)} samples, the first at {bad[:4]}: {got.view(np.float32)[bad[:4]]} vs {np.frombuffer(want, np.float32)[bad[:4]]}"


def upload(wave, axc):
    import torch
    return torch.from_numpy(wave.copy()).cuda(), torch.from_numpy(axc.copy()).cuda()


def mix(m, name, nb, pad, stream=None):
    """one call of m over planes(nb, pad) into fresh destinations, compared with the oracle"""
    import torch
    wave, axc = planes(nb, pad)
    if stream is None:
        d_wave, d_axc = upload(wave, axc)
        dest = Dest(nb)
        s = torch.cuda.current_stream().cuda_stream
    else:  # uploads, sentinel fills and the mixer behind one another on the side stream, nothing waited for in between
        with torch.cuda.stream(stream):
            d_wave, d_axc = upload(wave, axc)
            dest = Dest(nb)
        s = stream.cuda_stream
    m.process_device(d_wave.data_ptr(), wave.shape[1], d_axc.data_ptr(), axc.shape[1], nb, dest.left.data_ptr(), dest.right.data_ptr(),
                     dest.out.data_ptr(), hip_stream=s)
    torch.cuda.synchronize()
    dest.check(f"{name}, {nb} batches, pad {pad}", *expected(name, nb, pad))


@gpu
@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("pad", PAD)
@pytest.mark.parametrize("nb", NB)
def test_device_equals_oracle(pkg, nb, pad, name):
    """left, right and axc_out equal ao_mixer_run byte for byte; nothing is written behind the call; a mono mixer leaves d_right alone"""
    m = pkg.Mixer(LISTS[name])
    assert m.stereo == name.startswith("stereo")
    mix(m, name, nb, pad)
    m.close()


@gpu
@pytest.mark.parametrize("name", ["mono9", "stereo_inf_left"])
def test_enqueued_on_a_side_stream_behind_the_uploads(pkg, name):
    import torch
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    m = pkg.Mixer(LISTS[name])
    mix(m, name, 65, 3, stream=side)
    m.close()


@gpu
@pytest.mark.parametrize("name", ["mono9", "stereo_inf_right"])
def test_two_calls_of_different_length_on_one_handle(pkg, name):
    m = pkg.Mixer(LISTS[name])
    mix(m, name, 65, 0)
    mix(m, name, 2, 3)
    mix(m, name, 129, 3)
    m.close()


@gpu
def test_argument_errors(pkg):
    """what mi_mixer_process_device refuses, a stride shorter than the call among it -- in the words of every other post-stage"""
    import torch
    nb = 2
    wave, axc = planes(nb, 0)
    d_wave, d_axc = upload(wave, axc)
    dest = Dest(nb)
    s = torch.cuda.current_stream().cuda_stream
    stereo, mono = pkg.Mixer(LISTS["stereo_inf_left"]), pkg.Mixer(LISTS["mono1"])

    def call(m, nbatches=nb, row_stride=nb * WAVE_BATCH, axc_stride=nb, d_left=dest.left.data_ptr(), d_right=dest.right.data_ptr()):
        m.process_device(d_wave.data_ptr(), row_stride, d_axc.data_ptr(), axc_stride, nbatches, d_left, d_right, dest.out.data_ptr(), hip_stream=s)

    for bad, words in ((dict(row_stride=nb * WAVE_BATCH - 4), "a row stride is shorter than the call"),
                       (dict(row_stride=WAVE_BATCH), "a row stride is shorter than the call"),
                       (dict(axc_stride=nb - 1), "a row stride is shorter than the call"),
                       (dict(axc_stride=0), "a row stride is shorter than the call"),
                       (dict(d_left=dest.left.data_ptr() + 4), "16-byte aligned"),
                       (dict(d_right=dest.right.data_ptr() + 8), "16-byte aligned"),
                       (dict(row_stride=nb * WAVE_BATCH + 2), "multiple of 4 floats"),
                       (dict(nbatches=0), "NULL argument"),
                       (dict(nbatches=-1), "NULL argument")):
        for m in (stereo, mono):
            with pytest.raises(pkg.MiError) as e:
                call(m, **bad)
            assert e.value.code == pkg.MI_ERR_INVALID and words in str(e.value), (bad, str(e.value))
    with pytest.raises(pkg.MiError) as e:
        call(stereo, d_right=None)
    assert e.value.code == pkg.MI_ERR_INVALID and "stereo mixer needs a right-channel buffer" in str(e.value)
    torch.cuda.synchronize()
    dest.check("after the refusals", bytes([SENT_BYTE]) * (nb * WAVE_BATCH * 4), None, bytes([SENT_BYTE]) * nb)  # nothing ran
    call(mono, d_right=None)  # a mono mixer needs none
    call(stereo, row_stride=nb * WAVE_BATCH, axc_stride=nb)  # exactly the call's size is enough
    torch.cuda.synchronize()
    dest.check("tight strides", *expected("stereo_inf_left", nb, 0))
    stereo.close()
    mono.close()
