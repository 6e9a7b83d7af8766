"""The mixer restatement (src/mixer.cpp:56-98, 133-140, 190-213).  mixer.cpp cannot be built here (it needs the
reference's umbrella header with lame / shout / libconfig), so parity is unpinned by the reference; the restatement is
checked against the arithmetic written out in numpy (mixer_model.py), operation for operation."""
import numpy as np
import pytest

import libs
from common import WAVE_BATCH
from mixer_model import INF_ROW, LISTS, LONE_BATCH, NO_SIGNAL, ROWS, SILENT_BATCH, assert_mix_conditions, case, mixer_planes, numpy_mixer


def test_mono_mixer_sums_in_input_order():
    wave, axc = case(1)
    inputs = [(0, 1.0, 0.0), (3, 0.5, 0.0), (1, 2.0, 0.0), (5, 0.0, 0.0)]
    l, r, out = libs.oracle_mixer(inputs, wave, axc, 5)
    el, er, eout = numpy_mixer(inputs, wave, axc, 5)
    assert r is None and er is None
    assert np.array_equal(l, el) and np.array_equal(out, eout)
    assert not l[3 * WAVE_BATCH:4 * WAVE_BATCH].any() and out[3] == ord(" ")


def test_stereo_mixer_balance():
    wave, axc = case(2)
    inputs = [(0, 1.0, -1.0), (2, 1.0, 1.0), (4, 0.7, 0.25), (1, 1.0, 0.0)]
    l, r, out = libs.oracle_mixer(inputs, wave, axc, 5)
    el, er, eout = numpy_mixer(inputs, wave, axc, 5)
    assert r is not None
    assert np.array_equal(l, el) and np.array_equal(r, er) and np.array_equal(out, eout)
    # balance -1: fully left (ampr = 0 -> skipped on the right); balance +1: fully right
    only0 = (axc[0] != ord(" ")) & (axc[2] == ord(" ")) & (axc[4] == ord(" ")) & (axc[1] == ord(" "))
    for b in np.nonzero(only0)[0]:
        sl = slice(b * WAVE_BATCH, (b + 1) * WAVE_BATCH)
        assert np.array_equal(l[sl], wave[0, sl]) and not r[sl].any()


@pytest.mark.parametrize("name", list(LISTS))
@pytest.mark.parametrize("nb,pad", [(6, 0), (6, 3), (1, 0), (2, 3)])
def test_oracle_reads_only_what_the_reference_copies(name, nb, pad):
    """mixer_planes: NaN in every NO_SIGNAL batch, in the row no input lists and behind the call, +Inf on a row whose multiplier is
    0.0f in one channel.  ao_mixer_run equals the numpy mixer byte for byte (NaN != NaN, so bytes), no NaN comes out, and Inf comes
    out of the one channel its row feeds: `mult == 0.0f` skipped the input, it did not multiply it."""
    wave, axc = mixer_planes(ROWS, nb, pad)
    assert np.isnan(wave[:, nb * WAVE_BATCH:]).all() and np.isnan(wave[ROWS - 1]).all() and (axc[ROWS - 1] != NO_SIGNAL).all()
    assert np.isinf(wave[INF_ROW, :WAVE_BATCH]).any() and {ord("<"), ord(">")} <= set(axc[:, :nb].reshape(-1).tolist())
    assert nb <= LONE_BATCH or ((axc[:ROWS - 1, LONE_BATCH] != NO_SIGNAL).sum() == 1 and (axc[:ROWS - 1, SILENT_BATCH] == NO_SIGNAL).all())
    inputs = LISTS[name]
    l, r, out = libs.oracle_mixer(inputs, wave, axc, nb)
    el, er, eout = numpy_mixer(inputs, wave, axc, nb)
    assert (r is None) == (er is None)
    assert l.tobytes() == el.tobytes() and out.tobytes() == eout.tobytes() and (r is None or r.tobytes() == er.tobytes())
    assert_mix_conditions(name, axc, nb, l, r, out)
