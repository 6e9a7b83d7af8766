"""The pager decoder stage without a GPU: the numpy restatement (pocsag_model.py) against what its modulator sends, and the host twin
mi_pocsag_plan_host against the restatement byte for byte -- bits, Q, messages, prefix, counts and the state blob."""
import functools
import itertools

import numpy as np
import pytest

import pocsag_model as m
from pocsag_model import GEOM, IDLE_WORD, MESSAGE, SYNC, WAVE_BATCH, fresh_state, pocsag_model

BAUDS = (512, 1200, 2400)


@functools.lru_cache(maxsize=None)
def builders(baud):
    """(names, plane float32 [rows][NBATCHES * 2000], [(address, function, text)] sent per row)"""
    rows = m.builder_rows(baud)
    plane = np.stack([r[1] for r in rows]).astype(np.float32)
    plane.setflags(write=False)
    return [r[0] for r in rows], plane, [r[2] for r in rows]


def cfg_kw(pkg, baud=1200, **kw):
    """the same settings for the twin (a PocsagCfg) and for the model (keywords)"""
    c = pkg.pocsag_cfg(baud=baud, sync_errors={0: pkg.POCSAG_SYNC_EXACT}.get(kw.get("sync_errors", 2), kw.get("sync_errors", 2)),
                       preamble_errors={None: pkg.POCSAG_PREAMBLE_OFF, 0: pkg.POCSAG_PREAMBLE_EXACT}.get(kw.get("preamble_errors", 4), kw.get("preamble_errors", 4)),
                       correct={0: pkg.POCSAG_CORRECT_NONE}.get(kw.get("correct", 1), kw.get("correct", 1)), hold_timing=kw.get("hold_timing", False))
    return c, dict(baud=baud, **kw)


def same(twin, want, what):
    assert twin[0].tobytes() == want[0].tobytes(), f"{what}: messages\n{twin[0][['row', 'batch', 'twelfth', 'address', 'nwords']]}\nwant\n{want[0][['row', 'batch', 'twelfth', 'address', 'nwords']]}"
    assert twin[1].tobytes() == want[1].tobytes() and twin[2].tobytes() == want[2].tobytes(), f"{what}: bits or Q"
    assert np.array_equal(twin[3], want[3]) and tuple(twin[4]) == (len(want[0]), len(want[0])) and twin[5].tobytes() == want[4].tobytes(), f"{what}: prefix, counts or state"


def both(pkg, plane, state=None, en=None, what="", **kw):
    """the model's answer, after the twin's was found equal to it"""
    c, mk = cfg_kw(pkg, **kw)
    plane = np.atleast_2d(np.asarray(plane, np.float32))
    want = pocsag_model(plane, state, en, **mk)
    same(pkg.pocsag_plan_host(np.ones(len(plane)) if en is None else en, plane, c, state), want, what)
    return want


@pytest.mark.parametrize("baud", BAUDS)
def test_the_model_and_the_twin_find_what_every_builder_sends(pkg, baud):
    names, plane, sent = builders(baud)
    msgs = both(pkg, plane, baud=baud, what=f"{baud} baud")[0]
    for r, name in enumerate(names):
        assert m.found(msgs, r) == sent[r], name
    assert all(pkg.pocsag_message_text(x) == m.text_of(x) for x in msgs)
    dc = names.index("a DC offset")  # slicer 1 decodes the offset that slicer 0 loses; no clean signal is lost the other way (|mu| < the level)
    assert m.found(pocsag_model(plane[dc:dc + 1], baud=baud, slicers=(0,))[0]) == [] and m.found(pocsag_model(plane[dc:dc + 1], baud=baud, slicers=(1,))[0]) == sent[dc]
    inv = msgs[msgs["row"] == names.index("inverted polarity")]
    assert (inv["inverted"] == 1).all() and (msgs[msgs["row"] != names.index("inverted polarity")]["inverted"] == 0).all()
    for s in (0, 1):
        assert m.found(pocsag_model(plane[:1], baud=baud, slicers=(s,))[0]) == sent[0], f"slicer {s} alone on the clean page"


def sync_cut_rows():
    """[2][6 * 2000] at 1200 baud, a preamble of 40 bits: SYNC's first bit begins at twelfth 24000, batch 1's first sample (the last
    preamble bit ends with batch 0); and SYNC's seventeenth bit begins there"""
    bits = m.transmission([(0x12345, 3, m.alpha_words(m.ALPHA_TEXT))], preamble=40)
    L = GEOM[1200][0]
    return np.stack([m.render(bits, m.TWELFTHS - 40 * L, 6 * WAVE_BATCH, 1200), m.render(bits, m.TWELFTHS - 56 * L, 6 * WAVE_BATCH, 1200)]).astype(np.float32)


@pytest.mark.parametrize("rows", [1, 5])
def test_every_way_of_cutting_the_batches_into_calls(pkg, rows):
    """1200 baud, the first 6 batches: every composition of 6 into calls.  Row 0 is a page whose SYNC begins with batch 1's first
    sample -- a cut behind batch 0 falls between preamble and SYNC --, row 1 one whose SYNC lies across that boundary; the other rows
    are the first builders, whose SYNC is over within batch 0, so that their cuts fall inside codewords.  The placement is asserted
    from the state behind batch 0 and behind batch 1."""
    plane = np.concatenate([sync_cut_rows(), builders(1200)[1][:3, :6 * WAVE_BATCH]])[:rows]
    after = pocsag_model(plane[:2, :WAVE_BATCH])[4]
    assert (after["phase"][:2] == m.IDLE).all() and (pocsag_model(plane[:2, WAVE_BATCH:2 * WAVE_BATCH], after)[4]["phase"][:2] == m.TRANSMISSION).all()
    whole = pocsag_model(plane)
    c = pkg.pocsag_cfg()
    for mask in range(32):
        cuts, run = [], 1
        for i in range(5):
            if mask >> i & 1:
                cuts.append(run)
                run = 1
            else:
                run += 1
        cuts.append(run)
        state, done, got = None, 0, []
        for n in cuts:
            part = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
            want = pocsag_model(part, state)
            same(pkg.pocsag_plan_host(np.ones(rows), part, c, state), want, f"cuts {cuts} at {done}")
            state, done = want[4], done + n
            got.append(want[0])
        got = np.concatenate(got)
        assert state.tobytes() == whole[4].tobytes() and sorted(m.found(got)) == sorted(m.found(whole[0])), cuts


@pytest.mark.parametrize("baud", BAUDS)
def test_every_start_residue_of_the_grid(pkg, baud):
    """A bit's L twelfths hold L / gcd(L, 12) distinct sample phases... the grid repeats after one step, so the starts 0 .. step - 1
    twelfths, and the step's multiples up to L, cover every residue class of a start against the hypotheses: step + H starts."""
    L, step, H, _, _ = GEOM[baud]
    starts = list(range(step)) + [step * t for t in range(1, H)]
    bits = m.transmission([(0x1F0F6, 2, [])], preamble=40)
    nb = {512: 12, 1200: 5, 2400: 3}[baud]
    plane = np.stack([m.render(bits, 3000 + s, nb * WAVE_BATCH, baud) for s in starts])
    msgs = both(pkg, plane, baud=baud, what="start residues")[0]
    assert [m.found(msgs, r) for r in range(len(starts))] == [[(0x1F0F6, 2, "")]] * len(starts)
    t = (msgs["batch"].astype(np.int64) * m.TWELFTHS + msgs["twelfth"]) - (3000 + np.array(starts) + (40 + 32 + 12 * 32) * L)
    assert np.abs(t).max() <= L // 2, "the address word's place is where the modulator put it, within half a bit"


DRIFT_BATCHES = 13


def drifting(tau, ppm):
    """1200 baud: the long page, its bits beginning on hypothesis tau's grid (twelfth 20 L + tau step), the clock off by ppm"""
    L, step, _, _, _ = GEOM[1200]
    bits = m.transmission([(0x12345, 3, m.alpha_words(m.LONG_TEXT))], preamble=40)
    return m.render(bits, 20 * L + tau * step, DRIFT_BATCHES * WAVE_BATCH, 1200, ppm=ppm)


def lane_sequences(pkg, plane, hold):
    """the rows' hypothesis behind every batch (None: idle), from calls of one batch each, twin against model; and the records"""
    H = GEOM[1200][2]
    state, seq, msgs = None, [[] for _ in plane], []
    for b in range(DRIFT_BATCHES):
        want = both(pkg, plane[:, b * WAVE_BATCH:(b + 1) * WAVE_BATCH], state=state, hold_timing=hold, what=f"batch {b}")
        state = want[4]
        msgs.append(want[0])
        for r in range(len(plane)):
            seq[r].append(int(state["lane"][r]) % H if state["phase"][r] == m.TRANSMISSION else None)
    return seq, np.concatenate(msgs)


def test_timing_moves_across_the_wrap_and_between_0_and_1(pkg):
    """Pages that begin on the grids of hypotheses 0, 2 and H - 1, the clock 400 ppm slow (the walker moves up) and fast (down), in
    calls of one batch: the rows of 0 and H - 1 open on those hypotheses; every move is one step; H - 1 -> 0, 0 -> H - 1 (in step),
    0 -> 1 (a slot passed over) and 1 -> 0 (a bit replayed) all occur; every page comes out whole"""
    H = GEOM[1200][2]
    cases = [(tau, ppm) for tau in (0, 2, H - 1) for ppm in (-400.0, 400.0)]
    plane = np.stack([drifting(tau, ppm) for tau, ppm in cases]).astype(np.float32)
    seq, msgs = lane_sequences(pkg, plane, False)
    moves = set()
    for (tau, ppm), q in zip(cases, seq):
        q = [t for t in q if t is not None]
        assert len(q) >= 10 and (tau == 2 or q[0] == tau), (tau, ppm, q)
        steps = {(a, b) for a, b in zip(q, q[1:]) if a != b}
        # one step a move; in the drift's direction on the rows that open where they lie (the row of 2 opens a slot early on hypothesis
        # 0, whose bit of a slot is the latest, and is first moved up to where it lies)
        assert all((b - a) % H in ((1, H - 1) if tau == 2 else (1,) if ppm < 0 else (H - 1,)) for a, b in steps), (tau, ppm, q)
        moves |= steps
    assert {(H - 1, 0), (0, H - 1), (0, 1), (1, 0)} <= moves, moves
    assert all(m.found(msgs, r) == [(0x12345, 3, m.LONG_TEXT)] for r in range(len(cases))), m.found(msgs)
    assert all((int(x["lane_sync"]) - int(x["lane_end"])) % H != 0 for x in msgs)


def test_hold_timing_keeps_the_hypothesis(pkg):
    """the same rows with hold_timing: the hypothesis behind every batch of a transmission is the one the sync chose"""
    H = GEOM[1200][2]
    plane = np.stack([drifting(tau, ppm) for tau in (0, 2, H - 1) for ppm in (-400.0, 400.0)]).astype(np.float32)
    seq, msgs = lane_sequences(pkg, plane, True)
    for q in seq:
        q = [t for t in q if t is not None]
        assert len(q) >= 5 and len(set(q)) == 1, q
    assert (msgs["lane_sync"] == msgs["lane_end"]).all()


def flipped(bits, places):
    bits = list(bits)
    for p in places:
        bits[p] ^= 1
    return bits


def test_sync_and_preamble_errors_on_both_sides_of_their_bounds(pkg):
    page = [(0x1F0F6, 2, [])]
    bits = m.transmission(page, preamble=40)
    row = lambda b: m.render(b, 4321, 4 * WAVE_BATCH, 1200)  # noqa: E731
    sync2, sync3 = flipped(bits, [41, 50]), flipped(bits, [41, 50, 60])
    pre4, pre5 = flipped(bits, [10, 14, 20, 30]), flipped(bits, [10, 14, 20, 30, 36])
    want = [(0x1F0F6, 2, "")]
    assert m.found(both(pkg, row(sync2))[0]) == want and m.found(both(pkg, row(sync3))[0]) == []
    assert m.found(both(pkg, row(sync3), sync_errors=3)[0]) == want and m.found(both(pkg, row(flipped(bits, [41])), sync_errors=0)[0]) == []
    assert m.found(both(pkg, row(bits), sync_errors=0, preamble_errors=0)[0]) == want
    assert m.found(both(pkg, row(pre4))[0]) == want and m.found(both(pkg, row(pre5))[0]) == [] and m.found(both(pkg, row(pre5), preamble_errors=5)[0]) == want
    assert m.found(both(pkg, row(flipped(bits, [20])), preamble_errors=0)[0]) == [] and m.found(both(pkg, row(pre5), preamble_errors=None)[0]) == want


def test_joining_at_the_second_group_and_a_failed_sync_behind_word_15(pkg):
    """no preamble before the second group's SYNC: only MI_POCSAG_PREAMBLE_OFF opens there.  A second SYNC with five flips ends the
    transmission: the open message closes with the words it has."""
    long_page = [(0x1555D, 3, m.alpha_words(m.LONG_TEXT))]
    bits = m.transmission(long_page, preamble=40)
    second = 40 + 17 * 32  # the second group's SYNC
    two = m.transmission([(0x12346, 3, m.alpha_words(m.ALPHA_TEXT)), (0x1F0F6, 2, [])], preamble=40)  # the first page ends in the second group, the tone is in it
    late = m.render(two[second - 20:], 4000, 8 * WAVE_BATCH, 1200)
    assert m.found(both(pkg, late)[0]) == []
    got = both(pkg, late, preamble_errors=None)[0]
    assert m.found(got) == [(0x1F0F6, 2, "")], "the first page's words behind the SYNC belong to no open message and are dropped; the tone page is found"
    cut = both(pkg, m.render(flipped(bits, [second + 1, second + 5, second + 9, second + 13, second + 17]), 4000, 8 * WAVE_BATCH, 1200))[0]
    assert len(cut) == 1 and cut[0]["address"] == 0x1555D and cut[0]["nwords"] == 5 and m.LONG_TEXT.startswith(m.text_of(cut[0])[:12])


def test_encode_and_decode_on_every_single_double_and_triple_flip(pkg):
    assert pkg.pocsag_encode(SYNC >> 11) == SYNC and pkg.pocsag_encode(IDLE_WORD >> 11) == IDLE_WORD
    word = m.message_word(0xA5C3F)
    assert pkg.pocsag_encode(word >> 11) == word == m.codeword(word >> 11)
    none = pkg.POCSAG_CORRECT_NONE
    assert pkg.pocsag_decode(word, none) == (True, word, 0) == pkg.pocsag_decode(word, 2)
    for a in range(32):
        w1 = word ^ 1 << a
        assert pkg.pocsag_decode(w1, none)[0] is False and pkg.pocsag_decode(w1, 1) == (True, word, 1) == pkg.pocsag_decode(w1, 2)
        assert pkg.pocsag_decode(w1, 0) == (True, word, 1), "0 is the default, 1"
    for a, b in itertools.combinations(range(32), 2):
        w2 = word ^ 1 << a ^ 1 << b
        assert pkg.pocsag_decode(w2, none)[0] is False and pkg.pocsag_decode(w2, 1) == (False, w2, 2) and pkg.pocsag_decode(w2, 2) == (True, word, 2), (a, b)
        assert m.decode(w2, 1) == (False, w2, 2) and m.decode(w2, 2) == (True, word, 2)
    accepted2 = 0
    for a, b, c in itertools.combinations(range(32), 3):  # 4960: distance 6 leaves a triple at least three from any other codeword
        w3 = word ^ 1 << a ^ 1 << b ^ 1 << c
        good, stored, e = pkg.pocsag_decode(w3, 1)
        assert not good and stored == w3 and (good, stored, e) == m.decode(w3, 1), (a, b, c)
        accepted2 += pkg.pocsag_decode(w3, 2)[0]
    assert accepted2 == 0, "three flips are at least three from every codeword: not good at 2 either"
    with pytest.raises(pkg.MiError):
        pkg.pocsag_decode(word, 3)


def test_a_bad_word_a_message_word_with_none_open_and_the_cut_at_80_words(pkg):
    alpha = m.alpha_words(m.ALPHA_TEXT)
    bits = m.transmission([(0x12345, 3, alpha)], preamble=40)
    first = 40 + 32 + 11 * 32  # the first message word (the address is word 10)
    bad = both(pkg, m.render(flipped(bits, [first + 33, first + 40, first + 47]), 4000, 9 * WAVE_BATCH, 1200))[0]
    assert len(bad) == 1 and bad[0]["nbad"] == 1 and bad[0]["bad"][0] == 2 and bad[0]["nwords"] == len(alpha) and "?" in m.text_of(bad[0])
    assert pkg.pocsag_message_text(bad[0]) == m.text_of(bad[0]) and all(a in (b, "?") for a, b in zip(m.text_of(bad[0]), m.ALPHA_TEXT))
    one = both(pkg, m.render(flipped(bits, [first + 33]), 4000, 9 * WAVE_BATCH, 1200))[0]
    assert m.found(one) == [(0x12345, 3, m.ALPHA_TEXT)] and one[0]["corrected"] == 1 and one[0]["nbad"] == 0
    # the address word made bad: its message words find none open and are dropped
    lost = both(pkg, m.render(flipped(bits, [first - 30, first - 20, first - 10]), 4000, 9 * WAVE_BATCH, 1200))[0]
    assert len(lost) == 0
    words = [m.message_word(i) for i in range(85)]
    cut = both(pkg, m.render(m.transmission([(0x8, 1, words)], preamble=40), 4000, 24 * WAVE_BATCH, 1200))[0]
    assert len(cut) == 1 and cut[0]["nwords"] == 80 and cut[0]["truncated"] == 1 and list(cut[0]["words"]) == words[:80]


def test_sixteen_bad_words_end_a_transmission(pkg):
    bits = m.transmission([(0x12340, 3, m.alpha_words(m.LONG_TEXT))], preamble=40)
    g2 = 40 + 17 * 32 + 32  # the second group's word 0
    noisy = list(bits)
    rng = np.random.default_rng(3)
    for wd in range(16):
        for p in rng.choice(32, 5, replace=False):
            noisy[g2 + 32 * wd + p] ^= 1
    want = both(pkg, m.render(noisy, 4000, 9 * WAVE_BATCH, 1200))
    msg = want[0]
    assert len(msg) == 1 and msg[0]["nwords"] >= 15 + 16 - 1 and msg[0]["nbad"] >= 14 and want[4]["phase"][0] == m.IDLE


def capacity_case(nb, baud=1200):
    """(state, plane [1][nb * 2000]): a row inside a group of sixteen address words, the second of which ends in slot 0 of the call"""
    L, step, H, B, _ = GEOM[baud]
    bits = m.bits_of_words([m.address_word(8 * (100 + c) + c // 2, c % 4) for c in range(16)] + [IDLE_WORD] * 16, 40)
    k = 40 + 32 + 63  # the last bit of the group's second word
    lead = 4
    start = lead * m.TWELFTHS - L // 2 - k * L
    x = m.render(bits, start, (lead + nb) * WAVE_BATCH, baud).astype(np.float32)[None]
    st = pocsag_model(x[:, :lead * WAVE_BATCH], baud=baud)[4]
    return st, x[:, lead * WAVE_BATCH:]


@pytest.mark.parametrize("nb", [1, 2])
def test_the_capacity_bound_is_reached(pkg, nb):
    st, plane = capacity_case(nb)
    msgs = both(pkg, plane, state=st, what=f"capacity {nb}")[0]
    assert len(msgs) == pkg.pocsag_max_messages(nb) == m.max_messages(nb) == (5, 10)[nb - 1] and (msgs["nwords"] == 0).all()
    assert pkg.lib().mi_pocsag_max_messages(1200, nb) == len(msgs) and pkg.lib().mi_pocsag_max_messages(512, 1) == 3 and pkg.lib().mi_pocsag_max_messages(7, 1) == 0


def test_a_disabled_row_padded_strides_and_capped_outputs(pkg):
    names, plane, _ = builders(2400)
    rows, nb = 4, 4
    en = np.array([1, 0, 1, 1], np.uint8)
    st = fresh_state(rows)
    st["x"][:] = np.random.default_rng(2).normal(0, 0.1, (rows, 34)).astype(np.float32)
    part = plane[:rows, :nb * WAVE_BATCH]
    want = pocsag_model(part, st, en, baud=2400)
    assert want[4][1].tobytes() == st[1].tobytes() and len(want[0]) == 3 and not want[1][1].any()
    wide = np.full((rows, (nb + 2) * WAVE_BATCH + 4), np.float32(0.25))
    wide[:, :nb * WAVE_BATCH] = part
    c = pkg.pocsag_cfg(baud=2400)
    same(pkg.pocsag_plan_host(en, wide, c, st, nbatches=nb), want, "padded stride")
    L = pkg.lib()
    msgs = np.full(5, 0xA5, np.uint8).repeat(MESSAGE.itemsize).view(MESSAGE)
    first, count, blob = np.zeros(rows + 1, np.uint32), np.zeros(2, np.uint32), st.copy()
    import ctypes as C
    assert L.mi_pocsag_plan_host(C.byref(c), en.ctypes.data, rows, nb, wide.ctypes.data, wide.shape[1], blob.ctypes.data, None, None, msgs.ctypes.data, 2,
                                 first.ctypes.data, count.ctypes.data) == pkg.MI_OK
    assert tuple(count) == (3, 2) and msgs[:2].tobytes() == want[0][:2].tobytes() and (msgs[2:].view(np.uint8) == 0xA5).all() and blob.tobytes() == want[4].tobytes()


def test_the_text_helper_in_its_three_modes(pkg):
    msg = np.zeros((), MESSAGE)
    words = m.numeric_words(m.NUMERIC_TEXT)
    msg["nwords"], msg["words"][:len(words)], msg["function"] = len(words), words, 0
    assert pkg.pocsag_message_text(msg) == m.NUMERIC_TEXT == pkg.pocsag_message_text(msg, pkg.POCSAG_TEXT_NUMERIC) == m.text_of(msg)
    assert pkg.pocsag_message_text(msg, pkg.POCSAG_TEXT_ALPHA) == m.text_of(msg, "alpha")
    words = m.alpha_words("Ward 7\x07 bed 12~")
    msg = np.zeros((), MESSAGE)
    msg["nwords"], msg["words"][:len(words)], msg["function"] = len(words), words, 3
    assert pkg.pocsag_message_text(msg) == "Ward 7. bed 12~" == m.text_of(msg) and pkg.pocsag_message_text(msg, pkg.POCSAG_TEXT_NUMERIC) == m.text_of(msg, "numeric")
    msg["bad"][0] = 1 << 1
    assert pkg.pocsag_message_text(msg) == "Wa???7. bed 12~"[:2] + m.text_of(msg)[2:] and m.text_of(msg).count("?") == 4
    empty = np.zeros((), MESSAGE)
    assert pkg.pocsag_message_text(empty) == "" == pkg.pocsag_message_text(empty, pkg.POCSAG_TEXT_ALPHA)


@pytest.mark.parametrize("baud", BAUDS)
def test_ten_minutes_of_noise_and_of_voice_give_no_record(pkg, baud):
    """4800 batches of seeded white noise and of the voice builder through the twin at the defaults, in calls of 600 batches"""
    nb, call = 4800, 600
    for name, x in (("noise", m.noise(nb * WAVE_BATCH, 0.2, 1234 + baud)), ("voice", m.voice_like(nb * WAVE_BATCH, 77 + baud))):
        x = x.astype(np.float32)[None]
        state, total = None, 0
        for b in range(0, nb, call):
            got = pkg.pocsag_plan_host([1], x[:, b * WAVE_BATCH:(b + call) * WAVE_BATCH], pkg.pocsag_cfg(baud=baud), state)
            state, total = got[5], total + int(got[4][0])
        assert total == 0, f"{name} at {baud} baud: {total} records"
    # the model itself over the first half minute of the noise: equal to the twin, so what the twin found is what the model finds
    both(pkg, m.noise(240 * WAVE_BATCH, 0.2, 1234 + baud), baud=baud, what="noise")
