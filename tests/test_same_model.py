"""The SAME stage's host twin mi_same_plan_host against the numpy restatement in same_model.py, as bytes in bits, Q, messages and
state; the templates, the text helper, the hypothesis choice; and the conditions the defaults rest on.  No GPU."""
import numpy as np
import pytest

from same_model import (BATCH_UNITS, BURST, EOM, HEADER, HEADER_TEXT, LONGEST, MSG_REC, NB, NTAU, STATE, SYNC, UNITS, WAVE_BATCH, builders, fields_ok,
                        fresh_state, message_fields, mismatch, modulate, pick, same_model, templates, timing_cases, train, voice_like, START_CFG, start_unit_rows,
                        tie_cases, tie_start_unit)


def same(what, twin, want):
    """twin: same_plan_host's tuple; want: same_model's"""
    assert twin[1].tobytes() == want[1].tobytes(), f"{what}: bits, first at {np.argwhere(twin[1] != want[1])[:3]}"
    assert twin[2].tobytes() == want[2].tobytes(), f"{what}: Q"
    assert twin[0].tobytes() == want[0].tobytes(), f"{what}: messages\n{twin[0]}\nwant\n{want[0]}"
    assert np.array_equal(twin[3], want[3]) and int(twin[4][0]) == len(want[0]), f"{what}: prefix and count"
    assert twin[5].tobytes() == want[4].tobytes(), f"{what}: state"


def check_expected(names, msgs, expect):
    for r, name in enumerate(names):
        got = [(int(m["kind"]), int(m["nbursts"]), int(m["voted"]), int(m["truncated"]), bytes(m["bytes"][:m["nbytes"]])) for m in msgs[msgs["row"] == r]]
        assert got == expect[name], f"{name}: {got}"


def test_every_builder_decodes_what_was_sent_and_the_twin_equals_the_model(pkg):
    """one call over all rows: what each row's modulator sent is what the model finds -- on the clean rows with agree == nbytes and
    fields_ok -- and the twin gives the same bytes"""
    names, plane, expect = builders()
    want = same_model(plane)
    same("all rows", pkg.same_plan_host(np.ones(len(names)), plane), want)
    check_expected(names, want[0], expect)
    for m in want[0]:
        name = names[m["row"]]
        if "errors" not in name and "cut off" not in name:
            assert m["agree"] == m["nbytes"] and m["fields_ok"] == 1, name
    voted = want[0][want[0]["row"] == names.index("12 bit errors in one burst of three")]
    assert voted["agree"][0] < voted["nbytes"][0] and voted["fields_ok"][0] == 1, "the vote repairs the burst with 12 bit errors"
    assert (want[4]["grid"] == (BATCH_UNITS * NB) % UNITS).all() and (want[4]["batch"] == NB).all()


@pytest.mark.parametrize("rows,cuts", [(1, (NB,)), (5, (5, NB - 5)), (None, (5, NB - 5)), (None, (1,) * NB)])
def test_calls_cut_three_ways_over_more_than_a_grid_period(pkg, rows, cuts):
    """one call at 1 row, 5 + the rest at 5 rows and on every builder, and single batches on every builder, over 64 batches (the grid
    repeats after 48): the same messages into the same state as the one call over all rows, the twin equal to the model call by call"""
    names, plane, expect = builders()
    plane = plane[:rows] if rows else plane
    rows = plane.shape[0]
    whole = same_model(plane)
    state, done, msgs = fresh_state(rows), 0, []
    for n in cuts:
        part = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = same_model(part, state)
        same(f"cut {cuts[:2]} at {done}", pkg.same_plan_host(np.ones(rows), part, state=state), want)
        state, done = want[4], done + n
        msgs.append(want[0])
    msgs = np.concatenate(msgs)
    strip = lambda a: sorted((int(m["row"]), int(m["batch"]), int(m["unit"]), int(m["nbursts"]), bytes(m["bytes"])) for m in a)  # noqa: E731
    assert strip(msgs) == strip(whole[0]) and len(msgs) >= rows // 2 and state.tobytes() == whole[4].tobytes()
    check_expected(names[:rows], msgs, expect)


def check_start_units(msgs):
    """every row's one burst came out as sent, from a start within a hypothesis step and a bit of where the modulator put its 'Z'"""
    assert len(msgs) == 48 and list(msgs["row"]) == list(range(48))
    for s, m in enumerate(msgs):
        assert bytes(m["bytes"][:m["nbytes"]]) == HEADER_TEXT and (m["nbursts"], m["voted"], m["truncated"], m["fields_ok"]) == (1, 0, 0, 1), s
        sent = 48 * 41 + s + 128 * UNITS  # behind the 16 bytes of preamble
        assert m["agree"] == m["nbytes"] and abs(int(m["batch"]) * BATCH_UNITS + int(m["unit"]) - sent) <= UNITS // 2, (s, m["batch"], m["unit"], sent)


@pytest.mark.parametrize("cuts", [(10,), (3, 7), (1,) * 10])
def test_a_burst_at_every_start_unit_modulo_48(pkg, cuts):
    """48 rows, row s beginning its one burst at unit 48 * 41 + s: the twin equals the model as bytes call by call, and every row's
    header comes out as sent"""
    plane = start_unit_rows()
    state, done, msgs = fresh_state(48), 0, []
    for n in cuts:
        part = plane[:, done * WAVE_BATCH:(done + n) * WAVE_BATCH]
        want = same_model(part, state, **START_CFG)
        same(f"start units, cut {cuts[:2]} at {done}", pkg.same_plan_host(np.ones(48), part, pkg.same_cfg(**START_CFG), state), want)
        state, done = want[4], done + n
        msgs.append(want[0])
    msgs = np.concatenate(msgs)
    check_start_units(msgs[np.argsort(msgs["row"], kind="stable")])
    assert len(set(int(m["unit"]) for m in msgs)) >= 3, "the rows do not all open on one hypothesis"


def test_the_choice_among_hits_through_the_twin(pkg):
    """tie_cases(): a larger Q beats a lower tau, fewer mismatches beat a larger Q, and a hypothesis under min_quality is no hit --
    decided by the twin's own choice over a batch that is not silent, seen in the start the burst records"""
    for name, st, plane, settings, u in tie_cases():
        kw = settings(same_model(plane, st)[2][0, 0])
        want = same_model(plane, st, **kw)
        same(name, pkg.same_plan_host([1], plane, pkg.same_cfg(**kw), st), want)
        assert want[4]["an"][0] == 1 and want[4]["akind"][0] == EOM and want[4]["astart_unit"][0] == tie_start_unit(u), name


def test_a_disabled_row_padded_strides_and_capped_sentinel_filled_outputs(pkg):
    names, plane, _ = builders()
    plane = plane[:5, :40 * WAVE_BATCH]
    en = np.array([1, 0, 1, 1, 1], np.uint8)
    st = fresh_state(5)
    st["x"] = np.random.default_rng(2).normal(0, 0.1, (5, 30)).astype(np.float32)
    st["batch"], st["grid"] = 0xFFFFFFFF - 3, 80 * 7
    nb = 40
    want = same_model(plane, st, en)
    padded = np.full((5, nb * WAVE_BATCH + 1300), np.float32(0.25))
    padded[:, :nb * WAVE_BATCH] = plane
    twin = pkg.same_plan_host(en, padded, state=st, nbatches=nb)
    same("a disabled row, padded", twin, want)
    assert twin[5].view(STATE)[1].tobytes() == st[1].tobytes() and not twin[1][1].any() and want[4]["batch"][0] == nb - 4
    total = len(want[0])
    assert total >= 3
    L = pkg.lib()
    msgs = np.full(total + 2, 0xA5, np.uint8).repeat(MSG_REC.itemsize).view(MSG_REC)
    first, count, blob = np.zeros(6, np.uint32), np.zeros(2, np.uint32), st.copy()
    assert L.mi_same_plan_host(None, en.ctypes.data, 5, nb, padded.ctypes.data, padded.shape[1], blob.ctypes.data, None, None, msgs.ctypes.data, 2,
                               first.ctypes.data, count.ctypes.data) == pkg.MI_OK
    assert tuple(count) == (total, 2) and msgs[:2].tobytes() == want[0][:2].tobytes() and (msgs[2:].view(np.uint8) == 0xA5).all()
    assert blob.tobytes() == want[4].tobytes()


@pytest.mark.parametrize("hold", [False, True])
def test_every_timing_move_from_a_seeded_state(pkg, hold):
    names, st, plane, moves = timing_cases()
    kw = dict(max_bad=16, hold_timing=hold)  # (a batch is 8 bytes: no burst ends in it)
    want = same_model(plane, st, **kw)
    same(f"timing, hold {hold}", pkg.same_plan_host(np.ones(len(names)), plane, pkg.same_cfg(**kw), st), want)
    check_timing_moves(names, moves, want[4], hold)


def check_timing_moves(names, moves, after, hold):
    for name, (u, v), s in zip(names, moves, after):
        if s["phase"] == BURST:
            assert s["u"] == (u if hold else v), f"{name}: u {u} -> {s['u']}, hold {hold}"
    assert (after["phase"] == BURST).all()


def test_templates_within_one_float32_step_and_orthogonal_over_a_bit(pkg):
    T = pkg.same_templates()
    assert T.tobytes() == templates().tobytes()
    rho = np.arange(UNITS, dtype=np.float64)
    exact = np.stack([np.cos(2 * np.pi * 4 * rho / UNITS), np.sin(2 * np.pi * 4 * rho / UNITS), np.cos(2 * np.pi * 3 * rho / UNITS), np.sin(2 * np.pi * 3 * rho / UNITS)])
    assert (np.abs(T.astype(np.float64) - exact) <= np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)).all()
    # a space tone of amplitude 1 through the mark correlators over a bit's samples, at every rho of the first sample: the leak against
    # the space power.  In exact arithmetic over 30.72 samples the sums do not vanish (a bit is no whole number of samples): measured
    # 1.8e-5 of the space power at worst; the bound is 4 x that.
    worst = 0.0
    for rho0 in range(25):
        r = rho0 + 25 * np.arange(31 if rho0 <= 17 else 30)
        x = exact[3][r]
        pm = (x * T[0][r]).sum() ** 2 + (x * T[1][r]).sum() ** 2
        ps = (x * T[2][r]).sum() ** 2 + (x * T[3][r]).sum() ** 2
        worst = max(worst, pm / ps)
    print("mark power of a space tone, worst over rho:", worst)
    assert worst <= 4 * 1.8e-5


def test_message_text_and_fields_ok_on_good_and_malformed_headers(pkg):
    good = [HEADER_TEXT, LONGEST, b"ZCZC-EAS-RWT-012345+0015-0011200-ABCD EFG-"]
    bad = [HEADER_TEXT[:-1], HEADER_TEXT.replace(b"WXR", b"WxR"), HEADER_TEXT.replace(b"039173", b"03917A"), HEADER_TEXT.replace(b"+0030", b"+003"),
           HEADER_TEXT.replace(b"1591829", b"159182X"), HEADER_TEXT.replace(b"KCLE/NWS", b"KCLE\x7fNWS"), b"ZCZC-WXR-TOR+0030-1591829-KCLE/NWS-",
           LONGEST.replace(b"+0100", b"-032007+0100"), HEADER_TEXT.replace(b"ZCZC", b"ZCZD"), b"NNNN"]
    for text, ok in [(t, True) for t in good] + [(t, False) for t in bad]:
        m = np.zeros((), MSG_REC)
        m["nbytes"], m["bytes"][:len(text)] = len(text), np.frombuffer(text, np.uint8)
        assert fields_ok(text) == ok, text
        if ok:
            assert pkg.same_message_text(m) == message_fields(text), text
        else:
            with pytest.raises(pkg.MiError):
                pkg.same_message_text(m)
    m["kind"] = EOM
    with pytest.raises(pkg.MiError):
        pkg.same_message_text(m)
    assert fields_ok(b"NNNN", EOM) and not fields_ok(b"NNNM", EOM)


def flipped(p, n):
    for i in range(n):
        p ^= 1 << (5 + 9 * i)
    return p


def test_every_hypothesis_choice_tie(pkg):
    """seeded histories one bit before the sync's last: fewer mismatches beat a larger Q, a larger Q beats a lower tau, the lowest tau
    wins a full tie, a hypothesis under min_quality or over sync_errors is no hit -- in the model's pick and through the twin"""
    assert bin(SYNC[0] ^ SYNC[1]).count("1") == 10
    assert mismatch(flipped(SYNC[1], 4)) == (4, EOM) and mismatch(flipped(SYNC[0], 4)) == (4, HEADER)
    q = np.ones(NTAU, np.float32)
    mk = [(9, 0)] * NTAU
    for sets, qs, want in (({3: 2, 7: 1, 9: 1}, {3: 5.0, 9: 2.0}, 9), ({3: 1, 7: 1}, {}, 3), ({3: 5, 7: 4}, {}, 7), ({3: 0, 7: 1}, {3: 0.5}, 7)):
        m, qq = list(mk), q.copy()
        for t, v in sets.items():
            m[t] = (v, 0)
        for t, v in qs.items():
            qq[t] = v
        assert pick(m, qq, 4, 1.0) == want, sets
    # through the twin: a silent batch shifts a 1 into every history where the EOM pattern ends in 0, so hypotheses 4 and 11, seeded
    # with the pattern's other 63 bits, hit with one mismatch and hypothesis 2, seeded with one more flipped, with two: Q ties at 0 in
    # silence and the lowest tau of the two, 4, is chosen -- the start it records is 31 bits before hypothesis 4's first bit
    st = fresh_state(1)
    near = SYNC[1] >> 1
    assert SYNC[1] & 1 == 0
    st["hist"][0][[4, 11]] = near
    st["hist"][0][2] = near ^ (1 << 20)
    plane = np.zeros((1, WAVE_BATCH), np.float32)
    want = same_model(plane, st)
    same("tie", pkg.same_plan_host([1], plane, state=st), want)
    assert want[4]["an"][0] == 1 and want[4]["akind"][0] == EOM and want[4]["astart_unit"][0] == 48 * 4 - UNITS - 31 * UNITS + BATCH_UNITS
    assert want[4]["astart_batch"][0] == 0xFFFFFFFF


def test_ten_minutes_of_noise_and_of_voice_close_no_message_with_fields_ok(pkg):
    """the condition the defaults rest on, through the twin (which the tests above pin to the model): 4800 batches each"""
    n = 4800 * WAVE_BATCH
    for what, x in (("noise", np.random.default_rng(11).normal(0, 0.1, n)), ("voice", voice_like(n, 12))):
        msgs = pkg.same_plan_host([1], x.astype(np.float32)[None, :])[0]
        assert not (msgs["fields_ok"] == 1).any(), f"{what}: {msgs}"
