"""The aligned trailing window of live calls (tfp_live_window_aligned, csrc/tfp_live.hip live_key_cols_kernel,
live_window_boxes_kernel, live_pairs_kernel in front of launch_align): after every call the rows, frame
counts and first frames are tfp_live_window's, and every row's alignment is tfp_align_batch's on exactly
the kept frame values of the channel's window (the per-frame predicate of fp_handler.c:287-351 along the
clip's stored rows), with the form that served each call asserted through tfp_live_window_aligned_stats
and tfp_live_window_stats."""
import numpy as np
import pytest

import align_util as A
import live_util as L
import live_window_aligned_util as WA
import live_window_util as W
import scoped_util as S

pytestmark = pytest.mark.gpu

T, TICKS = W.T, W.TICKS


@pytest.fixture(scope="module")
def db(engine, tfp_lib):
    d = L.build_db(tfp_lib, engine)
    yield d
    engine.index_clear()


def _hist(n=8):
    return [np.zeros(0, np.int16) for _ in range(n)]


def _aligned_unmoved(tfp_lib, engine, lv, p, scopes, k, window, where):
    """The aligned call alone: it launches no fingerprint kernel, moves no push counter and does not move
    the engine's tfp_align_stats. Returns what it returned (the caller checks it against the definition)."""
    fp0, st0, al0 = engine.fingerprint_stats(), lv.stats(), engine.align_stats()
    got = lv.window_aligned(p, scopes, k, window)
    assert engine.fingerprint_stats() == fp0 and lv.stats() == st0 and engine.align_stats() == al0, where
    return got


@pytest.mark.parametrize("k", [1, 3, 32])
@pytest.mark.parametrize("tol", [0.001, 0.45])
@pytest.mark.parametrize("window", [1, 7, 25])
def test_every_tick_equals_window_rows_and_align_batch(engine, tfp_lib, oracle, db, window, tol, k):
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, tol)
    lv = tfp_lib.Live(engine, 8, TICKS * T)
    hist = _hist()
    npairs = 0
    for t in range(TICKS):
        W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
        first_call = _aligned_unmoved(tfp_lib, engine, lv, p, L.SCOPES8, k, window, t)
        rows, al, fc, ff = WA.check_aligned(tfp_lib, engine, lv, p, L.SCOPES8, k, window, t)
        assert first_call == (rows, al, fc, ff), t  # asked twice: the same answer
        assert lv.window(p, L.SCOPES8, k, window) == (rows, fc, ff), t
        npairs += 2 * sum(len(r) for r in rows)
    ast = lv.window_aligned_stats()
    assert ast == {"inplace_calls": 2 * TICKS, "general_calls": 0, "pairs": npairs}
    st = lv.window_stats()
    assert st["rebuilds"] == 1 and st["general_calls"] == 0 and st["slid_calls"] == 3 * TICKS
    # the last tick against the numpy brute force: the DB scenario's rows of the clip, the oracle's own
    # fingerprint of the call sliced to the window
    for c in range(8):
        _, qdb, _ = oracle.fingerprint(hist[c])
        assert len(qdb) - ff[c] == fc[c]
        for r, row in enumerate(rows[c]):
            m1, m2 = A.clip_rows(db, db["uuids"].index(row["audio_uuid"]))
            exp = A.brute_force(oracle, m1, m2, list(qdb[ff[c]:, 0]), list(qdb[ff[c]:, 1]), 1, tol)
            assert A.four(al[c][r]) == exp, (c, r, row)
    lv.close()


@pytest.mark.parametrize("window", [1, 2, 3])
def test_hop_edges(engine, tfp_lib, db, window):
    """Single samples across S = 254 ... 259 and 510 ... 515 (the tail appears, becomes final, the window's
    first frame moves), then ticks with per-channel lengths that all differ, 0 among them."""
    src = L.calls(tfp_lib, db, 4200)
    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, 4200)
    hist = _hist()
    at = 0
    for n in [254] + [1] * 5 + [251] + [1] * 5:
        W.push_all(lv, hist, src[:, at:at + n])
        at += n
        WA.check_aligned(tfp_lib, engine, lv, p, L.SCOPES8, 3, window, at)
    assert at == 515
    lv.reset()
    hist = _hist()
    pos = [0] * 8
    for tk in [1000, 1, 255, 256, 257, 511, 512, 513]:
        n = [tk * c // 7 for c in range(8)]  # channel 0 idle, channel 7 the whole tick
        blk = np.full((8, tk), 12345, np.int16)
        for c in range(8):
            blk[c, :n[c]] = src[c, pos[c]:pos[c] + n[c]]
            pos[c] += n[c]
        W.push_all(lv, hist, blk, nsamples=n)
        rows, al, fc, ff = WA.check_aligned(tfp_lib, engine, lv, p, L.SCOPES8, 3, window, tk)
        assert rows[0] == [] and al[0] == [WA.ZERO] * 3 and fc[0] == 0 and ff[0] == 0 and lv.samples(0) == 0
    assert lv.window_aligned_stats()["general_calls"] == 0 and lv.window_stats()["general_calls"] == 0
    lv.close()


def _long_clip(tfp_lib):
    """160,000 samples (625 frames) of noise whose gain follows a pseudo-random two-level sequence, one level
    per 256-sample frame (peaks of about 2,600 and about 30): the frames' keys fall in an aperiodic pattern,
    so a window's key sequence occurs once in the clip."""
    noise = tfp_lib.synth_pcm(0xBEEF, [0], 160000)[0].astype(np.float64)
    level = np.random.RandomState(7).randint(0, 2, 625)
    gain = np.where(level == 1, 2600.0, 30.0) / np.abs(noise).max()
    return np.round(noise * np.repeat(gain, 256)).astype(np.int16)


LONG_SCOPE_OWN, LONG_SCOPE_KEYS = 11, 12


@pytest.mark.parametrize("rows_of_clip,tol", [("own", 0.45), ("keys", 0.001)])
def test_band_edges_on_a_long_clip(tfp_lib, oracle, monkeypatch, rows_of_clip, tol):
    """The live DB's clips have at most 62 rows, so window + N - 1 fits one 256-diagonal band. One more clip
    of 160,000 samples (625 rows) is enrolled into the index delta and played on channel 0 from clip frame
    240 (offset + F - 1 crosses the band edge 255 | 256 as the call grows) and on channel 1 from clip frame
    600 to its end and 640 samples of silence beyond (the last, partial band; the window outruns the clip).
    Every tick equals tfp_align_batch, at window = 7 and at window = 48.

    A frame's box lies around the (int) truncation of its value (fp_handler.c:290), so at tol 0.001 a
    fingerprint's own stored values, a fraction above their keys, hit nothing at all (measured with the CPU
    oracle: no row at any tick). Two enrolments therefore: "own", the clip's own fingerprint, at tol 0.45,
    and "keys", each frame's truncated key just inside the box of tol 0.001, at tol 0.001. At window = 7
    the oracle finds one tick of channel 0 with a single attaining diagonal, and on channel 1 single
    diagonals away from the true start once the window holds the silence past the clip's end; so, as the
    issue provides, the localisation is asserted at window = 48 (the whole call so far): at least one tick
    per channel has a single attaining diagonal (the CPU oracle finds 26 and 30 of 44), and on every such
    tick first - offset is the true start, -240 and -600 call frames. The last tick equals the brute force
    on the oracle's own fingerprint of the call."""
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")
    eng = tfp_lib.Engine(0)
    L.build_db(tfp_lib, eng)
    clip = _long_clip(tfp_lib)
    fr = eng.fingerprint(clip)
    assert len(fr) == 625
    if rows_of_clip == "own":
        m1, m2, scope = fr["m1"].copy(), fr["m2"].copy(), LONG_SCOPE_OWN
    else:
        m1 = np.array([(int(v) if np.isfinite(v) else 0) * 1_000_000 + 500 for v in fr["q1"]], np.int32)
        m2, scope = np.zeros(625, np.int32), LONG_SCOPE_KEYS
    long_uuid = "7fffffff-2222-4000-8000-000000000090"
    eng.index_add(long_uuid, m1, m2)
    eng.index_set_scope([long_uuid], [scope])
    m1, m2 = m1.astype(np.int64), m2.astype(np.int64)
    nt = 44
    a = clip[240 * 256:240 * 256 + nt * T]
    b = clip[600 * 256:]
    b = np.concatenate([b, np.zeros(nt * T - len(b), np.int16)])
    src = np.stack([a, b])
    starts = (240, 600)
    p = tfp_lib.params(1, tol)
    lv = tfp_lib.Live(eng, 2, nt * T)
    for window in (7, 48):
        lv.reset()
        hist = _hist(2)
        single, bands = [0, 0], [set(), set()]
        for t in range(nt):
            W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
            rows, al, fc, ff = WA.check_aligned(tfp_lib, eng, lv, p, [scope, scope], 1, window, (window, t))
            for c in range(2):
                assert [r["audio_uuid"] for r in rows[c]] in ([], [long_uuid])
                if not rows[c]:
                    continue
                bands[c].add((al[c][0]["offset"] + fc[c] - 1) // 256)
                if window != 48:
                    continue
                # the reference's predicate over the kept frame values of the window, all diagonals
                q = lv.frames(c, ff[c])
                exp, _, multi = A.brute_force(oracle, m1, m2, [float(v) for v in q["q1"]], [float(v) for v in q["q2"]], 1, tol,
                                              more=True)
                assert A.four(al[c][0]) == exp, (t, c)
                if not multi:
                    single[c] += 1
                    assert ff[c] - al[c][0]["offset"] == -starts[c], (t, c, al[c][0])  # clip_start_frame
        if window == 48:
            assert single[0] >= 1 and single[1] >= 1, single  # the precondition: a unique diagonal exists
            # winning diagonals on both sides of the band edge 255 | 256, and in the last, partial band
            assert bands[0] >= {0, 1} and 2 in bands[1], bands
            for c in range(2):  # the last tick: the oracle's own fingerprint of the call, sliced to the window
                _, qdb, _ = oracle.fingerprint(hist[c])
                assert rows[c] and len(qdb) - ff[c] == fc[c]
                exp = A.brute_force(oracle, m1, m2, list(qdb[ff[c]:, 0]), list(qdb[ff[c]:, 1]), 1, tol)
                assert A.four(al[c][0]) == exp, c
    assert lv.window_aligned_stats()["general_calls"] == 0
    lv.close()
    eng.close()


def test_index_and_parameter_changes_between_calls(tfp_lib, monkeypatch):
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the index delta at this DB size too
    eng = tfp_lib.Engine(0)
    db = L.build_db(tfp_lib, eng)
    nt = 30
    src = L.calls(tfp_lib, db, nt * T)
    hist = _hist()
    lv = tfp_lib.Live(eng, 8, nt * T)
    state = {"t": 0, "p": tfp_lib.params(1, 0.45), "scopes": list(L.SCOPES8), "k": 3, "window": 7}

    def ticks(n, why):
        for _ in range(n):
            t = state["t"]
            W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
            got = WA.check_aligned(tfp_lib, eng, lv, state["p"], state["scopes"], state["k"], state["window"], (why, t))
            state["t"] += 1
        return got

    rows = ticks(10, "start")[0]
    first = rows[0][0]
    # a third copy of the clip channel 0 plays, under the greatest uuid, into the delta: it wins the channel
    fr = eng.fingerprint(db["pcm"][L.TWIN[0]])
    top = "ffffffff-2222-4000-8000-0000000000ff"
    eng.index_add(top, fr["m1"], fr["m2"])
    eng.index_set_scope([top], [2])
    rows, al, _, _ = ticks(2, "delta enrolment")
    assert eng.index_delta_stats()[1] == 1
    assert rows[0][0]["audio_uuid"] == top and rows[0][1]["audio_uuid"] == first["audio_uuid"]
    assert al[0][0]["aligned_count"] >= 1  # aligned from its staged rows (check_aligned: as tfp_align_batch does)
    eng.index_remove(top)
    rows = ticks(2, "removal")[0]
    assert all(r["audio_uuid"] != top for c in range(8) for r in rows[c]) and rows[0][0]["audio_uuid"] == first["audio_uuid"]
    fr = eng.fingerprint(tfp_lib.synth_pcm(L.SEED, [78], 9000)[0])
    eng.index_add("0b000000-2222-4000-8000-000000000078", fr["m1"], fr["m2"])
    eng.index_commit()
    ticks(2, "enrolment + merge")
    state["p"] = tfp_lib.params(1, 0.001)
    ticks(2, "tolerance")
    state["p"] = tfp_lib.params(1, 0.45)
    ticks(2, "tolerance again")
    state["scopes"] = [-1, 2, 0, 1, S.UNUSED_SCOPE, 0, 2, -1]
    ticks(2, "scopes")
    state["k"] = 32
    ticks(2, "k")
    state["window"] = 4
    rows = ticks(2, "window")[0]
    assert all(r["audio_uuid"] != top for c in range(8) for r in rows[c])
    assert state["t"] <= nt
    ast = lv.window_aligned_stats()
    assert ast["general_calls"] == 0 and ast["inplace_calls"] == state["t"]
    lv.close()
    eng.close()


@pytest.mark.parametrize("tol", [0.45, 0.001])
def test_general_form(engine, tfp_lib, db, tol):
    """coefs = 2: the rows come from the general form, the alignments test max2 as tfp_align_batch does.
    (No int16 input reaches a frame key outside the vote range, so that route of the general form cannot
    be driven through the public interface; it shares this code from the rows on.)"""
    ticks = 16
    src = W.two_part_calls(db)
    p = tfp_lib.params(2, tol)
    lv = tfp_lib.Live(engine, 8, ticks * T)
    hist = _hist()
    npairs = 0
    for t in range(ticks):
        W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
        rows = WA.check_aligned(tfp_lib, engine, lv, p, L.SCOPES8, 3, 7, t)[0]
        npairs += sum(len(r) for r in rows)
    assert lv.window_aligned_stats() == {"inplace_calls": 0, "general_calls": ticks, "pairs": npairs}
    assert lv.window_stats() == dict(zip(W.WSTAT_KEYS, (0, ticks, 0, 0, 0, 0)))
    lv.close()


def test_rowless_and_twin_clips(engine, tfp_lib, db):
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, TICKS * T)
    hist = _hist()
    twins = sorted(L.uuid_of(c) for c in L.TWIN)
    both = 0
    for t in range(0, 24, 2):
        W.push_all(lv, hist, src[:, t * T:(t + 2) * T])
        rows, al, _, _ = WA.check_aligned(tfp_lib, engine, lv, p, L.SCOPES8, 32, 7, t)
        for c in range(8):
            at = {r["audio_uuid"]: i for i, r in enumerate(rows[c])}
            assert L.uuid_of(L.ROWLESS) not in at
            if twins[0] in at:  # (assert_twins_tie: then both are, with equal counts)
                assert al[c][at[twins[0]]] == al[c][at[twins[1]]], (t, c)
                both += 1
    assert both
    lv.close()


def test_alternating_with_window_calls(engine, tfp_lib, db):
    """window and window_aligned alternate tick by tick on one object with differing `window` values: the
    mirror of the table's ranges predicts tfp_live_window_stats exactly when every call is fed to it."""
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, TICKS * T)
    rows_of = W.Rows(8)
    hist = _hist()
    last = None
    naligned = 0
    for t, window in enumerate([7, 7, 7, 7, 3, 3, 7, 3, 3, 3, 7, 7] * 2):
        W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
        if window != last:
            rows_of.restamp()
        last = window
        if t % 2:
            WA.check_aligned(tfp_lib, engine, lv, p, L.SCOPES8, 3, window, t)
            naligned += 1
        else:
            W.check_window(tfp_lib, engine, lv, p, L.SCOPES8, 3, window, t)
        rows_of.slid([len(h) for h in hist], window)
        rows_of.check(lv, t)
    assert lv.window_aligned_stats()["inplace_calls"] == naligned
    lv.close()
