"""The trailing window of live calls (tfp_live_window, csrc/tfp_live.hip live_slide_kernel): after every
call each channel's rows, frame count and first frame equal tfp_search_scoped_batch on exactly the kept
frame values of the last `window` frames of its call (application_handler.c:248-312 with the
recording's start moved along, searched as fp_handler.c:287-374 with the context predicate at
:308-314), with the form that served each call and the frames its count rows took and gave up asserted
through tfp_live_window_stats."""
import ctypes as C

import numpy as np
import pytest

import live_util as L
import live_window_util as W
import ranked_util as R
import scoped_util as S

pytestmark = pytest.mark.gpu

TFP_E_ARG = -1
T, TICKS = W.T, W.TICKS


@pytest.fixture(scope="module")
def db(engine, tfp_lib):
    d = L.build_db(tfp_lib, engine)
    yield d
    engine.index_clear()


def _hist(n=8):
    return [np.zeros(0, np.int16) for _ in range(n)]


def _window_no_fingerprint(tfp_lib, engine, lv, p, scopes, k, window, where):
    """check_window, and the call itself launches no fingerprint kernel and moves no push counter."""
    fp0, st0 = engine.fingerprint_stats(), lv.stats()
    rows, fc, ff = lv.window(p, scopes, k, window)
    assert engine.fingerprint_stats() == fp0 and lv.stats() == st0, where
    exp, efc, eff = W.definition_rows(tfp_lib, engine, lv, p, scopes, k, window)
    assert fc == efc and ff == eff, (where, fc, efc, ff, eff)
    for c in range(lv.nchannels):
        assert rows[c] == exp[c], (where, c, lv.samples(c))
        L.assert_twins_tie(rows[c])
    return rows


@pytest.mark.parametrize("k", [1, 3, 32])
@pytest.mark.parametrize("tol", [0.001, 0.45])
@pytest.mark.parametrize("window", [1, 2, 7, 25])
def test_every_tick_equals_the_window_search(engine, tfp_lib, oracle, db, window, tol, k):
    """8 two-part calls, 40 ticks of 160 samples, a searching push and then a window call per tick: every
    tick every channel equals the definition; while F <= window the rows are the push's; on the last tick
    they are the last window of the sliding search with hop 1; at the end they are the CPU oracle's."""
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, tol)
    lv = tfp_lib.Live(engine, 8, TICKS * T)
    rows_of = W.Rows(8)
    hist = _hist()
    leaders = []  # (tick, channel 0's anchored row 0, its window row 0)
    for t in range(TICKS):
        blk = src[:, t * T:(t + 1) * T]
        for c in range(8):
            hist[c] = np.concatenate([hist[c], blk[c]])
        anchored, fc = lv.push(blk, p, L.SCOPES8, k)
        rows = _window_no_fingerprint(tfp_lib, engine, lv, p, L.SCOPES8, k, window, t)
        rows_of.slid([len(h) for h in hist], window)
        rows_of.check(lv, t)
        for c in range(8):
            if fc[c] <= window:
                assert rows[c] == anchored[c], (t, c)
        leaders.append((t, anchored[0][:1], rows[0][:1]))
    st = lv.window_stats()
    assert st["rebuilds"] == 1 and st["general_calls"] == 0 and st["slid_calls"] == TICKS
    assert st["frames_added"] - st["frames_removed"] == sum(len(r) for r in rows_of.rng)
    # the last window of the sliding search over the call's frames [0, F), hop 1
    for c in range(8):
        fr = lv.frames(c)
        assert len(fr) == 25
        sl = engine.search_sliding_batch(fr, [0, len(fr)], p, window, 1, k, [L.SCOPES8[c]])
        assert rows[c] == sl[0][-1], c
    # the CPU oracle: its own fingerprint of the call, sliced to the window, brute force over the scope's clips
    for c in range(8):
        assert R.pairs(rows[c]) == W.oracle_window_rows(oracle, db, hist[c], tol, L.SCOPES8[c], k, window), c
    if window == 7 and tol == 0.45:
        # the window answers another question than the anchored rows: on the oracle's side channel 0's
        # first row differs on some tick after its call left its context's clip (and the engine agrees)
        differ = []
        for t in range(TICKS):
            h = src[0, :(t + 1) * T]
            a = L.oracle_rows(oracle, db, h, tol, L.SCOPES8[0], 1)
            w = W.oracle_window_rows(oracle, db, h, tol, L.SCOPES8[0], 1, window)
            if a and w and a[0][0] != w[0][0]:
                differ.append(t)
                assert R.pairs(leaders[t][1]) == a and R.pairs(leaders[t][2]) == w, t
        assert differ
    lv.close()


@pytest.mark.parametrize("window", [1, 2, 3])
def test_hop_edges(engine, tfp_lib, oracle, db, window):
    """Single samples across S = 254 ... 259 and 510 ... 515, then a first push of 1,000 samples and
    ticks around the hop with per-channel lengths that all differ (0 among them).

    The tail stored in the row fails at S = 255 -> 256 (frame 0 would count twice once it is final); a
    first frame that does not advance when the tail appears fails at S = 256 n -> 256 n + 1 (the row
    keeps a frame the window has left); window = 1 with a tail is the row whose stored range is empty
    (the rows come from the tail's bit alone)."""
    src = L.calls(tfp_lib, db, 4200)
    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, 4200)
    rows_of = W.Rows(8)
    hist = _hist()
    at = 0
    for n in [254] + [1] * 5 + [251] + [1] * 5:  # S = 254, 255 ... 259, 510, 511 ... 515
        W.push_all(lv, hist, src[:, at:at + n])
        at += n
        rows = _window_no_fingerprint(tfp_lib, engine, lv, p, L.SCOPES8, 3, window, at)
        rows_of.slid([len(h) for h in hist], window)
        rows_of.check(lv, at)
        if window == 1 and at % 256:
            assert all(not r for r in rows_of.rng)  # the stored ranges are empty: the tail alone
            assert any(rows[c] for c in range(8))
    assert at == 515
    for c in range(8):
        assert R.pairs(rows[c]) == W.oracle_window_rows(oracle, db, hist[c], 0.45, L.SCOPES8[c], 3, window), c
    lv.reset()
    rows_of.reset()
    hist = _hist()
    pos = [0] * 8
    for tk in [1000, 1, 255, 256, 257, 511, 512, 513]:
        n = [tk * c // 7 for c in range(8)]  # channel 0 idle, channel 7 the whole tick
        blk = np.full((8, tk), 12345, np.int16)  # past nsamples[c]: never read
        for c in range(8):
            blk[c, :n[c]] = src[c, pos[c]:pos[c] + n[c]]
            pos[c] += n[c]
        W.push_all(lv, hist, blk, nsamples=n)
        rows = _window_no_fingerprint(tfp_lib, engine, lv, p, L.SCOPES8, 3, window, tk)
        rows_of.slid([len(h) for h in hist], window)
        rows_of.check(lv, tk)
        assert rows[0] == [] and lv.samples(0) == 0
    for c in range(8):
        assert R.pairs(rows[c]) == W.oracle_window_rows(oracle, db, hist[c], 0.45, L.SCOPES8[c], 3, window), c
    st = lv.window_stats()
    assert st["general_calls"] == 0 and st["rebuilds"] == 1
    lv.close()


def test_catch_up_slides_then_restarts(engine, tfp_lib, oracle, db):
    """Ingest-only pushes for fewer than `window` frames between two calls, then for more: the first call
    slides every row, the second restarts every row (its target is disjoint from what the row holds)."""
    window = 7
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, TICKS * T)
    rows_of = W.Rows(8)
    hist = _hist()

    def ingest(t0, t1):
        for t in range(t0, t1):
            W.push_all(lv, hist, src[:, t * T:(t + 1) * T])

    def ask(where):
        rows = _window_no_fingerprint(tfp_lib, engine, lv, p, L.SCOPES8, 32, window, where)
        rows_of.slid([len(h) for h in hist], window)
        rows_of.check(lv, where)
        return rows, lv.window_stats()

    ingest(0, 16)  # S = 2,560: frames [3, 10)
    _, s0 = ask("first")
    assert s0["rows_restarted"] == 8 and s0["frames_added"] == 8 * 7 and s0["frames_removed"] == 0
    ingest(16, 20)  # S = 3,200: 2.5 frames on, the rows hold [3, 10) and owe [6, 12)
    _, s1 = ask("slide")
    assert s1["rows_restarted"] == s0["rows_restarted"]
    assert s1["frames_added"] - s0["frames_added"] == 8 * 2 and s1["frames_removed"] - s0["frames_removed"] == 8 * 3
    ingest(20, 36)  # S = 5,760: 10 frames on, the rows hold [6, 12) and owe [16, 22)
    rows, s2 = ask("restart")
    assert s2["rows_restarted"] - s1["rows_restarted"] == 8
    assert s2["frames_added"] - s1["frames_added"] == 8 * 6 and s2["frames_removed"] - s1["frames_removed"] == 8 * 6
    assert s2["slid_calls"] == 3 and s2["general_calls"] == 0 and s2["rebuilds"] == 1
    for c in range(8):
        assert R.pairs(rows[c]) == W.oracle_window_rows(oracle, db, hist[c], 0.45, L.SCOPES8[c], 32, window), c
    lv.close()


def test_packed_pairs_and_block_edges(engine, tfp_lib, db):
    """2,100 clips of a few crafted rows each; the call plays a clip and then the same clip 12 dB down, so
    its later frames take other keys than its first ones. Columns 2047 and 2048 have a row in the box of
    every key the call takes (its provisional tails' included), columns 2046 and 2049 only in the boxes
    of the keys of its first frames: as those frames leave the window the even column 2046 falls to 0
    while its odd neighbour 2047, packed into the same 32-bit word, stays at `window`, and the odd
    column 2049 falls to 0 while its even neighbour 2048 stays. 2047 | 2048 is the edge of the slide
    kernel's 2,048-column block and of the selection's second 1,024-column block. The four columns are
    scope 5, every other clip (rows in every key's box: they tie) alternates between scopes 0 and 1."""
    window = 6
    nsamp = TICKS * T
    loud = db["pcm"][L.TWIN[0]][1024:1024 + 15 * 256]
    quiet = (db["pcm"][L.TWIN[0]][1024 + 15 * 256:1024 + nsamp] // 4).astype(np.int16)
    call = np.concatenate([loud, quiet])
    src = np.stack([call, call])

    def keys_of(q1):
        return [int(v) if np.isfinite(v) else 0 for v in q1]  # (int) truncation, fp_handler.c:290

    key = keys_of(engine.fingerprint(call)["q1"])
    early, late = set(key[:10]), set(key[14:])
    assert early and late and not (early & late), (sorted(early), sorted(late))
    # every prefix a tick leaves, for the keys its zero-padded tail takes
    off = np.concatenate([[0], np.cumsum([(t + 1) * T for t in range(TICKS)])])
    pre = engine.fingerprint_batch(np.concatenate([call[:(t + 1) * T] for t in range(TICKS)]), off)
    every = sorted(set(key) | set(keys_of(pre["q1"])))
    n = 2100
    uuids = ["00000000-4444-4000-8000-%012d" % c for c in range(n)]  # column = c
    rows_all = np.array([k * 1_000_000 + 500 for k in every], np.int32)
    rows_early = np.array([k * 1_000_000 + 500 for k in sorted(early)], np.int32)
    m1 = [rows_early if c in (2046, 2049) else rows_all for c in range(n)]
    foff = np.concatenate([[0], np.cumsum([len(x) for x in m1])])
    engine.index_clear()
    engine.index_add_batch(uuids, foff, np.concatenate(m1), np.zeros(foff[-1], np.int32))
    engine.index_set_scope(uuids, [5 if 2046 <= c <= 2049 else c % 2 for c in range(n)])
    try:
        p = tfp_lib.params(1, 0.001)
        lv = tfp_lib.Live(engine, 2, nsamp)
        rows_of = W.Rows(2)
        hist = _hist(2)
        scopes = [5, -1]
        seen = set()
        for t in range(TICKS):
            W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
            rows = _window_no_fingerprint(tfp_lib, engine, lv, p, scopes, 32, window, t)
            rows_of.slid([len(h) for h in hist], window)
            rows_of.check(lv, t)
            first, F = W.window_of(tfp_lib, len(hist[0]), window)
            kw = keys_of(lv.frames(0, first)["q1"])
            assert len(kw) == F - first and set(kw) <= set(every)
            n_early = sum(k in early for k in kw)
            count = {2046: n_early, 2047: len(kw), 2048: len(kw), 2049: n_early}
            exp = sorted(((n_, uuids[c]) for c, n_ in count.items() if n_), reverse=True)
            assert [(r["match_count"], r["audio_uuid"]) for r in rows[0]] == exp, (t, rows[0], exp)
            if len(kw) == window:
                seen.add("all four at window" if n_early == window else "neighbours only" if n_early == 0 else "falling")
            # over every clip: 2,096 clips tie at every frame of the window, the greatest uuids first
            assert [r["audio_uuid"] for r in rows[1]] == [uuids[c] for c in range(n - 1, n - 33, -1)]
            assert all(r["match_count"] == len(kw) for r in rows[1])
        assert seen == {"all four at window", "falling", "neighbours only"}
        st = lv.window_stats()
        assert st["slid_calls"] == TICKS and st["general_calls"] == 0 and st["rebuilds"] == 1
        lv.close()
    finally:
        L.build_db(tfp_lib, engine)  # the module's DB back for the tests that follow


def test_mid_call_changes(tfp_lib, monkeypatch):
    """Index updates and changes of params, scope, k and window between calls, and a reset of one channel:
    every call equals the definition, the table restarts exactly on the steps that change its stamp, and
    a reset restarts one row only."""
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the index delta at this DB size too
    eng = tfp_lib.Engine(0)
    db = L.build_db(tfp_lib, eng)
    nt = 44
    src = L.calls(tfp_lib, db, nt * T)
    hist = _hist()
    lv = tfp_lib.Live(eng, 8, nt * T)
    rows_of = W.Rows(8)
    state = {"t": 0, "p": tfp_lib.params(1, 0.45), "scopes": list(L.SCOPES8), "k": 3, "window": 7, "rebuilds": 0}

    def ticks(n, rebuilt, why):
        if rebuilt:
            rows_of.restamp()
        for _ in range(n):
            t = state["t"]
            W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
            rows = _window_no_fingerprint(tfp_lib, eng, lv, state["p"], state["scopes"], state["k"], state["window"], (why, t))
            rows_of.slid([len(h) for h in hist], state["window"])
            rows_of.check(lv, (why, t))
            state["t"] += 1
        state["rebuilds"] += rebuilt
        assert lv.window_stats()["rebuilds"] == state["rebuilds"], why
        return rows

    rows = ticks(12, 1, "start")
    first = rows[0][0]  # scope 2's first row before the enrolments
    fr = eng.fingerprint(tfp_lib.synth_pcm(L.SEED, [77], 9000)[0])
    eng.index_add("0a000000-2222-4000-8000-000000000077", fr["m1"], fr["m2"])
    ticks(2, 1, "delta enrolment")
    assert eng.index_delta_stats()[1] == 1
    eng.index_commit()
    ticks(1, 0, "idle commit")
    fr = eng.fingerprint(tfp_lib.synth_pcm(L.SEED, [78], 9000)[0])
    eng.index_add("0b000000-2222-4000-8000-000000000078", fr["m1"], fr["m2"])
    eng.index_commit()
    ticks(2, 1, "enrolment + commit")
    # a third copy of the clip channel 0 plays, under the greatest uuid: it ties with the first row
    fr = eng.fingerprint(db["pcm"][L.TWIN[0]])
    top = "ffffffff-2222-4000-8000-0000000000ff"
    eng.index_add(top, fr["m1"], fr["m2"])
    eng.index_set_scope([top], [2])
    rows = ticks(2, 1, "tie enrolment")
    assert [r["audio_uuid"] for r in rows[0][:2]] == [top, first["audio_uuid"]]
    assert rows[0][0]["match_count"] == rows[0][1]["match_count"]
    eng.index_remove(top)
    rows = ticks(2, 1, "removal")
    assert rows[0][0]["audio_uuid"] == first["audio_uuid"]
    state["p"] = tfp_lib.params(1, 0.001)
    ticks(2, 1, "tolerance")
    state["p"] = tfp_lib.params(1, 0.001, 3, -1)
    ticks(2, 1, "ignore low")
    state["p"] = tfp_lib.params(1, 0.001, 3, 2000)
    ticks(2, 1, "ignore high")
    state["scopes"] = [-1, 2, 0, 1, S.UNUSED_SCOPE, 0, 2, -1]
    ticks(2, 0, "scopes")
    eng.index_set_scope([L.uuid_of(7)], [2])  # a clip moves to another context: the scope table, not the counts
    ticks(1, 0, "set_scope")
    state["k"] = 32
    ticks(2, 0, "k")
    state["window"] = 4
    ticks(2, 1, "window")
    state["p"] = tfp_lib.params(1, 0.45)
    ticks(1, 1, "tolerance again")
    # a new call on channel 2: its row alone starts again, the others slide on
    before = lv.window_stats()
    lv.reset(2)
    rows_of.reset(2)
    hist[2] = np.zeros(0, np.int16)
    ticks(4, 0, "reset")  # 640 samples: channel 2 has final frames again
    after = lv.window_stats()
    assert after["rows_restarted"] - before["rows_restarted"] == 1 and after["rebuilds"] == before["rebuilds"]
    assert state["t"] <= nt
    st = lv.window_stats()
    assert st["general_calls"] == 0 and st["slid_calls"] == state["t"]
    assert lv.stats()["incremental_pushes"] == 0 and lv.stats()["rebuilds"] == 0  # tfp_live_stats: not moved
    lv.close()
    eng.close()


@pytest.mark.parametrize("tol", [0.001, 0.1])
def test_coefs_2_takes_the_general_form(engine, tfp_lib, oracle, db, tol):
    ticks = 24
    src = W.two_part_calls(db)
    p = tfp_lib.params(2, tol)
    lv = tfp_lib.Live(engine, 8, ticks * T)
    hist = _hist()
    for t in range(ticks):
        W.push_all(lv, hist, src[:, t * T:(t + 1) * T])
        rows = _window_no_fingerprint(tfp_lib, engine, lv, p, L.SCOPES8, 3, 7, t)
    st = lv.window_stats()
    assert st == dict(zip(W.WSTAT_KEYS, (0, ticks, 0, 0, 0, 0)))
    for c in range(8):
        assert R.pairs(rows[c]) == W.oracle_window_rows(oracle, db, hist[c], tol, L.SCOPES8[c], 3, 7, coefs=2), c
    lv.close()


def test_argument_errors_write_nothing(engine, tfp_lib, db):
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, TICKS * T)
    hist = _hist()
    W.push_all(lv, hist, src[:, :1000])
    lib = tfp_lib.lib()
    k = 3
    out = (C.c_uint8 * (C.sizeof(tfp_lib.engine.Candidate) * 8 * k))(*([0xA5] * (C.sizeof(tfp_lib.engine.Candidate) * 8 * k)))
    cnt, fc, ff = [(C.c_int32 * 8)(*([-7] * 8)) for _ in range(3)]
    ok = np.asarray(L.SCOPES8, np.int32)
    bad = np.asarray([-2] + [0] * 7, np.int32)

    def call(params, scopes, k_, window, o=out, c=cnt):
        return lib.tfp_live_window(lv._h, params, scopes.ctypes.data, k_, window, o, c, fc, ff)

    for args in ((C.byref(p), ok, k, 0), (C.byref(p), ok, k, -3), (C.byref(p), ok, 0, 7), (C.byref(p), ok, 33, 7),
                 (C.byref(p), bad, k, 7), (None, ok, k, 7)):
        assert call(*args) == TFP_E_ARG, args[1:]
    assert call(C.byref(p), ok, k, 7, o=None) == TFP_E_ARG and call(C.byref(p), ok, k, 7, c=None) == TFP_E_ARG
    assert bytes(out) == b"\xa5" * len(out) and list(cnt) == [-7] * 8 and list(fc) == [-7] * 8 and list(ff) == [-7] * 8
    assert lv.window_stats() == dict.fromkeys(W.WSTAT_KEYS, 0)
    for kw in ({"window": 0}, {"k": 0}, {"scopes": [-2] + [0] * 7}):
        with pytest.raises(tfp_lib.TfpError) as ei:
            lv.window(p, **{"scopes": L.SCOPES8, "k": 3, "window": 7, **kw})
        assert ei.value.code == TFP_E_ARG, kw
    # frame_counts and first_frames may be NULL; invalid params give empty rows (fp_handler.c:247-250)
    assert lib.tfp_live_window(lv._h, C.byref(p), ok.ctypes.data, k, 7, out, cnt, None, None) == 0
    rows, fcs, ffs = lv.window(tfp_lib.params(3, 0.45), L.SCOPES8, 3, 2)
    assert rows == [[]] * 8 and fcs == [2] * 8 and ffs == [2] * 8
    # tfp_live_frames: the capacity error carries the need; a channel or first out of range
    got = C.c_int64(-1)
    buf = np.zeros(4, tfp_lib.FRAME_DTYPE)
    assert lib.tfp_live_frames(lv._h, 3, 0, buf.ctypes.data, 3, C.byref(got)) == TFP_E_ARG and got.value == 4
    assert lib.tfp_live_frames(lv._h, 3, 1, buf.ctypes.data, 3, C.byref(got)) == 0 and got.value == 3
    assert list(buf["frame_idx"][:3]) == [1, 2, 3]
    with pytest.raises(tfp_lib.TfpError) as ei:
        lv.frames(3, 0, cap=3)
    assert ei.value.code == TFP_E_ARG
    for ch, first in ((8, 0), (-1, 0), (3, 5), (3, -1)):
        with pytest.raises(tfp_lib.TfpError) as ei:
            lv.frames(ch, first)
        assert ei.value.code == TFP_E_ARG, (ch, first)
    assert len(lv.frames(3, 4)) == 0
    lv.close()
    # an empty index gives no rows; a channel with S = 0 gives none, frame_counts = 0 and first_frames = 0
    eng = tfp_lib.Engine(0)
    lv = tfp_lib.Live(eng, 2, 4000)
    lv.push(np.stack([src[0, :600], src[1, :600]]), None, nsamples=[600, 0])
    rows, fcs, ffs = lv.window(p, None, 3, 2)
    assert rows == [[], []] and fcs == [2, 0] and ffs == [1, 0]
    assert lv.window_stats()["slid_calls"] == 1 and lv.window_stats()["rebuilds"] == 0
    lv.close()
    eng.close()


def _codes(tfp_lib, pcm, law):
    """Codes whose expansion is near pcm: the nearest of the law's 256 values per sample."""
    table = tfp_lib.decode_g711(np.arange(256, dtype=np.uint8), law).astype(np.int32)
    order = np.argsort(table, kind="stable")
    pos = np.clip(np.searchsorted(table[order], pcm.astype(np.int32)), 0, 255)
    return order[pos].astype(np.uint8)


def test_g711_pushes_equal_int16_pushes_of_the_expansion(engine, tfp_lib, db):
    src = W.two_part_calls(db)
    p = tfp_lib.params(1, 0.45)
    a, b = tfp_lib.Live(engine, 8, TICKS * T), tfp_lib.Live(engine, 8, TICKS * T)
    hist = _hist()
    for t in range(20):
        law = (tfp_lib.ULAW, tfp_lib.ALAW)[t % 2]
        codes = _codes(tfp_lib, src[:, t * T:(t + 1) * T], law)
        pcm = tfp_lib.decode_g711(codes.reshape(-1), law).reshape(8, T)
        W.push_all(a, hist, pcm, law=law, codes=codes)
        assert b.push(pcm, None) is None
        rows = _window_no_fingerprint(tfp_lib, engine, a, p, L.SCOPES8, 3, 5, t)
        assert b.window(p, L.SCOPES8, 3, 5)[0] == rows, t
    assert a.window_stats() == b.window_stats() and a.window_stats()["slid_calls"] == 20
    a.close()
    b.close()
