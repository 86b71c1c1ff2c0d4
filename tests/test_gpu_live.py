"""Live calls (tfp_live_*, csrc/tfp_live.hip): after every push each channel's rows, counts and frame
count equal tfp_search_scoped_pcm_batch on exactly the samples the channel has taken since its last
reset (the recording application_handler.c:248-312 makes, searched as fp_handler.c:287-374 with the
context predicate at :308-314), with the path each push took asserted through tfp_live_stats."""
import numpy as np
import pytest

import live_util as L
import ranked_util as R
import scoped_util as S

pytestmark = pytest.mark.gpu

TFP_E_ARG, TFP_E_CAPACITY = -1, -5
T = 160  # a 20 ms SLIN tick at 8 kHz
TICKS = 40


@pytest.fixture(scope="module")
def db(engine, tfp_lib):
    d = L.build_db(tfp_lib, engine)
    yield d
    engine.index_clear()


def _run_ticks(tfp_lib, engine, lv, src, p, scopes, k, ticks=TICKS):
    hist = [np.zeros(0, np.int16) for _ in range(src.shape[0])]
    need = 0
    for t in range(ticks):
        for h in hist:  # frames a push of T samples must fingerprint: the old tail and everything after it
            need += tfp_lib.frame_count(len(h) + T) - len(h) // 256 + 1
        L.check_push(tfp_lib, engine, lv, hist, src[:, t * T:(t + 1) * T], p, scopes, k, where=t)
    return hist, need


@pytest.mark.parametrize("tol,k", [(0.001, 1), (0.001, 3), (0.001, 32), (0.45, 1), (0.45, 3), (0.45, 32)])
def test_every_tick_equals_the_prefix_search(engine, tfp_lib, oracle, db, tol, k):
    """8 channels, 40 ticks of 160 samples: every tick every channel equals the scoped prefix search.
    The work is O(new audio): at most one lead-in frame beyond the frames each push needs, far below
    re-fingerprinting the prefixes, and every final frame is added to a count row exactly once."""
    src = L.calls(tfp_lib, db, TICKS * T)
    p = tfp_lib.params(1, tol)
    lv = tfp_lib.Live(engine, 8, TICKS * T)
    hist, need = _run_ticks(tfp_lib, engine, lv, src, p, L.SCOPES8, k)
    st = lv.stats()
    assert st["incremental_pushes"] == TICKS and st["general_pushes"] == 0 and st["rebuilds"] == 1
    assert st["frames_fingerprinted"] <= need
    whole = sum(tfp_lib.frame_count((t + 1) * T) for t in range(TICKS)) * 8
    assert st["frames_fingerprinted"] * 4 < whole
    assert st["frames_added"] == sum(len(h) // 256 for h in hist)
    # the CPU oracle on the final prefixes (its own fingerprint and a brute-force count over the scope's clips)
    rows, _ = lv.push(np.zeros((8, 1), np.int16), p, L.SCOPES8, k, nsamples=[0] * 8)
    for c in range(8):
        assert R.pairs(rows[c]) == L.oracle_rows(oracle, db, hist[c], tol, L.SCOPES8[c], k), c
    assert all(r["audio_uuid"] != L.uuid_of(L.ROWLESS) for c in range(8) for r in rows[c])
    lv.close()


def test_hop_edges(engine, tfp_lib, oracle, db):
    """Tick sizes around the hop and the window, per-channel lengths that all differ (0 and the whole
    tick among them), then single samples across S = 255 -> 256 -> 257.

    A tail added by mistake fails at S = 255 -> 256: the provisional frame 0 would be in the count row
    at 255 and added again when it becomes final at 256 (and on every channel whose tick leaves a tail
    that the next tick completes). A missing lead-in hop fails at every push with floor(S_old / 256) > 0,
    first at the tick of 1 sample after the first push (channel 7: S_old = 1000, frame 3 would read zeros
    for samples 512 ... 767). The first push gives channel 7 three final frames at once."""
    sizes = [1000, 1, 255, 256, 257, 511, 512, 513]
    src = L.calls(tfp_lib, db, sum(sizes))
    p = tfp_lib.params(1, 0.45)
    lv = tfp_lib.Live(engine, 8, sum(sizes))
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    at = [0] * 8
    for tk in sizes:
        n = [tk * c // 7 for c in range(8)]  # channel 0 idle, channel 7 the whole tick
        blk = np.zeros((8, tk), np.int16)
        for c in range(8):
            blk[c, :n[c]] = src[c, at[c]:at[c] + n[c]]
            blk[c, n[c]:] = 12345  # past nsamples[c]: never read
            at[c] += n[c]
        rows = L.check_push(tfp_lib, engine, lv, hist, blk, p, L.SCOPES8, 3, nsamples=n, where=tk)
        assert rows[0] == [] and len(hist[0]) == 0
    assert lv.samples(7) == sum(sizes) and lv.samples(0) == 0
    # the kept frame values themselves (every one came through a push's clip, most behind a lead-in
    # frame): coefs = 2 boxes the second value of each, so a wrong one changes these rows
    L.check_push(tfp_lib, engine, lv, hist, blk, tfp_lib.params(2, 0.1), L.SCOPES8, 3, nsamples=[0] * 8, where="values")
    for c in range(8):
        assert R.pairs(lv.push(blk, p, L.SCOPES8, 3, nsamples=[0] * 8)[0][c]) == \
            L.oracle_rows(oracle, db, hist[c], 0.45, L.SCOPES8[c], 3), c
    lv.reset()
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    L.check_push(tfp_lib, engine, lv, hist, src[:, :254], p, L.SCOPES8, 3, where="254")
    for i in range(254, 259):  # S = 255, 256, 257, 258, 259
        L.check_push(tfp_lib, engine, lv, hist, src[:, i:i + 1], p, L.SCOPES8, 3, where=i + 1)
    st = lv.stats()
    assert st["general_pushes"] == 1 and st["rebuilds"] == 1
    assert st["incremental_pushes"] == len(sizes) + 8 + 6
    lv.close()


def test_mid_call_changes(tfp_lib, monkeypatch):
    """Index updates and parameter changes between pushes: every push after each equals the prefix
    search, and the count table is rebuilt exactly on the steps that change its stamp."""
    monkeypatch.setenv("TFP_INDEX_DELTA", "1")  # the index delta at this DB size too
    eng = tfp_lib.Engine(0)
    db = L.build_db(tfp_lib, eng)
    src = L.calls(tfp_lib, db, 42 * T)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    lv = tfp_lib.Live(eng, 8, 42 * T)
    state = {"t": 0, "p": tfp_lib.params(1, 0.45), "scopes": list(L.SCOPES8), "k": 3, "rebuilds": 0}

    def ticks(n, rebuilt, why):
        for _ in range(n):
            t = state["t"]
            rows = L.check_push(tfp_lib, eng, lv, hist, src[:, t * T:(t + 1) * T], state["p"], state["scopes"], state["k"],
                                where=(why, t))
            state["t"] += 1
        state["rebuilds"] += rebuilt
        assert lv.stats()["rebuilds"] == state["rebuilds"], why
        return rows

    rows = ticks(12, 1, "start")
    first = rows[0][0]  # scope 2's first row before the enrolments
    # an enrolment that lands in the delta
    fr = eng.fingerprint(tfp_lib.synth_pcm(L.SEED, [77], 9000)[0])
    eng.index_add("0a000000-2222-4000-8000-000000000077", fr["m1"], fr["m2"])
    ticks(3, 1, "delta enrolment")
    assert eng.index_delta_stats()[1] == 1
    # tfp_index_commit with nothing pending leaves the index, and the table, as they are; after an
    # enrolment it applies it, and the next push rebuilds once
    eng.index_commit()
    ticks(2, 0, "idle commit")
    fr = eng.fingerprint(tfp_lib.synth_pcm(L.SEED, [78], 9000)[0])
    eng.index_add("0b000000-2222-4000-8000-000000000078", fr["m1"], fr["m2"])
    eng.index_commit()
    ticks(2, 1, "enrolment + commit")
    # a third copy of the clip channel 0 plays, under the greatest uuid: it ties with the first row
    # and so enters at rank 1, the earlier rows move down a rank
    fr = eng.fingerprint(db["pcm"][L.TWIN[0]])
    top = "ffffffff-2222-4000-8000-0000000000ff"
    eng.index_add(top, fr["m1"], fr["m2"])
    eng.index_set_scope([top], [2])
    rows = ticks(3, 1, "tie enrolment")
    assert [r["audio_uuid"] for r in rows[0][:2]] == [top, first["audio_uuid"]]
    assert rows[0][0]["match_count"] == rows[0][1]["match_count"]
    # the current winner removed
    eng.index_remove(top)
    rows = ticks(3, 1, "removal")
    assert rows[0][0]["audio_uuid"] == first["audio_uuid"]
    # a tolerance change, an ignore-filter change: rebuilt; a scope change, another k: not
    state["p"] = tfp_lib.params(1, 0.001)
    ticks(3, 1, "tolerance")
    state["p"] = tfp_lib.params(1, 0.001, 3, -1)
    ticks(3, 1, "ignore low")
    state["p"] = tfp_lib.params(1, 0.001, 3, 2000)
    ticks(3, 1, "ignore high")
    state["scopes"] = [-1, 2, 0, 1, S.UNUSED_SCOPE, 0, 2, -1]
    ticks(3, 0, "scopes")
    eng.index_set_scope([L.uuid_of(7)], [2])  # a clip moves to another context: the scope table, not the counts
    ticks(2, 0, "set_scope")
    state["k"] = 32
    ticks(3, 0, "k")
    st = lv.stats()
    assert st["general_pushes"] == 0 and st["incremental_pushes"] == state["t"]
    lv.close()
    eng.close()


def test_column_block_edge(engine, tfp_lib, db):
    """1,100 clips of a few crafted rows each: the selection's block of 1,024 columns is crossed, the
    winners sit in the last column of block 0 and the first of block 1, and the scopes alternate.

    Every clip has one row in the box of every key the call's frames take (the synthetic audio's first
    coefficient hardly moves, so there are few), so all 1,100 clips tie at every tick and a scope's
    first row is its greatest uuid, i.e. its last column. Columns 0 ... 1024 alternate between scopes
    0 and 1 and the columns after them between scopes 2 and 3: scope 1's winner is column 1023, the last
    of block 0, scope 0's is column 1024, the first of block 1, both decided by the tie key alone, across
    the per-block lists' merge; over every clip the rows are columns 1099, 1098, ..."""
    src = np.repeat(L.calls(tfp_lib, db, 12 * T)[:1], 2, axis=0)  # both channels play the same call
    keys = sorted({int(v) if np.isfinite(v) else 0 for v in engine.fingerprint(src[0])["q1"]})  # (int) truncation, :290
    n = 1100
    uuids = ["00000000-3333-4000-8000-%012d" % c for c in range(n)]  # column = c
    engine.index_clear()
    m1 = np.array([k * 1_000_000 + 500 for k in keys], np.int32)
    for c in range(n):
        engine.index_add(uuids[c], m1, np.zeros(len(keys), np.int32))
    engine.index_set_scope(uuids, [c % 2 if c <= 1024 else 2 + c % 2 for c in range(n)])
    p = tfp_lib.params(1, 0.001)
    lv = tfp_lib.Live(engine, 2, 12 * T)
    hist = [np.zeros(0, np.int16) for _ in range(2)]
    for k, scopes in ((1, [1, 0]), (32, [0, -1])):
        lv.reset()
        hist = [np.zeros(0, np.int16) for _ in range(2)]
        for t in range(12):
            rows = L.check_push(tfp_lib, engine, lv, hist, src[:, t * T:(t + 1) * T], p, scopes, k, where=(k, t))
        if k == 1:
            assert rows[0][0]["audio_uuid"] == uuids[1023] and rows[1][0]["audio_uuid"] == uuids[1024]
        else:
            assert [r["audio_uuid"] for r in rows[0]] == [uuids[c] for c in range(1024, 1024 - 64, -2)]
            assert [r["audio_uuid"] for r in rows[1]] == [uuids[c] for c in range(1099, 1099 - 32, -1)]
    st = lv.stats()
    assert st["incremental_pushes"] == 24 and st["general_pushes"] == 0 and st["rebuilds"] == 1
    lv.close()
    L.build_db(tfp_lib, engine)  # the module's DB back for the tests that follow


@pytest.mark.parametrize("tol", [0.001, 0.1])
def test_coefs_2_takes_the_general_form(engine, tfp_lib, oracle, db, tol):
    ticks = 24
    src = L.calls(tfp_lib, db, ticks * T)
    p = tfp_lib.params(2, tol)
    lv = tfp_lib.Live(engine, 8, ticks * T)
    hist, _ = _run_ticks(tfp_lib, engine, lv, src, p, L.SCOPES8, 3, ticks)
    st = lv.stats()
    assert st["general_pushes"] == ticks and st["incremental_pushes"] == 0 and st["rebuilds"] == 0
    rows, _ = lv.push(np.zeros((8, 1), np.int16), p, L.SCOPES8, 3, nsamples=[0] * 8)
    for c in (0, 3, 7):
        assert R.pairs(rows[c]) == L.oracle_rows(oracle, db, hist[c], tol, L.SCOPES8[c], 3, coefs=2), c
    lv.close()


def test_resets_capacity_and_argument_errors(engine, tfp_lib, db):
    src = L.calls(tfp_lib, db, 30 * T)
    p = tfp_lib.params(1, 0.45)
    cap = 20 * T + 7
    lv = tfp_lib.Live(engine, 8, cap)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    for t in range(12):
        if t == 7:  # a new call on channel 2 while the others go on
            lv.reset(2)
            hist[2] = np.zeros(0, np.int16)
        L.check_push(tfp_lib, engine, lv, hist, src[:, t * T:(t + 1) * T], p, L.SCOPES8, 3, where=t)
    assert lv.samples(2) == 5 * T and lv.samples(3) == 12 * T
    # past max_samples: all or nothing, for every channel (channel 2 alone would still fit)
    big = src[:, 12 * T:12 * T + 8 * T + 8]
    before = [lv.samples(c) for c in range(8)]
    with pytest.raises(tfp_lib.TfpError) as ei:
        lv.push(big, p, L.SCOPES8, 3)
    assert ei.value.code == TFP_E_CAPACITY
    with pytest.raises(tfp_lib.TfpError) as ei:
        lv.push(big, None)
    assert ei.value.code == TFP_E_CAPACITY
    assert [lv.samples(c) for c in range(8)] == before
    n = [cap - before[c] if c != 2 else 3 for c in range(8)]  # exactly to the capacity
    L.check_push(tfp_lib, engine, lv, hist, big[:, :8 * T + 7], p, L.SCOPES8, 3, nsamples=n, where="fill")
    assert lv.samples(0) == cap
    st = lv.stats()
    assert st["incremental_pushes"] == 13 and st["general_pushes"] == 0 and st["rebuilds"] == 1
    blk = src[:, :T]
    for kw in ({"k": 0}, {"k": 33}, {"scopes": [-2] + [0] * 7}, {"nsamples": [T + 1] + [0] * 7}, {"nsamples": [-1] + [0] * 7}):
        with pytest.raises(tfp_lib.TfpError) as ei:
            lv.push(blk, p, **{"scopes": L.SCOPES8, "k": 3, "nsamples": [0] * 8, **kw})
        assert ei.value.code == TFP_E_ARG, kw
    assert [lv.samples(c) for c in range(8)] == [cap if c != 2 else before[2] + 3 for c in range(8)]
    # invalid params ingest and give empty rows (fp_handler.c:247-250)
    lv.reset()
    rows, fc = lv.push(blk, tfp_lib.params(3, 0.45), L.SCOPES8, 3)
    assert rows == [[]] * 8 and fc == [1] * 8 and lv.samples(5) == T
    lv.close()
    for bad in (0, 65535 * 256 + 1, -5):
        with pytest.raises(tfp_lib.TfpError) as ei:
            tfp_lib.Live(engine, 8, bad)
        assert ei.value.code == TFP_E_ARG
    tfp_lib.Live(engine, 1, 65535 * 256).close()  # the greatest capacity is accepted


def test_ingest_only_pushes_then_one_searching_push(engine, tfp_lib, db):
    src = L.calls(tfp_lib, db, 20 * T)
    p = tfp_lib.params(1, 0.001)
    lv = tfp_lib.Live(engine, 8, 20 * T)
    hist = [np.zeros(0, np.int16) for _ in range(8)]
    for t in range(19):
        assert lv.push(src[:, t * T:(t + 1) * T], None) is None
        for c in range(8):
            hist[c] = np.concatenate([hist[c], src[c, t * T:(t + 1) * T]])
    assert lv.stats()["frames_added"] == 0
    L.check_push(tfp_lib, engine, lv, hist, src[:, 19 * T:], p, L.SCOPES8, 32, where="catch up")
    st = lv.stats()
    assert st["incremental_pushes"] == 1 and st["rebuilds"] == 1 and st["general_pushes"] == 0
    assert st["frames_added"] == 8 * (20 * T // 256)
    lv.close()
